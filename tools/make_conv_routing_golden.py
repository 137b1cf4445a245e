#!/usr/bin/env python3
"""Record which kernel dove_convnet_conv_f32 and dove_resnet_conv_f32 choose over a grid that crosses every routing rule.

    tools/make_conv_routing_golden.py            writes tests/golden/conv_f32_routing.json

Run it at the revision whose routing is to be kept (the two _kernel_name functions need no device); tests/test_percep_cpu.py
(test_routing_is_as_recorded) replays the file against the built library.  '' is the record of a refused case.  The grid is the product
of the axes below thinned to a few thousand rows: a dense part around the vector walks, and every STEP-th row of the full product.
"""
import ctypes as C, itertools, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dove_amd import lib as L  # noqa: E402

FIELDS = ["entry", "k", "stride", "pad", "cin", "cout", "ldx", "x", "pool", "h", "w"]
ENTRIES = ["dove_convnet_conv_f32", "dove_resnet_conv_f32"]
KS, STRIDES, CINS, COUTS = (1, 3, 5, 7, 11), (1, 2, 3, 4), (3, 31, 32, 48, 64, 96), (30, 32, 64, 96, 124, 128, 132, 260)
LDXS = (lambda c: c, lambda c: c + 1, lambda c: c + 4, lambda c: 2 * c)
IMAGES, STEP = ((1, 1), (2, 2), (9, 140)), (61, 47)


def pads(k):
    return sorted({0, k // 2, k - 1})


def name(lib, row):
    """The kernel name of one row (the replay in tests/test_percep_cpu.py builds its arguments the same way)."""
    entry, k, stride, pad, cin, cout, ldx, x, pool, h, w = row
    a = (L.ConvnetConvF32Args, L.ResnetConvF32Args)[entry]()
    a.x, a.w, a.out = x, 256, 256
    a.n, a.h, a.w_in, a.cin, a.cout, a.stride, a.relu, a.ldx, a.ldo = 2, h, w, cin, cout, stride, 1, ldx, cout
    if entry == 0:
        a.kh, a.kw, a.pad_h, a.pad_w = k, k, pad, pad
    else:
        a.k, a.pool = k, pool
    return getattr(lib, ENTRIES[entry] + "_kernel_name")(C.byref(a)).decode()


def grid():
    rows = set()
    for entry in (0, 1):
        pools = (1, 2) if entry else (1,)
        full = [(entry, k, s, p, ci, co, ld(ci), x, pool, h, w)
                for k, s, ci, co, ld, x, pool, (h, w) in itertools.product(KS, STRIDES, CINS, COUTS, LDXS, (256, 260), pools, IMAGES)
                for p in (pads(k) if entry == 0 else (k // 2,))]
        rows.update(full[::STEP[entry]])
        # dense around the walks that read 16 bytes at a time: every channel count, row stride and alignment at k 1 and 3
        rows.update(r for r in full if r[1] in (1, 3) and r[2] in (1, 2) and r[9:] == (9, 140) and (r[7] == 256 or r[6] == r[4]))
        # the small images at every kernel side
        rows.update(r for r in full if r[2] == 1 and r[4] == 32 and r[5] in (64, 128) and r[6] == 32 and r[7] == 256 and r[9] < 9)
    return sorted(rows)


def main():
    lib = L.load()
    rows = grid()
    names = sorted({name(lib, r) for r in rows})
    out = {"fields": FIELDS + ["name"], "entries": ENTRIES, "names": names, "rows": [list(r) + [names.index(name(lib, r))] for r in rows]}
    path = os.path.join(ROOT, "tests", "golden", "conv_f32_routing.json")
    with open(path, "w") as f:
        f.write(json.dumps(out, separators=(",", ":")).replace("],[", "],\n[") + "\n")
    print("%s: %d rows, %s" % (path, len(rows), {n: sum(1 for r in out["rows"] if names[r[-1]] == n) for n in names}))


if __name__ == "__main__":
    main()
