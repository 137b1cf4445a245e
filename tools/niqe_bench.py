"""Time NIQE (csrc/niqe.hip) on a clip of uint8 frames.  Nothing here is a gate.

Event-bracketed medians of ``niqe.niqe`` (features + stats + the host distance, with its device-to-host copy), of ``ops.niqe_features``
(the two block launches and the solve) and of ``ops.niqe_stats``, with the input rate those reach and the floor from the bytes the path has
to move: the uint8 input once, the fp64 half-scale image written once and read once, at the 6.29 TB/s a float4 copy reaches on this chip
(docs/measurement.md).  Per-kernel times come from a kernel trace taken in a run of its own; ``--kernel-stats`` reads its table:

    python tools/niqe_bench.py [--size 720x1280 --frames 33 --reps 20]
    rocprofv3 --kernel-trace --stats -d DIR -o niqe -- python tools/niqe_bench.py --reps 5
    python tools/niqe_bench.py --kernel-stats DIR/.../niqe_kernel_stats.csv

Prints one JSON line."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12                                             # bytes / s, measured float4 copy (docs/measurement.md)


def traffic(n, h, w):
    """Bytes the path has to move for n frames of h x w x 3 uint8: the cropped input once, I2 (fp64, a quarter of the pixels) written and read."""
    hc, wc = (h // 96) * 96, (w // 96) * 96
    return {"input": n * hc * wc * 3, "i2_write": n * hc * wc * 2, "i2_read": n * hc * wc * 2}


def kernel_stats(path):
    """rocprofv3 --stats table -> {kernel: {calls, total_ms, average_us}} for the NIQE kernels."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "niqe_" in name:                                 # e.g. "void (anonymous namespace)::niqe_block_kernel<true>(...)"
                out[name[name.index("niqe_"):].split("(")[0]] = {
                    "calls": int(row["Calls"]), "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3),
                    "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
    return out


def median_ms(fn, reps):
    import torch
    fn()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return sorted(ts)[len(ts) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=str, default="720x1280")
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-stats", type=str, default="", help="a rocprofv3 --stats kernel table of an earlier run: print its NIQE rows")
    args = ap.parse_args(argv)
    h, w = (int(v) for v in args.size.lower().split("x"))
    bytes_ = traffic(args.frames, h, w)
    total = sum(bytes_.values())
    out = {"clip": [args.frames, h, w], "bytes": bytes_, "floor_ms": round(total / COPY_RATE * 1e3, 4)}
    if args.kernel_stats:
        out["kernels"] = kernel_stats(args.kernel_stats)
        print(json.dumps(out))
        return out
    import numpy as np
    import torch

    from dove_amd import niqe, ops
    if not torch.cuda.is_available():
        raise RuntimeError("niqe_bench measures on the GPU; no HIP device is visible")
    g = torch.Generator(device="cuda").manual_seed(0)
    clip = torch.randint(0, 256, (args.frames, h, w, 3), device="cuda", dtype=torch.uint8, generator=g)
    x = clip.permute(0, 3, 1, 2)
    rng = np.random.default_rng(0)
    a = rng.standard_normal((36, 36))
    model = niqe.NiqeModel(rng.standard_normal(36), a @ a.T / 36 + 0.1 * np.eye(36))
    feats, _ = ops.niqe_features(x)
    ms = {"niqe": median_ms(lambda: niqe.niqe(model, clip), args.reps),
          "features": median_ms(lambda: ops.niqe_features(x), args.reps),
          "stats": median_ms(lambda: ops.niqe_stats(feats), args.reps)}
    out["ms"] = {k: round(v, 4) for k, v in ms.items()}
    out["input_gb_per_s"] = {k: round(bytes_["input"] / (ms[k] * 1e-3) / 1e9, 1) for k in ("niqe", "features")}
    out["moved_gb_per_s_features"] = round(total / (ms["features"] * 1e-3) / 1e9, 1)
    out["share_of_floor_features"] = round(out["floor_ms"] / ms["features"], 3)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
