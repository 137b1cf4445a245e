"""Time the degradation operators (dove_amd.ops, csrc/degrade.hip) one by one on a clip and set each against its memory-traffic floor:
one read of the fp32 input and one write of the output (fp32, or uint8 for JPEG) at the streaming rate measured for gn_apply
(docs/measurement.md: 5.1 TB/s).  The floor ignores the blur's halo re-reads and the JPEG workspace; nothing here is a gate.

hipEvents around CALLS calls after warm-up (docs/measurement.md).  Prints one JSON line per clip size.

    python tools/degrade_bench.py [--frames 33 --sizes 720x1280 1080x1920 --calls 10]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_RATE = 5.1e12      # bytes/s, gn_apply's read + write pass on the whole chip (docs/measurement.md)


def time_ms(fn, calls, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def bench(frames, h, w, calls):
    from dove_amd import degrade, lib as L, ops
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((frames, h, w, 3), device="cuda", generator=g) * 255
    px = frames * h * w * 3
    oh, ow = h // 4, w // 4
    kernels = {k: torch.from_numpy(degrade.blur_kernel("aniso", k, 2.0, 1.0, 0.5).astype(np.float32)).cuda() for k in (7, 13, 21)}
    steps = {f"blur_k{k}": (lambda kk=kern: ops.blur2d(x, kk), 8 * px) for k, kern in kernels.items()}
    for name, mode in (("bilinear", L.RESIZE_BILINEAR), ("bicubic", L.RESIZE_BICUBIC), ("area", L.RESIZE_AREA)):
        steps[f"resize_{name}_quarter"] = (lambda m=mode: ops.resize(x, oh, ow, m), 4 * px + 4 * frames * oh * ow * 3)
    steps["gaussian_colour"] = (lambda: ops.add_gaussian_noise(x, 10.0, False, 1), 8 * px)
    steps["gaussian_gray"] = (lambda: ops.add_gaussian_noise(x, 10.0, True, 1), 8 * px)
    steps["poisson_colour"] = (lambda: ops.add_poisson_noise(x, 1.0, False, 1), 8 * px)
    steps["poisson_gray"] = (lambda: ops.add_poisson_noise(x, 1.0, True, 1), 8 * px)
    steps["jpeg_q75"] = (lambda: ops.jpeg_roundtrip(x, 75), 5 * px)
    out = {"clip": [frames, h, w, 3], "calls": calls}
    for name, (fn, floor_bytes) in steps.items():
        ms = time_ms(fn, calls)
        floor_ms = floor_bytes / STREAM_RATE * 1e3
        out[name] = {"ms": round(ms, 3), "floor_ms": round(floor_ms, 3), "x_floor": round(ms / floor_ms, 1)}
        torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--sizes", type=str, nargs="+", default=["720x1280", "1080x1920"])
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args(argv)
    results = []
    for size in args.sizes:
        h, w = (int(v) for v in size.lower().split("x"))
        results.append(bench(args.frames, h, w, args.calls))
        print(json.dumps(results[-1]))
    return results


if __name__ == "__main__":
    main()
