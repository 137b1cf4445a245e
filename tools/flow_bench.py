"""Time dove_amd.flow.raft_flow (csrc/flow.hip) for one frame pair: the wall time of a call, and the share and rate of its fp32
convolutions (every conv2d_f32 and the all-pairs correlation, 2 * M * N * K FLOP each) against the 155 TFLOP/s the f32-input MFMA
reaches on this chip (docs/measurement.md).  Nothing here is a gate.

hipEvents around CALLS calls after warm-up for the wall time; a second pass brackets each convolution with its own pair of events (read
after one synchronize at the end).  Weights are the rule-generated ones: the time does not depend on their values.  Prints one JSON line.
For the per-kernel table run it under the profiler:

    python tools/flow_bench.py [--size 720x1280 --iters 20 --calls 5]
    rocprofv3 --kernel-trace --stats -d prof_out -- python tools/flow_bench.py --calls 1"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32_MFMA_PEAK = 155e12


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=str, default="720x1280")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args(argv)
    from dove_amd import flow, ops
    h, w = (int(v) for v in args.size.lower().split("x"))
    weights = flow.RaftWeights.from_state_dict(flow.random_raft_state(0)).to("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    img1, img2 = (torch.rand((1, 3, h, w), device="cuda", generator=g) * 2 - 1 for _ in range(2))

    def run():
        return flow.raft_flow(weights, img1, img2, iters=args.iters)

    for _ in range(2):
        run()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.calls):
        run()
    t1.record()
    torch.cuda.synchronize()
    wall_ms = t0.elapsed_time(t1) / args.calls

    records = []                                                 # (flop, start event, end event) per convolution of one call
    conv, pyramid = ops.conv2d_f32, ops.corr_pyramid_f32

    def timed(fn, flop_of):
        def wrapper(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            records.append((flop_of(a, out), s, e))
            return out
        return wrapper

    ops.conv2d_f32 = timed(conv, lambda a, out: 2 * out.numel() * a[1].shape[0] * a[1].shape[1] * a[1].shape[2])
    ops.corr_pyramid_f32 = timed(pyramid, lambda a, out: 2 * out[0].numel() * a[0].shape[3])      # includes the three small pools
    try:
        run()
        torch.cuda.synchronize()
    finally:
        ops.conv2d_f32, ops.corr_pyramid_f32 = conv, pyramid
    flop = sum(r[0] for r in records)
    conv_ms = sum(r[1].elapsed_time(r[2]) for r in records)
    out = {"pair": [h, w], "iters": args.iters, "calls": args.calls, "raft_flow_ms": round(wall_ms, 2), "conv_calls": len(records),
           "conv_tflop": round(flop / 1e12, 3), "conv_ms": round(conv_ms, 2), "conv_tflops": round(flop / conv_ms / 1e9, 1),
           "conv_share_of_f32_mfma_peak": round(flop / (conv_ms * 1e-3) / F32_MFMA_PEAK, 3),
           "workspace_gib": round(flow.workspace_bytes(*(-(-v // 8) * 8 for v in (h, w)), 1) / 2**30, 2)}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
