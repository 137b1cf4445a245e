"""Time the video-compression step (ops.vcodec_roundtrip, csrc/vcodec.hip) on one 16-frame block, split into motion search and the rest
(coding, colour conversion, rate control).  Nothing here is a gate.

A call runs 7 passes (6 QP halvings and the final one) over its groups; every pass searches each P frame once, frame t of all groups in one
launch.  The motion share is timed with the operator on its own in exactly that launch shape: ``groups`` frames per launch,
7 * (gop - 1) launches.  The rest is the whole call minus that.

The search is set against its LDS traffic: per macroblock and candidate wave 16 window rows of two ds_read2_b32 and one ds_read_b32
(10 LDS cycles) plus the block row as a quarter of a ds_read_b128 per unrolled row (4 cycles), four waves per macroblock: 896 LDS cycles,
on 256 CUs at 2.4 GHz.

``--tools`` times the call with an H.264 tool set (names of ops.VCODEC_TOOLS, or ``all``): quarter-sample refinement after every search, one
launch per macroblock anti-diagonal of every I frame, and two edge passes per frame, in each of the 7 passes.  The motion share is the
integer search alone either way.

hipEvents around CALLS calls after warm-up (docs/measurement.md).  Prints one JSON line per size.

    python tools/vcodec_bench.py [--frames 16 --gop 8 --sizes 180x320 720x1280 --bitrate 30000 --calls 5 --tools all]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QP_PASSES = 7                 # csrc/vcodec.hip: 6 halvings of 0..51 and the final pass
LDS_CYCLES_PER_MB = 896
CUS, CLOCK = 256, 2.4e9


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


def clip(frames, h, w):
    """A smooth texture that slides by (1, 2) pixels per frame, plus noise: vectors worth finding and residuals worth coding."""
    g = torch.Generator(device="cuda").manual_seed(0)
    base = torch.rand((1, 3, (h + 64) // 8, (w + 64) // 8), device="cuda", generator=g)
    base = torch.nn.functional.interpolate(base, size=(h + 64, w + 64), mode="bicubic", align_corners=False)[0].permute(1, 2, 0) * 255
    fr = torch.stack([base[t:t + h, 2 * t:2 * t + w] for t in range(frames)])
    return (fr + torch.randn(fr.shape, device="cuda", generator=g) * 3).contiguous()


def bench(frames, h, w, gop, bitrate, calls, tools=()):
    from dove_amd import ops
    x = clip(frames, h, w)
    groups = -(-frames // gop)
    searches = QP_PASSES * (min(gop, frames) - 1)
    out, qp, bits = ops.vcodec_roundtrip(x, bitrate, gop, want_stats=True, tools=tools)
    total = time_ms(lambda: ops.vcodec_roundtrip(x, bitrate, gop, tools=tools), calls)
    ph, pw = -(-h // 16) * 16, -(-w // 16) * 16
    luma = torch.nn.functional.pad(x[:groups + 1, :, :, 1].clamp(0, 255), (0, pw - w, 0, ph - h), mode="replicate").to(torch.uint8).contiguous()
    one = time_ms(lambda: ops.motion_search_u8(luma[1:], luma[:-1]), calls * 10)
    motion = one * searches
    mbs = (ph // 16) * (pw // 16) * groups * searches
    floor = mbs * LDS_CYCLES_PER_MB / (CUS * CLOCK) * 1e3
    return {"clip": [frames, h, w, 3], "gop": gop, "bitrate": bitrate, "tools": list(tools), "calls": calls, "qp": qp.cpu().tolist(), "bits": bits.cpu().tolist(),
            "total_ms": round(total, 3), "motion_ms": round(motion, 3), "rest_ms": round(total - motion, 3),
            "motion_launches": searches, "motion_launch_us": round(one * 1e3, 2), "motion_lds_floor_ms": round(floor, 3),
            "motion_x_floor": round(motion / floor, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--gop", type=int, default=8)
    ap.add_argument("--sizes", type=str, nargs="+", default=["180x320", "720x1280"])
    ap.add_argument("--bitrate", type=int, default=30000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--tools", type=str, nargs="*", default=[], help="H.264 tools of the call: intra16 qpel deblock, or all")
    args = ap.parse_args(argv)
    tools = ["intra16", "qpel", "deblock"] if args.tools == ["all"] else args.tools
    results = []
    for size in args.sizes:
        h, w = (int(v) for v in size.lower().split("x"))
        results.append(bench(args.frames, h, w, args.gop, args.bitrate, args.calls, tools))
        print(json.dumps(results[-1]))
    return results


if __name__ == "__main__":
    main()
