"""Time the trunk convolutions of LPIPS / DISTS (csrc/conv_f32.hip) and the metrics themselves.  Nothing here is a gate.

For one frame pair (two images through the trunk as one batch) every conv layer of VGG16 and AlexNet is timed on both walks of
``dove_convnet_conv_f32``: ``convnet3x3_f32_kernel`` where the shape takes it, and ``conv_f32_kernel`` (the general walk, reached through
``ops.conv2d_f32`` for the 3 x 3 layers, which is the same launch) - each the median of ``--reps`` launches bracketed by events, with the
achieved TFLOP/s (2 * M * N * K) against the 155 TFLOP/s the f32-input MFMA reaches on this chip (docs/measurement.md).  Then the wall time
of ``percep.lpips`` (alex, vgg) and ``percep.dists`` on a clip of ``--frames`` uint8 frames.  Weights are the rule-generated ones: the time
does not depend on their values.  Prints one JSON line.

    python tools/percep_bench.py [--size 720x1280 --frames 33 --reps 5]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32_MFMA_PEAK = 155e12


def median_ms(fn, reps):
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
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    from dove_amd import lib as L
    from dove_amd import ops, percep
    h, w = (int(v) for v in args.size.lower().split("x"))
    g = torch.Generator(device="cuda").manual_seed(0)

    # the trunk layers of one pair: (name, cin, cout, k, stride, pad, input h, input w)
    layers, hh, ww = [], h, w
    for si, stage in enumerate(percep.VGG_STAGES):
        if si:
            hh, ww = hh // 2, ww // 2
        for n, cout, cin in stage:
            layers.append((f"vgg.features.{n}", cin, cout, 3, 1, 1, hh, ww))
    hh, ww = h, w
    for n, cout, cin, k, stride, pad in percep.ALEX_CONVS:
        if n in (3, 6):
            hh, ww = (hh - 3) // 2 + 1, (ww - 3) // 2 + 1
        layers.append((f"alex.features.{n}", cin, cout, k, stride, pad, hh, ww))
        hh, ww = (hh + 2 * pad - k) // stride + 1, (ww + 2 * pad - k) // stride + 1

    table = []
    for name, cin, cout, k, stride, pad, hh, ww in layers:
        x = torch.randn((2, hh, ww, cin), device="cuda", generator=g)
        wt = torch.randn((k, k, cin, cout), device="cuda", generator=g) * (2.0 / (k * k * cin)) ** 0.5
        b = torch.zeros(cout, device="cuda")
        ho, wo = (hh + 2 * pad - k) // stride + 1, (ww + 2 * pad - k) // stride + 1
        out = torch.empty((2, ho, wo, cout), device="cuda")
        flop = 2.0 * 2 * ho * wo * cout * k * k * cin
        row = {"layer": name, "shape": f"{cin}->{cout} k{k} s{stride} @ 2x{hh}x{ww}", "gflop": round(flop / 1e9, 1),
               "kernel": ops.convnet_conv_kernel_name(tuple(x.shape), tuple(wt.shape), stride, (pad, pad))}
        ms = median_ms(lambda: ops.convnet_conv_f32(x, wt, b, stride=stride, pad=(pad, pad), out=out), args.reps)
        row["ms"], row["tflops"] = round(ms, 3), round(flop / ms / 1e9, 1)
        row["share_of_f32_mfma_peak"] = round(flop / (ms * 1e-3) / F32_MFMA_PEAK, 3)
        if row["kernel"] != "conv_f32_kernel":                  # the same call on the general walk's kernel
            ms = median_ms(lambda: ops.conv2d_f32(x, wt, b, act=L.ACT_RELU, out=out), args.reps)
            row["conv_f32_kernel_ms"], row["conv_f32_kernel_tflops"] = round(ms, 3), round(flop / ms / 1e9, 1)
        table.append(row)
        del x, wt, out

    clip = {}
    pred = torch.randint(0, 256, (args.frames, h, w, 3), device="cuda", dtype=torch.uint8, generator=g)
    gt = torch.randint(0, 256, (args.frames, h, w, 3), device="cuda", dtype=torch.uint8, generator=g)
    for name in ("lpips", "lpips-vgg", "dists"):
        if name == "dists":
            W, fn = percep.DistsWeights.from_state_dicts(*percep.random_dists_state(0)).to("cuda"), percep.dists
        else:
            net = "vgg" if name == "lpips-vgg" else "alex"
            W, fn = percep.LpipsWeights.from_state_dicts(*percep.random_lpips_state(0, net), net).to("cuda"), percep.lpips
        fn(W, pred[:1], gt[:1])
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn(W, pred, gt)
        e.record()
        torch.cuda.synchronize()
        clip[name] = round(s.elapsed_time(e), 1)
    vgg = [r for r in table if r["layer"].startswith("vgg")]
    out = {"pair": [h, w], "frames": args.frames, "layers": table,
           "vgg_pair_ms": round(sum(r["ms"] for r in vgg), 2),
           "vgg_pair_tflops": round(sum(r["gflop"] for r in vgg) / sum(r["ms"] for r in vgg), 1),
           "clip_ms": clip, "pairs_per_group": percep.group_size("vgg", h, w)}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
