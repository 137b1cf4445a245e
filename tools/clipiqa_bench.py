"""Time CLIP-IQA (csrc/clipiqa.hip, dove_amd/clipiqa.py) on one frame, stage by stage.  Nothing here is a gate.

One uint8 frame goes through prep, the stem, the four stages, the attention pool and the score; each is the median of ``--reps`` runs
bracketed by events after one warm-up of every shape, with the conv FLOPs of the stage (2 * M * N * K from the shapes, the BatchNorm being
folded) over that time against the 155 TFLOP/s the f32-input MFMA reaches on this chip (docs/measurement.md).  The stages are timed one
after another on the same data, so their sum is the frame.  Weights are the rule-generated ones: the time does not depend on their
values.  The peak of the live activations of one ``clipiqa`` call is reported in floats per input pixel, next to ``group_size``'s 32.
Prints one JSON line.

    python tools/clipiqa_bench.py [--size 720x1280 --reps 5 --frames 33]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32_MFMA_PEAK = 155e12


def conv_flops(h: int, w: int) -> dict:
    """stage -> conv FLOPs of one h x w frame, from the shapes alone."""
    from dove_amd import clipiqa as Q
    hh, ww = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = {"stem": 2.0 * hh * ww * 9 * (3 * 32 + 32 * 32 + 32 * 64)}
    hh, ww = hh // 2, ww // 2
    for p, inplanes, planes, stride, down in Q._blocks():
        name = p.split(".")[1]
        f = hh * ww * (inplanes * planes + 9 * planes * planes)          # conv1 and conv2 run before the pool
        hh, ww = hh // stride, ww // stride
        f += hh * ww * (planes * 4 * planes + (inplanes * 4 * planes if down else 0))
        out[name] = out.get(name, 0.0) + 2.0 * f
    out["attnpool"] = 2.0 * (3 * 2048 * 2048 + 1024 * 2048 + 2 * (hh * ww + 1) * 32 * 2048)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=str, default="720x1280")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=0, help="also time clipiqa() on a clip of this many frames (0: skip)")
    args = ap.parse_args(argv)
    from dove_amd import clipiqa as Q
    from dove_amd import ops
    h, w = (int(v) for v in args.size.lower().split("x"))
    g = torch.Generator(device="cuda").manual_seed(0)
    W = Q.ClipIqaWeights.from_state_dict(*Q.random_clipiqa_state(0)).to("cuda")
    frame = torch.randint(0, 256, (1, h, w, 3), device="cuda", dtype=torch.uint8, generator=g).permute(0, 3, 1, 2)
    steps = [("prep", lambda x: ops.percep_prep_f32(x, 1.0, 0.0, Q.CLIP_MEAN, Q.CLIP_STD)), ("stem", lambda x: Q.stem(W, [x]))]
    steps += [(f"layer{li + 1}", lambda x, li=li: Q.stage(W, [x], li)) for li in range(4)]
    steps += [("attnpool", lambda x: ops.clip_attnpool_f32(x, W.attn)), ("score", lambda x: ops.clipiqa_score(x, W.text[0], W.logit_scale))]
    times = {name: [] for name, _ in steps}
    for rep in range(args.reps + 1):                                    # the first pass warms every shape up and is not counted
        x = frame
        for name, fn in steps:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            x = fn(x)
            e.record()
            torch.cuda.synchronize()
            if rep:
                times[name].append(s.elapsed_time(e))
    med = lambda v: sorted(v)[len(v) // 2]
    flops = conv_flops(h, w)
    table = []
    for name, _ in steps:
        ms = med(times[name])
        row = {"stage": name, "ms": round(ms, 3)}
        if name in flops:
            row.update(gflop=round(flops[name] / 1e9, 1), tflops=round(flops[name] / ms / 1e9, 1),
                       share_of_f32_mfma_peak=round(flops[name] / (ms * 1e-3) / F32_MFMA_PEAK, 3))
        table.append(row)
    whole = Q.clipiqa(W, frame)                                          # the public entry, timed as one call
    torch.cuda.synchronize()
    del x
    base = torch.cuda.memory_allocated()                                 # weights and the frame
    torch.cuda.reset_peak_memory_stats()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    whole = Q.clipiqa(W, frame)
    e.record()
    torch.cuda.synchronize()
    tower = sum(flops[k] for k in flops if k != "attnpool")
    out = {"frame": [h, w], "stages": table, "sum_of_stages_ms": round(sum(r["ms"] for r in table), 2), "clipiqa_call_ms": round(s.elapsed_time(e), 2),
           "tower_gflop": round(tower / 1e9, 1), "tower_tflops": round(tower / sum(r["ms"] for r in table if r["stage"] in flops and r["stage"] != "attnpool") / 1e9, 1),
           "value": float(whole[0]), "frames_per_group": Q.group_size(h, w), "peak_activation_gb": round((torch.cuda.max_memory_allocated() - base) / 1e9, 3),
           "peak_activation_floats_per_pixel": round((torch.cuda.max_memory_allocated() - base) / (4.0 * h * w), 2)}
    if args.frames:
        clip = torch.randint(0, 256, (args.frames, h, w, 3), device="cuda", dtype=torch.uint8, generator=g)
        Q.clipiqa(W, clip)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        Q.clipiqa(W, clip)
        e.record()
        torch.cuda.synchronize()
        out.update(clip_frames=args.frames, clip_ms=round(s.elapsed_time(e), 2), clip_ms_per_frame=round(s.elapsed_time(e) / args.frames, 3),
                   clip_tower_tflops=round(tower * args.frames / s.elapsed_time(e) / 1e9, 1))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
