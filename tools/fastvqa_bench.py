"""Time FasterVQA / FAST-VQA (csrc/swin3d.hip, dove_amd/fastvqa.py) stage by stage.  Nothing here is a gate.

``score_clip()`` runs on one uint8 clip with every operator of ``dove_amd.ops`` that the walk calls wrapped in a pair of events (the
stage timer of tools/musiq_bench.py); a stage's time is the sum over its calls in one pass (the median pass of ``--reps``, after one
warm-up).  The Linears carry 2 M N K FLOPs, the window attention 4 N^2 32 per window and head, against the 155 TFLOP/s the f32-input
MFMA reaches on this chip (docs/measurement.md).  Weights are the rule-generated ones: the time does not depend on their values.
Prints one JSON line per variant.

    python tools/fastvqa_bench.py [--variant FasterVQA,FAST-VQA --size 720x1280 --frames 100 --reps 3]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from musiq_bench import Stages  # noqa: E402


def _label(name, args):
    if name == "linear_f32":
        return f"linear {args[1].shape[2]}->{args[1].shape[3]}"
    if name == "swin3d_window_attention_f32":
        return f"window attention N {args[0].shape[1]}, {args[1]} heads"
    return name.replace("swin3d_", "").replace("vqa_", "").replace("_f32", "").replace("_f64", "")


def _flops(name, args):
    if name == "linear_f32":
        return 2.0 * args[0].shape[0] * args[1].shape[2] * args[1].shape[3]
    if name == "swin3d_window_attention_f32":
        w, n, _ = args[0].shape
        return 4.0 * w * args[1] * n * n * 32
    return 0.0


class VqaStages(Stages):
    NAMES = ("vqa_fragments_f32", "linear_f32", "layernorm_f32", "swin3d_window_gather_f32", "swin3d_window_attention_f32",
             "swin3d_window_scatter_f32", "gelu_f32", "swin3d_patch_merge_f32", "vqa_head_f64")
    label, flops = staticmethod(_label), staticmethod(_flops)


def measure(Q, ops, W, frames, reps):
    """-> (stage table of the median pass, wall ms of an unwrapped call, peak activation bytes, (raw, rescaled))."""
    Q.score_clip(frames, W, seed=0)                                     # warms every shape up
    torch.cuda.synchronize()
    passes = []
    for _ in range(reps):
        with VqaStages(ops) as st:
            Q.score_clip(frames, W, seed=0)
        t = st.table()
        passes.append((sum(r["ms"] for r in t), t))
    passes.sort(key=lambda p: p[0])
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    v = Q.score_clip(frames, W, seed=0)
    e.record()
    torch.cuda.synchronize()
    return passes[len(passes) // 2][1], s.elapsed_time(e), torch.cuda.max_memory_allocated() - base, v


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", type=str, default="FasterVQA,FAST-VQA")
    ap.add_argument("--size", type=str, default="720x1280")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args(argv)
    from dove_amd import fastvqa as Q
    from dove_amd import ops
    h, w = (int(v) for v in args.size.lower().split("x"))
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (args.frames, h, w, 3), device="cuda", dtype=torch.uint8, generator=g)
    outs = []
    for name in args.variant.split(","):
        cfg = Q.preset(name)
        W = Q.VqaWeights.from_state_dict(Q.random_state(cfg, 0), cfg).to("cuda")
        table, ms, peak, v = measure(Q, ops, W, frames, args.reps)
        out = {"variant": name, "clip": [args.frames, h, w], "clips": cfg.num_clips, "window": list(cfg.window), "stages": table,
               "sum_of_stages_ms": round(sum(r["ms"] for r in table), 2), "score_clip_ms": round(ms, 2), "raw": v[0],
               "peak_activation_gb": round(peak / 1e9, 3), "clips_per_group": Q.group_size(cfg)}
        print(json.dumps(out))
        outs.append(out)
        del W
    return outs


if __name__ == "__main__":
    main()
