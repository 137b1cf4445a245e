"""Time DOVER (csrc/convnext3d.hip, csrc/swin3d.hip, dove_amd/dover.py) stage by stage.  Nothing here is a gate.

``score_clip()`` runs on one uint8 clip with every operator of ``dove_amd.ops`` that the two walks call wrapped in a pair of events (the
stage timer of tools/musiq_bench.py); a stage's time is the sum over its calls in one pass (the median pass of ``--reps``, after one
warm-up).  The two branches are also timed alone.  The depthwise conv is timed per production map against a floor: the time a device
copy of the same map takes (one read and one write of it, at the copy rate measured here, the median of ``--kernel_reps`` each).
Weights are the rule-generated ones: the time does not depend on their values.  Prints one JSON line.

    python tools/dover_bench.py [--size 720x1280 --frames 100 --reps 3 --kernel_reps 20]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fastvqa_bench import _flops, _label  # noqa: E402
from musiq_bench import Stages  # noqa: E402


def _dover_label(name, args):
    if name == "dwconv3d_f32":
        return f"dwconv {tuple(args[0].shape[1:])}"
    return _label(name, args)


class DoverStages(Stages):
    NAMES = ("vqa_fragments_f32", "vqa_resized_view_f32", "dwconv3d_f32", "linear_f32", "layernorm_f32", "swin3d_window_gather_f32",
             "swin3d_window_attention_f32", "swin3d_window_scatter_f32", "gelu_f32", "swin3d_patch_merge_f32", "vqa_head_f64")
    label, flops = staticmethod(_dover_label), staticmethod(_flops)


def _median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return sorted(times)[len(times) // 2]


def depthwise_table(ops, cfg, reps):
    """Per stage: the depthwise launch on the production map against a device copy of that map."""
    rows = []
    d, h, w = cfg.clip_len // 2, cfg.size[0] // 4, cfg.size[1] // 4
    g = torch.Generator(device="cuda").manual_seed(1)
    for i, c in enumerate(cfg.dims):
        x = torch.randn(1, d, h >> i, w >> i, c, device="cuda", generator=g)
        wt, b, out = torch.randn(3, 7, 7, c, device="cuda", generator=g), torch.randn(c, device="cuda", generator=g), torch.empty_like(x)
        conv = _median_ms(lambda: ops.dwconv3d_f32(x, wt, b, out=out), reps)
        copy = _median_ms(lambda: out.copy_(x), reps)
        rows.append({"map": list(x.shape), "tile": list(ops.dwconv3d_tile(h >> i, w >> i)), "dwconv_us": round(1e3 * conv, 1),
                     "copy_us": round(1e3 * copy, 1), "copy_gb_s": round(2 * x.numel() * 4 / (copy * 1e-3) / 1e9, 1),
                     "times_the_floor": round(conv / copy, 2), "gflop_s": round(2 * 147 * x.numel() / (conv * 1e-3) / 1e9, 1)})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=str, default="720x1280")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel_reps", type=int, default=20)
    args = ap.parse_args(argv)
    from dove_amd import dover as Q
    from dove_amd import fastvqa, ops
    h, w = (int(v) for v in args.size.lower().split("x"))
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (args.frames, h, w, 3), device="cuda", dtype=torch.uint8, generator=g)
    W = Q.DoverWeights.from_state_dict(Q.random_state(Q.DEFAULT, 0)).to("cuda")
    plan = Q.sample_plan(args.frames, h, w, seed=0)
    x = fastvqa.clip_view(frames)
    Q.score_clip(frames, W, plan=plan)                                  # warms every shape up
    torch.cuda.synchronize()
    passes = []
    for _ in range(args.reps):
        with DoverStages(ops) as st:
            v = Q.score_clip(frames, W, plan=plan)
        t = st.table()
        passes.append((sum(r["ms"] for r in t), t))
    passes.sort(key=lambda p: p[0])
    table = passes[len(passes) // 2][1]
    out = {"clip": [args.frames, h, w], "stages": table, "sum_of_stages_ms": round(sum(r["ms"] for r in table), 2),
           "score_clip_ms": round(_median_ms(lambda: Q.score_clip(frames, W, plan=plan), args.reps), 2),
           "technical_ms": round(_median_ms(lambda: fastvqa.score_clip(x, W.technical(), plan=plan["technical"]), args.reps), 2),
           "aesthetic_ms": round(_median_ms(lambda: Q.aesthetic_raw(W, x, plan["aesthetic"]), args.reps), 2),
           "depthwise": depthwise_table(ops, W.cfg, args.kernel_reps), "scores": v}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
