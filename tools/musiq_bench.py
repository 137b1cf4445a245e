"""Time MUSIQ (csrc/musiq.hip, dove_amd/musiq.py) stage by stage.  Nothing here is a gate.

``musiq()`` runs on one uint8 frame and on a clip of ``--frames`` frames with every operator of ``dove_amd.ops`` that the walk calls wrapped
in a pair of events; a stage's time is the sum over its calls in one pass (the median pass of ``--reps``, after one warm-up), so the stages
add up to the device time of the call.  The GEMM and conv stages carry their FLOPs (2 M N K from the shapes) against the 155 TFLOP/s the
f32-input MFMA reaches on this chip (docs/measurement.md); attention counts 4 T^2 64 per head and frame.  Weights are the rule-generated
ones: the time does not depend on their values.  The peak of the live activations of one call is reported per patch token, next to
``TOKEN_FLOATS``.  Prints one JSON line.

    python tools/musiq_bench.py [--size 720x1280 --reps 3 --frames 33]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32_MFMA_PEAK = 155e12


def _label(name, args):
    if name == "linear_f32":
        return f"linear {args[1].shape[2]}->{args[1].shape[3]}"
    if name in ("resnet_conv_f32", "convnet_conv_f32"):
        k, _, cin, cout = args[1].shape
        return f"conv {k}x{k} {cin}->{cout}"
    if name == "musiq_groupnorm_f32":
        return "groupnorm"
    return name.replace("musiq_", "").replace("_f32", "")


def _flops(name, args):
    if name == "linear_f32":
        return 2.0 * args[0].shape[0] * args[1].shape[2] * args[1].shape[3]
    if name == "convnet_conv_f32":                                      # the stem conv: stride 2 over the 37 x 37 frame
        k, _, cin, cout = args[1].shape
        return 2.0 * args[0].shape[0] * 16 * 16 * k * k * cin * cout
    if name == "resnet_conv_f32":
        k, _, cin, cout = args[1].shape
        return 2.0 * args[0].shape[0] * args[0].shape[1] * args[0].shape[2] * k * k * cin * cout
    if name == "mha_f32":
        n, t, d = args[0].shape
        return 4.0 * n * t * t * d
    return 0.0


class Stages:
    """Wraps the operators for the length of a ``with`` block; ``table()`` after it."""
    NAMES = ("musiq_patches_f32", "convnet_conv_f32", "resnet_conv_f32", "linear_f32", "musiq_groupnorm_f32", "layernorm_f32", "musiq_embed_f32",
             "mha_f32", "gelu_f32", "musiq_score")

    label, flops = staticmethod(_label), staticmethod(_flops)            # a subclass for another network replaces NAMES and these two

    def __init__(self, ops):
        self.ops, self.events, self.saved, self.depth = ops, [], {}, 0

    def _wrap(self, name, fn):
        def timed(*a, **k):
            if self.depth:                                              # linear_f32 calls resnet_conv_f32: counted once, as the Linear
                return fn(*a, **k)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.depth += 1
            s.record()
            try:
                return fn(*a, **k)
            finally:
                e.record()
                self.depth -= 1
                self.events.append((self.label(name, a), self.flops(name, a), s, e))
        return timed

    def __enter__(self):
        for n in self.NAMES:
            self.saved[n] = getattr(self.ops, n)
            setattr(self.ops, n, self._wrap(n, self.saved[n]))
        return self

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(self.ops, n, fn)
        torch.cuda.synchronize()

    def table(self):
        rows = {}
        for label, fl, s, e in self.events:
            r = rows.setdefault(label, {"stage": label, "calls": 0, "ms": 0.0, "gflop": 0.0})
            r["calls"] += 1
            r["ms"] += s.elapsed_time(e)
            r["gflop"] += fl / 1e9
        out = []
        for r in rows.values():
            r["ms"] = round(r["ms"], 3)
            if r["gflop"]:
                r["tflops"] = round(r["gflop"] / r["ms"], 1)
                r["share_of_f32_mfma_peak"] = round(r["gflop"] * 1e9 / (r["ms"] * 1e-3) / F32_MFMA_PEAK, 3)
                r["gflop"] = round(r["gflop"], 1)
            else:
                del r["gflop"]
            out.append(r)
        return out


def measure(Q, ops, W, x, reps):
    """-> (stage table of the median pass, wall ms of an unwrapped call, peak activation bytes, value)."""
    Q.musiq(W, x)                                                       # warms every shape up
    torch.cuda.synchronize()
    passes = []
    for _ in range(reps):
        with Stages(ops) as st:
            Q.musiq(W, x)
        t = st.table()
        passes.append((sum(r["ms"] for r in t), t))
    passes.sort(key=lambda p: p[0])
    table = passes[len(passes) // 2][1]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    v = Q.musiq(W, x)
    e.record()
    torch.cuda.synchronize()
    return table, s.elapsed_time(e), torch.cuda.max_memory_allocated() - base, v


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=str, default="720x1280")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=33, help="also time musiq() on a clip of this many frames (0: skip)")
    args = ap.parse_args(argv)
    from dove_amd import musiq as Q
    from dove_amd import ops
    h, w = (int(v) for v in args.size.lower().split("x"))
    g = torch.Generator(device="cuda").manual_seed(0)
    W = Q.MusiqWeights.from_state_dict(Q.random_musiq_state(0)).to("cuda")
    tokens = Q.token_geometry(h, w)["length"] - 1
    frame = torch.randint(0, 256, (1, h, w, 3), device="cuda", dtype=torch.uint8, generator=g)
    table, ms, peak, v = measure(Q, ops, W, frame, args.reps)
    out = {"frame": [h, w], "tokens": tokens + 1, "stages": table, "sum_of_stages_ms": round(sum(r["ms"] for r in table), 2),
           "musiq_call_ms": round(ms, 2), "value": float(v[0]), "frames_per_group": Q.group_size(h, w),
           "peak_activation_gb": round(peak / 1e9, 3), "peak_activation_floats_per_token": round(peak / (4.0 * tokens), 1),
           "token_floats_of_group_size": Q.TOKEN_FLOATS}
    if args.frames:
        clip = torch.randint(0, 256, (args.frames, h, w, 3), device="cuda", dtype=torch.uint8, generator=g)
        table, ms, peak, _ = measure(Q, ops, W, clip, args.reps)
        per_group = min(args.frames, Q.group_size(h, w)) * tokens
        out.update(clip_frames=args.frames, clip_stages=table, clip_sum_of_stages_ms=round(sum(r["ms"] for r in table), 2),
                   clip_ms=round(ms, 2), clip_ms_per_frame=round(ms / args.frames, 3), clip_peak_activation_gb=round(peak / 1e9, 3),
                   clip_peak_activation_floats_per_token=round(peak / (4.0 * per_group), 1))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
