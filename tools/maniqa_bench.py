"""Time MANIQA (csrc/maniqa.hip, dove_amd/maniqa.py) stage by stage.  Nothing here is a gate.

``maniqa()`` runs on one uint8 frame at the real configuration with every operator of ``dove_amd.ops`` that the walk calls wrapped in a
pair of events (the stage timer of tools/musiq_bench.py); a stage's time is the sum over its calls in one pass (the median pass of
``--reps``, after one warm-up).  The production GEMMs of ``bmm_f32`` are timed alone (the median of ``--kernel_reps``) beside ``linear_f32``
at M = 3072, K = N = 768, the fp32 GEMM the metric block had; the window attention is timed per production shape against a device copy
of its operands (one read of QKV and one write of the output, at the copy rate measured here).  Weights are the rule-generated ones: the
time does not depend on their values.  Prints one JSON line.

    python tools/maniqa_bench.py [--size 720x1280 --reps 3 --kernel_reps 20]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dover_bench import _median_ms  # noqa: E402
from musiq_bench import Stages, _flops, _label  # noqa: E402


def _bmm_n(args):
    a, b = args[0], args[1]
    return b.shape[-2] if b.shape[-1] == a.shape[-1] and b.shape[-2] != a.shape[-1] else b.shape[-1]


def _maniqa_label(name, args):
    if name == "bmm_f32":
        batch = max([t.shape[0] for t in args[:2] if t.dim() == 3] or [1])
        return f"bmm {batch} x {args[0].shape[-2]} x {_bmm_n(args)} x {args[0].shape[-1]}"
    if name == "window_attention_f32":
        return f"window attention {tuple(args[0].shape)} / {args[1]} heads"
    if name == "softmax_rows_f32":
        return f"softmax rows of {args[0].shape[1]}"
    if name == "mha_f32":
        return "mha 785 tokens"
    return _label(name, args)


def _maniqa_flops(name, args):
    if name == "bmm_f32":
        batch = max([t.shape[0] for t in args[:2] if t.dim() == 3] or [1])
        return 2.0 * batch * args[0].shape[-2] * _bmm_n(args) * args[0].shape[-1]
    if name == "window_attention_f32":
        w, n, d3 = args[0].shape
        return 4.0 * w * n * n * d3 / 3
    return _flops(name, args)


class ManiqaStages(Stages):
    NAMES = ("maniqa_crops_f32", "linear_f32", "maniqa_tokens_f32", "layernorm_f32", "mha_f32", "gelu_f32", "mix_f32", "bmm_f32",
             "softmax_rows_f32", "swin3d_window_gather_f32", "window_attention_f32", "swin3d_window_scatter_f32", "maniqa_score")
    label, flops = staticmethod(_maniqa_label), staticmethod(_maniqa_flops)


def gemm_table(ops, reps):
    """The four production GEMMs and the shared-weight Linear of one crop, beside linear_f32 at M = 3072, K = N = 768."""
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    rows = []
    for what, M, N, K, bt in (("TAB scores, C = 3072", 3072, 3072, 784, True), ("TAB A v, C = 3072", 3072, 784, 3072, False),
                              ("TAB scores, C = 768", 768, 768, 784, True), ("TAB A v, C = 768", 768, 784, 768, False),
                              ("q, k, v Linears of one crop", 3072, 2352, 784, False)):
        a, b = rnd(M, K), rnd(N, K) if bt else rnd(K, N)
        out = torch.empty(M, N, device="cuda")
        ms = _median_ms(lambda: ops.bmm_f32(a, b, b_transposed=bt, out=out), reps)
        rows.append({"gemm": what, "m_n_k": [M, N, K], "kernel": ops.bmm_f32_kernel_name(bt), "us": round(1e3 * ms, 1),
                     "tflops": round(2.0 * M * N * K / (ms * 1e-3) / 1e12, 1)})
    x, w = rnd(3072, 768), rnd(1, 1, 768, 768)
    out = torch.empty(3072, 768, device="cuda")
    ms = _median_ms(lambda: ops.linear_f32(x, w, out=out), reps)
    rows.append({"gemm": "linear_f32 (the yardstick)", "m_n_k": [3072, 768, 768], "us": round(1e3 * ms, 1),
                 "tflops": round(2.0 * 3072 * 768 * 768 / (ms * 1e-3) / 1e12, 1)})
    ms = _median_ms(lambda: ops.bmm_f32(x, w[0, 0], out=out), reps)
    rows.append({"gemm": "bmm_f32 at the yardstick's shape", "m_n_k": [3072, 768, 768], "us": round(1e3 * ms, 1),
                 "tflops": round(2.0 * 3072 * 768 * 768 / (ms * 1e-3) / 1e12, 1)})
    return rows


def window_table(ops, fastvqa, crops, reps):
    """The window attention of all crops of a frame, per Swin stage, against a device copy of its operands."""
    g = torch.Generator(device="cuda").manual_seed(2)
    index = torch.from_numpy(fastvqa.relative_index((1, 4, 4)).astype("int32")).cuda()
    region = torch.from_numpy(fastvqa.geometry((1, 28, 28), (1, 4, 4), (1, 1), True)["region"]).cuda()
    rows = []
    for dim in (768, 384):
        qkv = torch.randn(crops * 49, 16, 3 * dim, device="cuda", generator=g)
        table = torch.randn(49, 4, device="cuda", generator=g)
        att = _median_ms(lambda: ops.window_attention_f32(qkv, 4, table, index, region=region), reps)
        src, dst = torch.empty(4 * qkv.numel() // 3, device="cuda"), torch.empty(4 * qkv.numel() // 3, device="cuda")
        copy = _median_ms(lambda: dst.copy_(src), reps)                 # reads QKV's bytes and writes the output's, twice over: 8/3 of QKV moved
        floor = copy * 0.5
        rows.append({"qkv": list(qkv.shape), "heads_of": dim // 4, "attention_us": round(1e3 * att, 1), "operand_copy_us": round(1e3 * floor, 1),
                     "times_the_floor": round(att / floor, 2)})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=str, default="720x1280")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel_reps", type=int, default=20)
    args = ap.parse_args(argv)
    from dove_amd import fastvqa, ops
    from dove_amd import maniqa as Q
    h, w = (int(v) for v in args.size.lower().split("x"))
    g = torch.Generator(device="cuda").manual_seed(0)
    frame = torch.randint(0, 256, (1, h, w, 3), device="cuda", dtype=torch.uint8, generator=g)
    W = Q.ManiqaWeights.from_state_dict(Q.random_state(Q.CFG, 0)).to("cuda")
    Q.maniqa(W, frame)                                                  # warms every shape up
    torch.cuda.synchronize()
    passes = []
    for _ in range(args.reps):
        with ManiqaStages(ops) as st:
            v = Q.maniqa(W, frame)
        t = st.table()
        passes.append((sum(r["ms"] for r in t), t))
    passes.sort(key=lambda p: p[0])
    table = passes[len(passes) // 2][1]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = _median_ms(lambda: Q.maniqa(W, frame), args.reps)
    out = {"frame": [h, w], "crops": Q.CFG["crops"], "stages": table, "sum_of_stages_ms": round(sum(r["ms"] for r in table), 2),
           "ms_per_frame": round(ms, 2), "peak_activation_mb": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1),
           "group_size": Q.group_size(), "gemms": gemm_table(ops, args.kernel_reps),
           "window_attention": window_table(ops, fastvqa, Q.CFG["crops"], args.kernel_reps), "score": float(v[0])}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
