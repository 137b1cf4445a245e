"""MANIQA without a GPU (dove_amd/maniqa.py): the checkpoint's shapes, packing and loader, the crop grid, the restatement's
(tests/maniqa_ref.py) reshape quirk, the conditions that keep the GPU gates from being blind, the new exports and the command line."""
import json
import os
import re

import numpy as np
import pytest
import torch

import maniqa_ref as R
from dove_amd import lib as L
from dove_amd import maniqa as Q
from dove_amd import ops
from test_musiq_cpu import images

# The tiny network of the GPU tests: 4 x 4 tokens (T = 16: every GEMM over the token axis is one short K step), C = 256 channel rows (two
# row tiles of the GEMM, one of them whole), windows of 2 x 2 = 4 tokens (a quarter-filled attention tile) with shift 1, Swin heads of 32
# (two of them) and of 32 (one), 4 crops on a 2 x 2 grid.  Block 5 is in the checkpoint and never run.
TINY = {"side": 32, "patch": 8, "dim": 64, "heads": 1, "blocks": 6, "hooks": (1, 2, 3, 4), "mlp_ratio": 4, "window": 2,
        "swin_heads": (2, 1), "swin_layers": 1, "swin_depth": 2, "dim_mlp": 32, "crops": 4}
SIZE = (40, 48)
_CACHE = {}


def state(cfg=None, seed=5):
    key = ("sd", "tiny" if cfg is None else "real", seed)
    if key not in _CACHE:
        _CACHE[key] = Q.random_state(TINY if cfg is None else cfg, seed, all_blocks=True)
    return _CACHE[key]


def reference():
    """The restatement on the tiny network and ``images(*SIZE)``, computed once and shared with tests/test_maniqa_gpu.py."""
    if "ref" not in _CACHE:
        x, probes = images(*SIZE), {}
        s64 = R.maniqa(x, state(), TINY, torch.float64, Q.TAB_RESHAPE_QUIRK, Q.SWIN_SCALE, Q.NUM_TAB, probes)
        s32 = R.maniqa(x, state(), TINY, torch.float32, Q.TAB_RESHAPE_QUIRK, Q.SWIN_SCALE, Q.NUM_TAB)
        _CACHE["ref"] = {"x": x, "s64": s64, "s32": s32.double(), "probes": probes}
    return _CACHE["ref"]


# ---- shapes, packing and the loader -----------------------------------------------------------------------------------------------------
def test_configuration_and_shapes():
    s = Q.param_shapes()
    assert s["vit.patch_embed.proj.weight"] == (768, 3, 8, 8) and s["vit.pos_embed"] == (1, 785, 768) and s["vit.cls_token"] == (1, 1, 768)
    assert s["vit.blocks.9.attn.qkv.weight"] == (2304, 768) and "vit.blocks.10.norm1.weight" not in s and "vit.norm.weight" not in s
    assert s["tablock1.1.c_k.weight"] == (784, 784) and s["tablock2.0.c_v.bias"] == (784,)
    assert s["conv1.weight"] == (768, 3072, 1, 1) and s["conv2.weight"] == (384, 768, 1, 1)
    assert s["swintransformer1.layers.0.blocks.1.attn.relative_position_bias_table"] == (49, 4)
    assert s["swintransformer1.layers.0.blocks.0.mlp.fc1.weight"] == (768, 768) and s["swintransformer2.layers.0.blocks.1.attn.qkv.weight"] == (1152, 384)
    assert "swintransformer1.layers.1.blocks.0.norm1.weight" not in s
    assert s["fc_score.0.weight"] == (384, 384) and s["fc_weight.3.weight"] == (1, 384)
    full = Q.param_shapes(all_blocks=True)
    assert full["vit.blocks.11.mlp.fc2.weight"] == (768, 3072) and full["vit.norm.bias"] == (768,) and set(s) < set(full)
    assert (Q.NUM_CROPS, Q.NUM_TAB, Q.TAB_RESHAPE_QUIRK, Q.SWIN_SCALE, Q.CFG["crops"]) == (20, 2, True, 0.8, 20)
    # the C = 3072 score matrix is 37.7 MB per crop, 76 MB with the rows and their q, k, v: two frames of 20 crops under 4 GiB
    per_crop = 4 * 3072 * (3072 + 4 * 784)
    assert Q.group_size() == (4 << 30) // (20 * per_crop) == 2 and Q.group_size(budget=1) == 1 and Q.group_size(TINY) > 100
    for bad in ({"heads": 6}, {"swin_heads": (3, 4)}, {"hooks": (6, 7, 8, 12)}, {"dim_mlp": 100}, {"swin_heads": (2, 1)}):
        with pytest.raises(ValueError, match="unsupported configuration"):
            Q.param_shapes({**Q.CFG, **bad})


def test_packing_and_loader(tmp_path):
    sd = state()
    assert "vit.blocks.5.attn.qkv.weight" in sd and "vit.norm.weight" in sd                     # the unused ViT keys are there ...
    extra = {**sd, "swintransformer1.layers.0.blocks.1.attn_mask": torch.zeros(4, 4, 4), "vit.head.weight": torch.zeros(10, 64)}
    torch.save({"params": {"module." + k: v for k, v in extra.items()}}, tmp_path / "maniqa_tiny.pth")
    W = Q.ManiqaWeights.load(str(tmp_path), TINY)                                              # ... and load, with buffers and a ViT head
    P = W.params
    assert W.cfg == TINY and not any(k.startswith("vit.blocks.5") or k.startswith("vit.norm") for k in P)
    assert tuple(P["patch.weight"].shape) == (1, 1, 192, 64) and torch.equal(P["patch.weight"][0, 0], sd["vit.patch_embed.proj.weight"].flatten(1).t())
    assert tuple(P["pos"].shape) == (17, 64) and tuple(P["cls"].shape) == (64,)
    assert torch.equal(P["vit.blocks.2.attn.qkv.weight"][0, 0], sd["vit.blocks.2.attn.qkv.weight"].t())
    assert torch.equal(P["conv1.weight"], sd["conv1.weight"].flatten(1)) and tuple(P["conv2.weight"].shape) == (32, 64)
    assert tuple(P["swintransformer1.layers.0.blocks.1.attn.relative_position_bias_table"].shape) == (9, 2)
    # packed q, k, v equal the separate Linears in fp64, for a TABlock and for a ViT block
    x = torch.randn(5, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    got = x @ P["tablock2.1.qkv.weight"].double() + P["tablock2.1.qkv.bias"].double()
    want = torch.cat([R._lin(x, sd, f"tablock2.1.{n}", torch.float64) for n in ("c_q", "c_k", "c_v")], 1)
    assert tuple(P["tablock2.1.qkv.weight"].shape) == (16, 48) and P["tablock2.1.qkv.weight"].is_contiguous()
    assert float((got - want).abs().max()) < 1e-12                                              # one GEMM or three: the summation order is the BLAS's
    t = torch.randn(3, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    got = t @ P["vit.blocks.0.attn.qkv.weight"][0, 0].double() + P["vit.blocks.0.attn.qkv.bias"].double()
    assert float((got - R._lin(t, sd, "vit.blocks.0.attn.qkv", torch.float64)).abs().max()) < 1e-12
    h = torch.randn(3, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    got = h @ P["head.hidden.weight"][0, 0].double() + P["head.hidden.bias"].double()
    want = torch.cat([R._lin(h, sd, "fc_score.0", torch.float64), R._lin(h, sd, "fc_weight.0", torch.float64)], 1)
    assert float((got - want).abs().max()) < 1e-12 and torch.equal(P["head.w.weight"], sd["fc_weight.3.weight"].flatten())
    # refusals, by name
    for name, pattern in (("tablock1.0.c_k.weight", r"tablock1\.0\.c_k\.weight is missing"), ("vit.blocks.4.norm2.bias", r"vit\.blocks\.4\.norm2\.bias is missing")):
        bad = dict(sd)
        del bad[name]
        with pytest.raises(ValueError, match=pattern):
            Q.ManiqaWeights.from_state_dict(bad, TINY)
    bad = dict(sd)
    bad["conv2.weight"] = torch.zeros(32, 64, 3, 3)
    with pytest.raises(ValueError, match=r"conv2\.weight has shape \(32, 64, 3, 3\)"):
        Q.ManiqaWeights.from_state_dict(bad, TINY)
    with pytest.raises(ValueError, match="has shape"):                                          # a tiny file is no MANIQA checkpoint
        Q.ManiqaWeights.from_state_dict(sd)
    with pytest.raises(TypeError, match="ManiqaWeights"):
        Q.maniqa(object(), torch.zeros(1, 3, 224, 224))
    with pytest.raises(TypeError, match="ManiqaWeights"):
        Q.ManiqaMetric(object())
    m = Q.ManiqaMetric(W)
    assert m.metric_name == "maniqa" and m.lower_better is False and m.full_reference is False


# ---- the crop grid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(224, 224), (224, 225), (720, 1280), (2880, 5120)], ids=lambda s: "%dx%d" % s)
def test_crop_origins(hw):
    H, W = hw
    o = Q.crop_origins(H, W)
    assert o.dtype == np.int32 and o.shape == (Q.NUM_CROPS, 2) == (20, 2)
    assert o.min() >= 0 and (o[:, 0] + 224).max() <= H and (o[:, 1] + 224).max() <= W
    assert [tuple(r) for r in o] == R.crop_origins(H, W, 224, 20)
    if hw == (224, 224):
        assert not o.any()
    if hw == (224, 225):
        assert not o.any()                                                                      # a step of (225 - 224) // 4 = 0
    if hw == (720, 1280):
        assert tuple(o[0]) == (0, 0) and tuple(o[1]) == (0, 264) and tuple(o[5]) == (124, 0) and tuple(o[19]) == (372, 1056)
        assert len({tuple(r) for r in o}) == 20
    t = Q.crop_origins(40, 48, 32, 4)
    assert [tuple(r) for r in t] == [(0, 0), (0, 8), (4, 0), (4, 8)]
    for fn in (lambda: Q.crop_origins(223, 400), lambda: Q.crop_origins(400, 200)):
        with pytest.raises(ValueError, match="smaller than the 224 x 224 crop"):
            fn()


# ---- the reshape quirk ------------------------------------------------------------------------------------------------------------------
def test_tab_reshape_quirk():
    sd = state()
    x = torch.randn(2, 24, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(4))   # C = 24, N = 16: not square
    q, k, v = (R._lin(x, sd, f"tablock1.0.{n}", torch.float64) for n in ("c_q", "c_k", "c_v"))
    y = ((q @ k.transpose(1, 2)) * 16 ** -0.5).softmax(-1) @ v
    plain = y + x
    quirk = y.transpose(1, 2).contiguous().view(2, 24, 16) + x                                  # the dense [N,C] buffer read as [C,N]
    assert torch.equal(R.tablock(x, sd, "tablock1.0", torch.float64, quirk=False), plain)
    assert torch.equal(R.tablock(x, sd, "tablock1.0", torch.float64, quirk=True), quirk)
    assert float((quirk - plain).abs().max()) > 0.1
    assert quirk[0, 0, 1] == y[0, 1, 0] + x[0, 0, 1] and quirk[0, 1, 8] == y[0, 0, 1] + x[0, 1, 8]   # flat index n C + c, read as c' N + n'


# ---- the random state -------------------------------------------------------------------------------------------------------------------
def test_random_state_is_not_degenerate():
    """Conditions under the fp64 restatement that keep the GPU gates from being blind.  The three noise levels' scores differ pairwise by
    at least 100 x the restatement's own fp32-vs-fp64 deviation of the score (tests/test_musiq_cpu.py's rule).  Of every softmax matrix
    (4 TABlocks, 4 Swin blocks) the mean over rows of the largest probability lies in [2 / n, 0.9] for rows of n entries: a uniform
    softmax has 1 / n, a one-hot one 1.  Seen: TABlocks at C = 256 0.04 and 0.07 (uniform: 0.004), at C = 64 0.63 and 0.87 (0.016), Swin
    blocks 0.57 to 0.78 (0.25).  Every crop's sum of weights over its 16 positions is at least 0.01, so that the division amplifies an
    error of the two sums by at most 100 (seen: from 0.06)."""
    ref = reference()
    dev = float((ref["s32"] - ref["s64"]).abs().max())
    diffs = [abs(float(ref["s64"][i] - ref["s64"][j])) for i, j in ((0, 1), (0, 2), (1, 2))]
    print(f"scores {ref['s64'].tolist()}, fp32-vs-fp64 {dev:.3e}, score differences {diffs}")
    assert dev > 0 and min(diffs) >= 100 * dev
    pr = ref["probes"]
    assert len(pr["tab"]) == 4 and len(pr["swin"]) == 4 and len(pr["w"]) == 1
    for kind in ("tab", "swin"):
        for a in pr[kind]:
            n, peak = a.shape[-1], float(a.max(-1).values.mean())
            print(f"{kind} softmax {tuple(a.shape)}: mean row maximum {peak:.3f} (uniform {1 / n:.4f})")
            assert 2.0 / n <= peak <= 0.9
    low = float(pr["w"][0].min())
    print(f"smallest sum of weights {low:.3f}")
    assert low >= 0.01


# ---- the library ------------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ("dove_bmm_f32", "dove_bmm_f32_tiles", "dove_bmm_f32_kernel_name", "dove_softmax_rows_f32", "dove_window_attention_f32",
               "dove_window_attention_tiles", "dove_maniqa_crops_f32", "dove_maniqa_tokens_f32", "dove_mix_f32", "dove_maniqa_score")


def test_exports_and_argument_checks():
    """The header declares the new entry points, lib.py binds them, the library built for gfx950 exports them, each refuses bad arguments
    before any HIP call, and the queries need no device."""
    import test_abi
    assert set(NEW_EXPORTS) <= set(test_abi.header_symbols())
    plain = {"dove_bmm_f32_tiles", "dove_bmm_f32_kernel_name", "dove_window_attention_tiles"}
    assert plain <= set(L.PLAIN) and set(NEW_EXPORTS) - plain <= set(L.SIGNATURES)
    with open(os.path.join(test_abi.ROOT, "dove_amd", "csrc", "build.sh")) as f:
        assert re.search(r'SRCS="[^"]*\bmaniqa\b', f.read())
    if not os.path.exists(L.LIB_PATH):                                      # hipcc --offload-arch=gfx950 needs no GPU
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    assert lib.dove_abi_version() == 15
    assert ops.bmm_f32_tiles() == (128, 128, 32) and ops.window_attention_tiles() == (32, 64, 192)
    names = {ops.bmm_f32_kernel_name(bt, tr) for bt in (False, True) for tr in (False, True)}
    assert len(names) == 4 and all(n.startswith("bmm_f32_kernel") for n in names)
    assert lib.dove_bmm_f32(None, 4, 0, None, 4, 0, None, None, 0, 0, None, 4, 0, 1, 1, 4, 4, 1.0, 0, None) == -1
    assert b"dove_bmm_f32" in lib.dove_last_error()
    assert lib.dove_softmax_rows_f32(None, 1, 1, 1, None, 1, None) == -1 and b"dove_softmax_rows_f32" in lib.dove_last_error()
    assert lib.dove_window_attention_f32(None, None, None, 96, 1, 4, 1, 32, 1.0, None, 9, None, None, 1, None, 32, None) == -1
    assert b"dove_window_attention_f32" in lib.dove_last_error()
    assert lib.dove_maniqa_crops_f32(None, 1, 3, 32, 32, None, 4, 32, 8, None, None) == -1 and b"dove_maniqa_crops_f32" in lib.dove_last_error()
    assert lib.dove_maniqa_tokens_f32(None, None, None, 1, 16, 64, None, None) == -1 and b"dove_maniqa_tokens_f32" in lib.dove_last_error()
    assert lib.dove_mix_f32(None, 4, 0, None, 0, 0, 1.0, 1, 4, 4, 0, None, 4, 0, None) == -1 and b"dove_mix_f32" in lib.dove_last_error()
    assert lib.dove_maniqa_score(None, 64, 1, 4, 16, 32, None, None, None, None, None, None, None) == -1 and b"dove_maniqa_score" in lib.dove_last_error()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_eval_writes_the_json_and_names_the_small_clip(tmp_path, capsys):
    pred = tmp_path / "pred"
    pred.mkdir()
    rng = np.random.default_rng(0)
    np.save(pred / "good.npy", rng.integers(0, 256, (3, 224, 230, 3), dtype=np.uint8))
    np.save(pred / "small.npy", np.zeros((2, 100, 100, 3), dtype=np.uint8))
    seen = []

    def stub(frames):
        seen.append(tuple(frames.shape))
        return [0.25, 0.5, 0.61239]

    out = Q.main(["eval", "--pred", str(pred), "--metric_weights", "unused", "--out", str(tmp_path / "o")], score_fn=stub)
    text = capsys.readouterr().out
    assert seen == [(3, 224, 230, 3)]
    assert out == {"per_sample": {"good": {"maniqa": 0.4541}}, "average": {"maniqa": 0.4541}, "count": 1}
    assert "Error processing small" in text and "100 x 100 are smaller than the 224 x 224 crop" in text
    with open(tmp_path / "o" / "metrics_maniqa.json") as f:
        assert json.load(f) == out


def test_command_lines_name_the_missing_file(tmp_path):
    for cmd in ("score", "eval"):
        with pytest.raises(FileNotFoundError, match=r"no file matching maniqa\*\.pth or ckpt_koniq10k\*\.pt in "):
            Q.main([cmd, "--pred", str(tmp_path), "--metric_weights", str(tmp_path)])
    with pytest.raises(SystemExit):
        Q.main(["score", "--pred", str(tmp_path)])
