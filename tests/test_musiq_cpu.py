"""MUSIQ without a GPU (dove_amd/musiq.py): the token geometry and spatial hash against the restatement's unfold and F.interpolate, the
StdConv standardisation, the checkpoint loader, the compact sequence against pyiqa's padded and masked one, the conditions on the
rule-generated state that keep the GPU gates from being blind, and the plumbing."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import musiq_ref as R
from dove_amd import metrics as M
from dove_amd import musiq as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_SIZES = [(64, 96), (70, 45), (33, 47)]
_CACHE = {}


def state(num_classes=1):
    key = ("sd", num_classes)
    if key not in _CACHE:
        _CACHE[key] = Q.random_musiq_state(31, num_classes)
    return _CACHE[key]


def images(H, W):
    """The three noise levels of tests/test_percep_gpu.py's ``_images``."""
    g = torch.Generator().manual_seed(H * 1000 + W)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(9 * xx + 5 * yy), 0.5 + 0.4 * torch.cos(7 * yy * xx + 1), 0.2 + 0.6 * xx * yy])
    ref = (base + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return torch.stack([(ref + s * torch.randn(3, H, W, generator=g)).clamp(0, 1) for s in (0.02, 0.1, 0.3)]).float()


def reference(size, num_classes=1):
    """The restatement on ``images(*size)``, computed once and shared with tests/test_musiq_gpu.py: scores and token-0 features in fp64 and
    fp32, and the fp64 pre-softmax scores of every block."""
    key = ("ref", size, num_classes)
    if key not in _CACHE:
        x, taps = images(*size), []
        s64, f64 = R.musiq(state(num_classes), x, torch.float64, taps=taps if num_classes == 1 else None)
        s32, f32 = R.musiq(state(num_classes), x, torch.float32)
        _CACHE[key] = {"s64": s64, "f64": f64, "s32": s32.double(), "f32": f32.double(), "taps": taps}
    return _CACHE[key]


def test_build_list_and_header():
    with open(os.path.join(ROOT, "dove_amd", "csrc", "build.sh")) as f:
        assert re.search(r'SRCS="[^"]*\bmusiq\b', f.read())
    with open(os.path.join(ROOT, "include", "dove_hip.h")) as f:
        h = f.read()
    for sym in ("dove_musiq_patches_f32", "dove_musiq_groupnorm_f32", "dove_layernorm_f32", "dove_musiq_embed_f32", "dove_mha_f32",
                "dove_mha_f32_tiles", "dove_gelu_f32", "dove_musiq_score"):
        assert re.search(rf"\b{sym}\s*\(", h), sym
    assert "#define DOVE_ABI_VERSION 15" in h


def _geometry_matches(H, W):
    geo = Q.token_geometry(H, W)
    pat, spatial, scale, mask = R.multiscale_patches(torch.zeros(1, 1, H, W), padded=False)
    tok = geo["tokens"]
    assert bool(mask.all()) and pat.shape[1] == tok.shape[0] == geo["length"] - 1, (H, W)
    assert torch.equal(tok[:, 0].long(), scale) and torch.equal(tok[:, 3].long(), spatial), (H, W)
    first = 0
    for s, ((rh, rw, pt, pl, resized), (ch, cw)) in enumerate(zip(geo["scales"], geo["counts"])):
        want = R.resize(torch.zeros(1, 1, H, W), R.LONGER[s]).shape[-2:] if s < 2 else (H, W)
        assert (rh, rw) == tuple(want) and resized == (s < 2), (H, W, s)
        assert (ch, cw) == (-(-rh // 32), -(-rw // 32)) and (pt, pl) == ((32 * ch - rh) // 2, (32 * cw - rw) // 2)
        rows = tok[first:first + ch * cw]
        assert rows[:, 1].tolist() == [i for i in range(ch) for _ in range(cw)] and rows[:, 2].tolist() == list(range(cw)) * ch
        first += ch * cw
    assert first == tok.shape[0]


def test_token_geometry_matches_the_unfold_and_the_hash():
    for H in range(1, 71):
        for W in (1, 31, 32, 33, 64, 65, 224, 225, 385):
            _geometry_matches(H, W)
    _geometry_matches(720, 1280)
    _geometry_matches(1080, 1920)
    assert Q.token_geometry(720, 1280)["length"] == 1033 == 1 + 28 + 84 + 920
    pos = torch.arange(10, dtype=torch.float32)[None, None]
    for n in range(1, 201):
        assert Q.hash_index(n).tolist() == F.interpolate(pos, size=n, mode="nearest")[0, 0].long().tolist(), n


def test_standardised_weights_match_the_restatement():
    sd = state()
    W = Q.MusiqWeights.from_state_dict(sd)
    for name, cout, cin, k in Q.STEM_CONVS:
        w = sd[f"{name}.weight"].double()
        m, s = w.mean(dim=(1, 2, 3), keepdim=True), w.std(dim=(1, 2, 3), keepdim=True)
        want = (w - m) / (s + 1e-5)
        got = Q.standardise(sd[f"{name}.weight"])
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name
        packed = W.convs[name][0]
        assert tuple(packed.shape) == (k, k, cin, cout) and packed.dtype == torch.float32
        assert torch.equal(packed, want.float().permute(2, 3, 1, 0))                            # rounded once
    x = torch.randn(2, 3, 32, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    a = R.std_conv(F.pad(x, (2, 3, 2, 3)), sd["conv_root.weight"].double(), 2)
    b = F.conv2d(F.pad(x, (2, 3, 2, 3)), Q.standardise(sd["conv_root.weight"]), None, 2)
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())


def test_loader_names_missing_keys_bad_shapes_and_the_file_pattern(tmp_path):
    sd = dict(state())
    W = Q.MusiqWeights.from_state_dict({"params": sd})                                          # the wrapper is unwrapped
    assert W.num_classes == 1 and W.to("cpu") is W
    assert Q.MusiqWeights.from_state_dict(state(10)).num_classes == 10
    bad = dict(sd)
    del bad["block1.gn_proj.bias"]
    with pytest.raises(ValueError, match=r"MUSIQ checkpoint: block1\.gn_proj\.bias is missing"):
        Q.MusiqWeights.from_state_dict(bad)
    bad = dict(sd)
    bad["transformer_encoder.posembed_input.position_emb"] = torch.zeros(1, 49, 384)
    with pytest.raises(ValueError, match=r"position_emb has shape \(1, 49, 384\), expected \(1, 100, 384\)"):
        Q.MusiqWeights.from_state_dict(bad)
    bad = dict(sd)
    del bad["transformer_encoder.transformer.encoderblock_13.attention.query.weight"]
    with pytest.raises(ValueError, match=r"encoderblock_13\.attention\.query\.weight is missing"):
        Q.MusiqWeights.from_state_dict(bad)
    with pytest.raises(FileNotFoundError, match=r"musiq\*\.pth"):
        Q.MusiqWeights.load(str(tmp_path))
    torch.save({"params": sd}, tmp_path / "musiq_koniq_ckpt.pth")
    W2 = Q.MusiqWeights.load(str(tmp_path))
    assert all(torch.equal(W2.params[k], W.params[k]) for k in W.params) and all(torch.equal(W2.convs[k][0], W.convs[k][0]) for k in W.convs)


@pytest.mark.parametrize("size", NET_SIZES, ids=lambda s: "%dx%d" % s)
def test_compact_sequence_equals_the_padded_masked_one(size):
    """Deleting the padding rows changes nothing: a masked key's softmax weight is exactly 0 and only token 0 reaches the head."""
    ref = reference(size)
    s, f = R.musiq(state(), images(*size), torch.float64, padded=False)
    err = float((s - ref["s64"]).abs().max())
    print(f"{size}: compact against padded: {err:.3e}, scores {ref['s64'].tolist()}")
    assert bool(((s - ref["s64"]).abs() <= 1e-12 * ref["s64"].abs()).all())
    assert float((f - ref["f64"]).abs().max()) <= 1e-12 * float(ref["f64"].abs().max())


@pytest.mark.parametrize("size", NET_SIZES, ids=lambda s: "%dx%d" % s)
def test_random_state_is_not_degenerate(size):
    """Conditions under the fp64 restatement that keep the GPU gates from being blind: the three noise levels' scores differ pairwise by at
    least 100 x the restatement's own fp32-vs-fp64 deviation of the score; the pre-softmax scores of blocks 0 and 13 have a standard
    deviation in [0.3, 10] (neither a uniform nor a one-hot softmax); every valid score is above -800, far from the mask fill."""
    ref = reference(size)
    dev = float((ref["s32"] - ref["s64"]).abs().max())
    diffs = [abs(float(ref["s64"][i] - ref["s64"][j])) for i, j in ((0, 1), (0, 2), (1, 2))]
    stds = [float(ref["taps"][b].std()) for b in (0, 13)]
    low = min(float(t.min()) for t in ref["taps"])
    print(f"{size}: fp32-vs-fp64 {dev:.3e}, score differences {diffs}, score std of blocks 0 / 13 {stds}, lowest valid score {low:.2f}")
    assert len(ref["taps"]) == 14 and dev > 0
    assert min(diffs) >= 100 * dev
    assert all(0.3 <= s <= 10 for s in stds)
    assert low > -800


def test_plumbing():
    tokens = Q.token_geometry(720, 1280)["length"] - 1
    assert Q.group_size(720, 1280) == (4 << 30) // (4 * Q.TOKEN_FLOATS * tokens) == 25 and Q.group_size(8000, 8000) == 1
    assert Q.group_size(720, 1280, budget=1) == 1
    assert "musiq" in M.NR_METRICS and M.NR_METRICS[0] == "niqe" and M.NR_METRICS[-1] == "musiq"
    with pytest.raises(NotImplementedError, match="pyiqa"):
        M.create_metric("musiq")
    with pytest.raises(TypeError, match="MusiqWeights"):
        M.create_metric("musiq", weights=object())
    W = Q.MusiqWeights.from_state_dict(state())
    m = M.create_metric("musiq", weights=W)
    assert isinstance(m, Q.MusiqMetric) and m.lower_better is False and m.metric_name == "musiq" and m.eval() is m
    with pytest.raises(TypeError, match="MusiqWeights"):
        Q.musiq(object(), torch.zeros(1, 3, 8, 8))
    from dove_amd import eval_metrics as E
    assert E.load_weights(["psnr", "musiq"], "") == {}
    assert list(E.init_models(["psnr", "musiq"], "cpu")) == ["psnr"]


def test_command_lines_name_the_missing_file(tmp_path):
    """eval_metrics raises FileNotFoundError for an absent checkpoint, as for the other network metrics; the inference command line
    refuses musiq before it builds a model when the directory holds no musiq*.pth, and without --metric_weights as before."""
    from dove_amd import cli
    from dove_amd import eval_metrics as E
    with pytest.raises(FileNotFoundError, match=r"musiq\*\.pth"):
        E.load_weights(["psnr", "musiq"], str(tmp_path))
    with pytest.raises(NotImplementedError, match=r"musiq\*\.pth"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "musiq", "--metric_weights", str(tmp_path)])
    with pytest.raises(NotImplementedError, match="--metric_weights DIR adds") as e:
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "musiq"])
    added = re.split(r", | and ", str(e.value).split("--metric_weights DIR adds ")[1].rstrip(")"))
    assert added == list(M.NETWORK_METRICS + M.NR_METRICS) and added[-1] == "musiq"     # every registered metric that needs weights, by name
