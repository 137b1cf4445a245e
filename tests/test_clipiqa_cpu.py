"""CLIP-IQA without a GPU (dove_amd/clipiqa.py): the BatchNorm fold, the checkpoint loader, the tokenizer, the text tower, the condition
on the rule-generated state that keeps the GPU gate from being blind, the minimum side, and the plumbing."""
import gzip
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clipiqa_ref as R
from dove_amd import clipiqa as Q
from dove_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_SIZES = [(Q.MIN_SIDE, Q.MIN_SIDE), (67, 95), (128, 160)]
_STATE = {}


def state():
    if not _STATE:
        _STATE["sd"], _STATE["text"] = Q.random_clipiqa_state(31)
    return _STATE["sd"], _STATE["text"]


def images(H, W):
    """The three noise levels of tests/test_percep_gpu.py's ``_images``."""
    g = torch.Generator().manual_seed(H * 1000 + W)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(9 * xx + 5 * yy), 0.5 + 0.4 * torch.cos(7 * yy * xx + 1), 0.2 + 0.6 * xx * yy])
    ref = (base + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return torch.stack([(ref + s * torch.randn(3, H, W, generator=g)).clamp(0, 1) for s in (0.02, 0.1, 0.3)]).float()


def test_build_list_and_header():
    with open(os.path.join(ROOT, "dove_amd", "csrc", "build.sh")) as f:
        assert re.search(r'SRCS="[^"]*\bclipiqa\b', f.read())
    with open(os.path.join(ROOT, "include", "dove_hip.h")) as f:
        h = f.read()
    for sym in ("dove_resnet_conv_f32", "dove_resnet_conv_f32_kernel_name", "dove_avgpool_cl_f32", "dove_clip_attnpool_f32",
                "dove_clip_attnpool_workspace_bytes", "dove_clipiqa_score"):
        assert re.search(rf"\b{sym}\s*\(", h), sym


def test_bn_fold_matches_the_unfolded_bottleneck():
    """One bottleneck with a downsample branch and stride 2: the convs with fp64 folded weights against conv + F.batch_norm in fp64,
    to 1e-12 of the output's largest magnitude."""
    sd, _ = state()
    p = "visual.layer2.0"
    x = torch.randn(2, 256, 9, 11, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    want = R.bottleneck(sd, p, x, 2)
    fold = lambda conv, bn: Q.fold_bn(sd[f"{conv}.weight"], *(sd[f"{bn}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")))
    t = F.relu(F.conv2d(x, *fold(f"{p}.conv1", f"{p}.bn1")))
    t = F.relu(F.conv2d(t, *fold(f"{p}.conv2", f"{p}.bn2"), padding=1))
    t = F.conv2d(F.avg_pool2d(t, 2), *fold(f"{p}.conv3", f"{p}.bn3"))
    got = F.relu(t + F.conv2d(F.avg_pool2d(x, 2), *fold(f"{p}.downsample.0", f"{p}.downsample.1")))
    rel = float((got - want).abs().max() / want.abs().max())
    print(f"BN fold: relative deviation {rel:.3e}")
    assert want.shape == (2, 512, 4, 5) and rel <= 1e-12
    # the packed weights are that fold rounded once
    W = Q.ClipIqaWeights.from_state_dict(*state())
    w64, b64 = fold(f"{p}.conv2", f"{p}.bn2")
    assert torch.equal(W.convs[f"{p}.conv2"][0], w64.float().permute(2, 3, 1, 0)) and torch.equal(W.convs[f"{p}.conv2"][1], b64.float())
    assert W.logit_scale == pytest.approx(100.0, rel=1e-6) and len(W.convs) == 3 + 16 * 3 + 4 and len(W.attn) == 8
    assert torch.allclose(W.text[0].norm(dim=1), torch.ones(10, dtype=torch.float64), atol=1e-15)


def test_loader_rejects_missing_keys_and_bad_shapes(tmp_path):
    sd, text = state()
    shapes = Q.visual_param_shapes()
    assert set(shapes) <= set(sd) and "visual.attnpool.positional_embedding" not in shapes
    for name in shapes:
        bad = dict(sd)
        del bad[name]
        with pytest.raises(ValueError, match=re.escape(f"{name} is missing")):
            Q.ClipIqaWeights.from_state_dict(bad, text)
        bad[name] = torch.zeros(tuple(shapes[name]) + (2,))
        with pytest.raises(ValueError, match=re.escape(f"{name} has shape")):
            Q.ClipIqaWeights.from_state_dict(bad, text)
    with pytest.raises(ValueError, match="clipiqa_text.npz"):
        Q.ClipIqaWeights.from_state_dict(sd)
    with pytest.raises(ValueError, match="text features"):
        Q.ClipIqaWeights.from_state_dict(sd, {"features": np.zeros((3, 1024))})
    # the directory loader: no model, then a model with neither the text file nor a vocabulary, then both files
    with pytest.raises(FileNotFoundError, match="RN50"):
        Q.ClipIqaWeights.load(str(tmp_path))
    torch.save(sd, tmp_path / "RN50.pth")
    with pytest.raises(FileNotFoundError, match=r"clipiqa_text.*bpe_simple_vocab_16e6.*python -m dove_amd.clipiqa text"):
        Q.ClipIqaWeights.load(str(tmp_path))
    Q.save_text(str(tmp_path / "clipiqa_text.npz"), 3.0 * text["features"], text["prompts"], text["logit_scale"])
    W, W0 = Q.ClipIqaWeights.load(str(tmp_path)), Q.ClipIqaWeights.from_state_dict(sd, text)
    assert W.prompts == tuple(p for pair in Q.PROMPTS for p in pair)
    assert torch.allclose(W.text[0], W0.text[0], atol=1e-15) and all(torch.equal(a, b) for a, b in zip(W.attn, W0.attn))
    assert all(torch.equal(W.convs[k][0], W0.convs[k][0]) and torch.equal(W.convs[k][1], W0.convs[k][1]) for k in W0.convs)


def test_torchscript_archive_fallback(tmp_path):
    """OpenAI's RN50.pt is a TorchScript archive, which ``torch.load(weights_only=True)`` refuses: the loader falls back to
    ``torch.jit.load(...).state_dict()``.  Checked on a tiny scripted module."""

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.logit_scale = torch.nn.Parameter(torch.tensor(4.5))
            self.lin = torch.nn.Linear(3, 2)

        def forward(self, x):
            return self.lin(x) * self.logit_scale

    m = Tiny()
    path = str(tmp_path / "RN50.pt")
    torch.jit.script(m).save(path)
    sd = Q._load_sd(path)
    assert set(sd) == {"logit_scale", "lin.weight", "lin.bias"} and torch.equal(sd["lin.weight"], m.lin.weight.detach())
    torch.save(m.state_dict(), path)                                      # a plain state dict takes the first way
    assert torch.equal(Q._load_sd(path)["lin.bias"], m.lin.bias.detach())


WORDS = ["good", "image", "sharp", "edges", "blurry", "noise-free", "resolution", "high", "noisy", "a", "aaaa", "losslessness", "bad",
         "low", "noise", "free", "y", "it", "'s"]


def _merges(n=60):
    """A rule-built merge list, made the way byte-pair vocabularies are: over WORDS, join the most frequent neighbouring pair (ties: the
    first in sorted order), n times.  A rule's parts therefore exist before the rule."""
    byte = Q._bytes_to_unicode()
    corpus = []
    for w in WORDS:
        chars = [byte[b] for b in w.encode()]
        corpus.append(chars[:-1] + [chars[-1] + "</w>"])
    merges = []
    for _ in range(n):
        counts = {}
        for parts in corpus:
            for pair in zip(parts, parts[1:]):
                counts[pair] = counts.get(pair, 0) + 1
        if not counts:
            break
        a, b = min(counts, key=lambda p: (-counts[p], p))
        merges.append((a, b))
        corpus = [R.naive_bpe_step(parts, a, b) for parts in corpus]
    return merges


def test_tokenizer_against_the_naive_encoder(tmp_path):
    """The byte-pair encoder against tests/clipiqa_ref.py's one-rule-at-a-time encoder on a rule-built merge list, the vocabulary file's
    format, and the frame of a token row.  Agreement with CLIP's real vocabulary cannot be checked here: the file is not part of the
    repository (it ships with the ``clip`` package), so the ids of the real prompts are not pinned."""
    merges = _merges()
    path = tmp_path / "vocab.txt.gz"
    with gzip.open(path, "wt", encoding="utf-8") as f:
        f.write('"bpe_simple_vocab_16e6.txt#version: 0.2\n' + "\n".join(" ".join(m) for m in merges) + "\nzz zz\nqq qq\n")
    tok = Q.Tokenizer.from_file(str(path), count=len(merges))           # the lines behind the counted merges are not read
    assert len(tok.rank) == len(merges) and tok.sot == 512 + len(merges) and tok.eot == tok.sot + 1
    real = Q.Tokenizer([])
    assert (real.sot, real.eot) == (512, 513) and Q.SOT == 512 + Q.MERGES and Q.EOT == Q.SOT + 1
    assert real.ids["!"] == 0 and real.ids["a"] == 64 and real.ids["a</w>"] == 256 + 64
    words = WORDS + ["goodness", "images", "freer", "noisier", "sharpedges", "aaaaa", "hi-res"]
    n_merged = 0
    for w in words:
        chars = "".join(tok.byte[b] for b in w.encode())
        got = tok.bpe(chars)
        assert got == R.naive_bpe(chars, merges), w
        assert "".join(got) == chars + "</w>"
        n_merged += len(got) < len(chars)
    assert n_merged >= 6, "the merge list never fired"
    rows = tok(["Good   image", "noise-free IMAGE", ""])
    assert rows.shape == (3, 77) and rows.dtype == torch.int64
    ids = tok.encode("good image")
    assert rows[0, 0] == tok.sot and rows[0, 1:1 + len(ids)].tolist() == ids and rows[0, 1 + len(ids)] == tok.eot
    assert int(rows[0, 2 + len(ids):].abs().sum()) == 0 and int(rows[0].argmax()) == 1 + len(ids)
    assert rows[1].tolist()[1:1 + len(tok.encode("noise-free image"))] == tok.encode("noise") + tok.encode("-") + tok.encode("free image")
    assert rows[2, :3].tolist() == [tok.sot, tok.eot, 0]
    assert [len(tok.encode(w)) for w in ("it's", "a1b")] == [len(tok.encode("it")) + len(tok.encode("'s")), 3]
    with pytest.raises(ValueError, match="context holds 77"):
        tok(["y " * 76])
    assert tok(["y " * 75]).shape == (1, 77)                             # SOT + 75 + EOT fits exactly


def test_text_tower_against_the_restatement():
    """A two-layer, rule-generated text tower: the module's written-out attention against nn.functional's, in fp64."""
    g = torch.Generator().manual_seed(8)
    shapes = {k: v for k, v in Q.text_param_shapes().items() if not re.match(r"transformer\.resblocks\.([2-9]|1\d)\.", k)}
    sd = {k: (torch.randn(s, generator=g, dtype=torch.float64) * (0.02 if len(s) == 2 else 0.1) + (1.0 if k.endswith(("ln_1.weight", "ln_2.weight", "ln_final.weight")) else 0.0))
          for k, s in shapes.items()}
    tokens = torch.zeros(4, 77, dtype=torch.int64)
    for i, n in enumerate((3, 5, 8, 77)):
        tokens[i, :n] = torch.randint(1, 49000, (n,), generator=g)
        tokens[i, 0], tokens[i, n - 1] = Q.SOT, Q.EOT
    old = Q.TEXT_LAYERS
    try:
        Q.TEXT_LAYERS = 2
        got = Q.encode_text(sd, tokens)
    finally:
        Q.TEXT_LAYERS = old
    want = R.text_tower(sd, tokens)
    assert got.shape == (4, 1024) and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # what follows EOT does not reach the features (causal mask, and the row read is EOT's)
    t2 = tokens.clone()
    t2[0, 3:10] = 7
    Q.TEXT_LAYERS = 2
    try:
        assert float((Q.encode_text(sd, t2) - got).abs().max()) <= 1e-12 * float(want.abs().max())
    finally:
        Q.TEXT_LAYERS = old


@pytest.mark.parametrize("size", NET_SIZES, ids=lambda s: "%dx%d" % s)
def test_random_state_does_not_saturate_the_score(size):
    """With exp(logit_scale) = 100 a random state can push every pair softmax to 0 or 1, where the GPU gate on the score would see nothing.
    For the GPU test's images under the fp64 restatement: every pair's |logit difference| <= 3, and the scores of the three noise levels
    differ pairwise by more than 1e-3."""
    sd, text = state()
    s, f, d = R.clipiqa_ref(sd, text, images(*size).double(), want_parts=True)
    print(f"{size}: scores {s.tolist()}, largest |logit difference| {float(d.abs().max()):.3f}")
    assert float(d.abs().max()) <= 3.0
    assert min(abs(float(s[i] - s[j])) for i, j in ((0, 1), (0, 2), (1, 2))) > 1e-3
    assert bool(((s > 0) & (s < 1)).all())


def test_min_side_agrees_with_the_restatement():
    sd, text = state()
    assert Q.MIN_SIDE == 31
    x = torch.rand(1, 3, Q.MIN_SIDE, Q.MIN_SIDE + 1, generator=torch.Generator().manual_seed(1))
    assert tuple(R.visual_features(sd, x).shape) == (1, 2048, 1, 1)
    with pytest.raises((ValueError, RuntimeError)):
        R.clipiqa_ref(sd, text, torch.rand(1, 3, Q.MIN_SIDE - 1, 40))
    with pytest.raises(ValueError, match=f"minimum side is {Q.MIN_SIDE}"):
        Q._images(torch.rand(1, 3, 40, Q.MIN_SIDE - 1))
    for s in (32, 63, 64, 67, 95):
        assert Q._out_side(s) == R.visual_features(sd, torch.zeros(1, 3, s, 31)).shape[2]
    assert (Q._out_side(720), Q._out_side(1280)) == (22, 40)


def test_group_size_and_plumbing():
    assert Q.group_size(720, 1280) == (4 << 30) // (128 * 720 * 1280) == 36 and Q.group_size(2880, 5120) == 2 and Q.group_size(8000, 8000) == 1
    assert "clipiqa" in M.NR_METRICS and M.NR_METRICS[0] == "niqe"
    with pytest.raises(NotImplementedError, match="pyiqa"):
        M.create_metric("clipiqa")
    with pytest.raises(TypeError, match="ClipIqaWeights"):
        M.create_metric("clipiqa", weights=object())
    W = Q.ClipIqaWeights.from_state_dict(*state())
    m = M.create_metric("clipiqa", weights=W)
    assert isinstance(m, Q.ClipIqaMetric) and m.lower_better is False and m.metric_name == "clipiqa"
    assert W.to("cpu") is W
    from dove_amd import eval_metrics as E
    assert E.load_weights(["psnr", "clipiqa"], "") == {}
    assert list(E.init_models(["psnr", "clipiqa"], "cpu")) == ["psnr"]


def test_command_lines_name_the_missing_files(tmp_path):
    """eval_metrics raises FileNotFoundError for an absent checkpoint, as for the other network metrics; the inference command line
    refuses clipiqa before it builds a model when the directory holds no RN50 file, and without --metric_weights as before."""
    from dove_amd import cli
    from dove_amd import eval_metrics as E
    with pytest.raises(FileNotFoundError, match=r"RN50\*\.pt"):
        E.load_weights(["psnr", "clipiqa"], str(tmp_path))
    with pytest.raises(NotImplementedError, match=r"RN50\*\.pt"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "clipiqa", "--metric_weights", str(tmp_path)])
    with pytest.raises(NotImplementedError, match="--metric_weights DIR adds") as e:
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "clipiqa"])
    added = re.split(r", | and ", str(e.value).split("--metric_weights DIR adds ")[1].rstrip(")"))
    assert added == list(M.NETWORK_METRICS + M.NR_METRICS) and "clipiqa" in added     # every registered metric that needs weights, by name
    torch.save({}, tmp_path / "RN50.pt")                                  # accepted now: the loader is reached and names the first key
    with pytest.raises(FileNotFoundError, match="clipiqa_text"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "clipiqa", "--metric_weights", str(tmp_path)])
