"""The no-reference metric CLIP-IQA (pyiqa's ``clipiqa``: CLIP RN50, fixed prompts) on the GPU, visual tower in exact fp32 (csrc/clipiqa.hip).

The definition, restated from pyiqa's ``clipiqa`` and OpenAI CLIP's ``ModifiedResNet``:

  images in [0,1] of any size (one channel is repeated; no resize, no crop) -> (v - mean) / std with CLIP's constants;
  stem: conv 3->32 3x3 stride 2, conv 32->32 3x3, conv 32->64 3x3 (each BatchNorm, ReLU), AvgPool2d(2);
  four stages of (3, 4, 6, 3) bottlenecks, planes (64, 128, 256, 512), expansion 4: conv1 1x1, conv2 3x3 (stride 1), AvgPool2d(stride),
    conv3 1x1, each with BatchNorm (eval mode, eps 1e-5), ReLU after conv1, conv2 and the sum with the identity; the first block of a stage
    has the identity AvgPool2d(stride) -> conv 1x1 -> BatchNorm; AvgPool2d floors odd sizes;
  attention pool: 2048 wide, 32 heads, output 1024, WITHOUT the positional embedding (which is what makes the metric size-free): tokens
    [mean over the positions; the positions], the mean token is the only query;
  score: the L2-normalised embedding against the L2-normalised text features of P (positive, negative) prompt pairs, logits scaled by
    exp(logit_scale); the value is the mean over the pairs of softmax(pair)[0], in [0,1], higher is better.

The user supplies the checkpoint (OpenAI's ``RN50.pt``) and either the text features (``clipiqa_text*.npz``) or CLIP's BPE vocabulary file,
from which ``python -m dove_amd.clipiqa text`` computes them once: the text tower depends on no image and runs in plain torch on the host, in
fp64.  This module walks the visual tower in Python; every operator is a kernel of the library.  BatchNorm is folded into the conv weights
in fp64 and rounded once to fp32.  Frames go through the tower in groups sized so that the live activations stay under
``ACTIVATION_BUDGET``; a frame's value does not depend on the grouping.
"""
from __future__ import annotations

import argparse
import functools
import gzip
import math
import os
import re
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

from . import iqa, ops
from .iqa import ACTIVATION_BUDGET, FLOAT32_DTYPES, GpuMetric, find_file, find_first, for_groups, score_folder
from .netweights import Weights, bn_affine, checked, fan_in_normal, he_normal, pack_conv_weight, random_tensors, strip

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
LAYERS, PLANES, EXPANSION = (3, 4, 6, 3), (64, 128, 256, 512), 4
STEM = (("conv1", "bn1", 32, 3, 2), ("conv2", "bn2", 32, 32, 1), ("conv3", "bn3", 64, 32, 1))      # conv, bn, cout, cin, stride
EMBED_DIM, HEADS, OUTPUT_DIM = 2048, 32, 1024
BN_EPS = 1e-5
# pyiqa's five prompt pairs (positive, negative), restated from memory; ``text_features(prompts=...)`` overrides them
PROMPTS = (("Good image", "bad image"), ("Sharp image", "blurry image"), ("sharp edges", "blurry edges"),
           ("High resolution image", "low resolution image"), ("Noise-free image", "noisy image"))
CONTEXT, SOT, EOT, MERGES = 77, 49406, 49407, 48894
TEXT_WIDTH, TEXT_HEADS, TEXT_LAYERS, VOCAB = 512, 8, 12, 49408
# Live fp32 activations of one tower group, per input pixel.  The peak is the first block of stage 2, whose conv1 and conv2 still run at
# stage 1's resolution (the pool sits behind conv2): its 256-channel input, kept for the identity branch, next to the 128-channel outputs
# of conv1 and conv2 at 1/4 side, (256 + 128 + 128) / 16 = 32 floats per input pixel.  The stem's conv3 (32 in, 64 out at 1/2 side) and
# stage 1's first block (64 + 64 next to the 256-channel identity, which conv3 overwrites in place) need 24.  Measured with
# tools/clipiqa_bench.py (docs/kernels.md).  One 2880 x 5120 frame is 1.9 GB, so 4 GiB holds two of them and 36 frames of 720 x 1280.
FILE_PATTERNS = {"model": ("RN50*.pt", "RN50*.pth"), "text": ("clipiqa_text*.npz",), "vocab": ("bpe_simple_vocab_16e6.txt*",)}
TEXT_DRAW = 50                                      # random_clipiqa_state's text features: see there
COUNTERS = {"groups": 0}                            # tower groups walked, for tests and tools


def _out_side(s: int) -> int:
    s = (s - 1) // 2 + 1                            # the stem's stride-2 conv (3 x 3, pad 1)
    for _ in range(4):                              # the stem's AvgPool2d(2) and the stride of stages 2 to 4
        s //= 2
    return s


MIN_SIDE = next(s for s in range(1, 1024) if _out_side(s) >= 1)      # 31: the feature map is 1 x 1 at this size


def _blocks():
    """(prefix, inplanes, planes, stride, has_downsample) of the 16 bottlenecks in order."""
    inplanes = 64
    for li, (n, planes) in enumerate(zip(LAYERS, PLANES)):
        for i in range(n):
            stride = 2 if (li > 0 and i == 0) else 1
            yield f"visual.layer{li + 1}.{i}", inplanes, planes, stride, i == 0
            inplanes = planes * EXPANSION


def _bn_shapes(name: str, c: int) -> dict:
    return {f"{name}.{k}": (c,) for k in ("weight", "bias", "running_mean", "running_var")}


def visual_param_shapes() -> dict:
    """name -> shape of the entries of CLIP RN50's state dict that the metric reads (the visual tower without its positional embedding,
    and ``logit_scale``)."""
    s = {}
    for conv, bn, cout, cin, _ in STEM:
        s[f"visual.{conv}.weight"] = (cout, cin, 3, 3)
        s.update(_bn_shapes(f"visual.{bn}", cout))
    for p, inplanes, planes, _, down in _blocks():
        for conv, bn, cout, cin, k in (("conv1", "bn1", planes, inplanes, 1), ("conv2", "bn2", planes, planes, 3),
                                       ("conv3", "bn3", planes * EXPANSION, planes, 1)):
            s[f"{p}.{conv}.weight"] = (cout, cin, k, k)
            s.update(_bn_shapes(f"{p}.{bn}", cout))
        if down:
            s[f"{p}.downsample.0.weight"] = (planes * EXPANSION, inplanes, 1, 1)
            s.update(_bn_shapes(f"{p}.downsample.1", planes * EXPANSION))
    for n, o in (("q", EMBED_DIM), ("k", EMBED_DIM), ("v", EMBED_DIM), ("c", OUTPUT_DIM)):
        s[f"visual.attnpool.{n}_proj.weight"] = (o, EMBED_DIM)
        s[f"visual.attnpool.{n}_proj.bias"] = (o,)
    s["logit_scale"] = ()
    return s


def text_param_shapes() -> dict:
    """name -> shape of the text tower's entries of CLIP RN50's state dict."""
    w = TEXT_WIDTH
    s = {"token_embedding.weight": (VOCAB, w), "positional_embedding": (CONTEXT, w), "ln_final.weight": (w,), "ln_final.bias": (w,),
         "text_projection": (w, OUTPUT_DIM)}
    for i in range(TEXT_LAYERS):
        p = f"transformer.resblocks.{i}"
        s.update({f"{p}.ln_1.weight": (w,), f"{p}.ln_1.bias": (w,), f"{p}.ln_2.weight": (w,), f"{p}.ln_2.bias": (w,),
                  f"{p}.attn.in_proj_weight": (3 * w, w), f"{p}.attn.in_proj_bias": (3 * w,), f"{p}.attn.out_proj.weight": (w, w),
                  f"{p}.attn.out_proj.bias": (w,), f"{p}.mlp.c_fc.weight": (4 * w, w), f"{p}.mlp.c_fc.bias": (4 * w,),
                  f"{p}.mlp.c_proj.weight": (w, 4 * w), f"{p}.mlp.c_proj.bias": (w,)})
    return s


def random_clipiqa_state(seed: int):
    """Rule-generated (state dict, text) for tests and tools.  Conv weights are normal with He std; BatchNorm weights are uniform in
    [0.5, 1.5] ([0.1, 0.3] for a block's bn3, so that the residual sums stay tame), biases and running means 0.05 * normal, running
    variances uniform in [0.5, 1.5]; the projections normal with std 1 / sqrt(2048), their biases 0.05 * normal; logit_scale = ln 100.
    text = {features [10,1024] fp64, prompts, logit_scale}: a positive row is normal, its negative is the positive plus a normal
    perturbation of 0.4 of its length, so that a pair's logits differ by a unit or two and no pair softmax saturates.  TEXT_DRAW, the
    third key of that generator, was chosen among 60 so that the scores of the tests' images (seed 31) also differ between noise levels
    by several 1e-3 under the fp64 restatement; tests/test_clipiqa_cpu.py asserts both."""
    def rule(name, shape, rng):
        if name == "logit_scale":
            return math.log(100.0)
        if len(shape) == 4:
            return he_normal(rng, shape)
        if len(shape) == 2:
            return fan_in_normal(rng, shape)
        if name.endswith("running_var"):
            return rng.uniform(0.5, 1.5, shape)
        if name.endswith(".weight"):
            return rng.uniform(0.1, 0.3, shape) if ".bn3." in name else rng.uniform(0.5, 1.5, shape)
        return 0.05 * rng.standard_normal(shape)

    sd = random_tensors(visual_param_shapes(), seed, lambda name: f"clipiqa.{name}", rule)
    rng = np.random.default_rng([int(seed), zlib.crc32(b"clipiqa.text"), TEXT_DRAW])
    pos = rng.standard_normal((len(PROMPTS), OUTPUT_DIM))
    neg = pos + 0.4 * rng.standard_normal(pos.shape)
    feats = np.stack([pos, neg], axis=1).reshape(2 * len(PROMPTS), OUTPUT_DIM)
    return sd, {"features": feats, "prompts": [p for pair in PROMPTS for p in pair], "logit_scale": math.log(100.0)}


def fold_bn(w: torch.Tensor, gamma, beta, mean, var, eps: float = BN_EPS):
    """conv weight [Cout,Cin,kh,kw] and eval-mode BatchNorm -> (weight, bias) in fp64: s = gamma / sqrt(var + eps), w s, beta - mean s."""
    s, shift = bn_affine(gamma, beta, mean, var, eps)
    return w.double() * s[:, None, None, None], shift


def _folded(sd: dict, conv: str, bn: str):
    w, b = fold_bn(sd[f"{conv}.weight"], *(sd[f"{bn}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")))
    return pack_conv_weight(w), b.float().contiguous()                  # one rounding to fp32


def _normalised(features) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(features), dtype=torch.float64)
    if t.dim() != 2 or t.shape[1] != OUTPUT_DIM or t.shape[0] < 2 or t.shape[0] % 2:
        raise ValueError(f"CLIP-IQA text features: shape {tuple(t.shape)}, expected [2 P, {OUTPUT_DIM}] (positive, negative rows per pair)")
    return (t / t.norm(dim=1, keepdim=True)).contiguous()


# OpenAI's file is a TorchScript archive: a plain state dict is tried first, the archive's state dict second
_load_sd = functools.partial(iqa.load_state_dict, torchscript=True)


@dataclass
class ClipIqaWeights(Weights):
    convs: dict = field(default_factory=dict)       # conv name -> (w [kh,kw,cin,cout] with its BatchNorm folded in, bias)
    attn: list = field(default_factory=list)        # wq, bq, wk, bk, wv, bv, wc, bc (float32, [out,in] weights)
    text: list = field(default_factory=list)        # [features float64 [2P,1024], L2-normalised]
    logit_scale: float = 100.0                      # exp of CLIP's parameter
    prompts: tuple = ()

    @classmethod
    def from_state_dict(cls, sd: dict, text=None) -> "ClipIqaWeights":
        """``sd``: CLIP RN50's state dict; ``text``: {features [2P,1024], prompts, logit_scale} as ``clipiqa_text.npz`` holds them."""
        if text is None:
            raise ValueError("CLIP-IQA needs the text features of its prompts: pass the contents of clipiqa_text.npz, or make them with "
                             "`python -m dove_amd.clipiqa text --model RN50.pt --vocab bpe_simple_vocab_16e6.txt.gz --out DIR/clipiqa_text.npz`")
        sd = checked(strip(sd), visual_param_shapes(), "CLIP RN50 checkpoint")
        convs = {f"visual.{conv}": _folded(sd, f"visual.{conv}", f"visual.{bn}") for conv, bn, _, _, _ in STEM}
        for p, _, _, _, down in _blocks():
            for i in (1, 2, 3):
                convs[f"{p}.conv{i}"] = _folded(sd, f"{p}.conv{i}", f"{p}.bn{i}")
            if down:
                convs[f"{p}.downsample"] = _folded(sd, f"{p}.downsample.0", f"{p}.downsample.1")
        attn = [sd[f"visual.attnpool.{n}_proj.{k}"].float().contiguous() for n in "qkvc" for k in ("weight", "bias")]
        prompts = tuple(str(p) for p in text["prompts"]) if "prompts" in text else ()
        return cls(convs=convs, attn=attn, text=[_normalised(text["features"])], logit_scale=float(torch.exp(sd["logit_scale"].double())),
                   prompts=prompts)

    @classmethod
    def load(cls, directory: str) -> "ClipIqaWeights":
        """From a ``--metric_weights`` directory: ``RN50*.pt`` / ``RN50*.pth``, and ``clipiqa_text*.npz`` or CLIP's vocabulary file."""
        sd = strip(_load_sd(find_file(directory, FILE_PATTERNS["model"])))
        npz, vocab = find_first(directory, FILE_PATTERNS["text"]), find_first(directory, FILE_PATTERNS["vocab"])
        if npz is not None:
            with np.load(npz, allow_pickle=False) as z:
                text = {k: z[k] for k in z.files}
        elif vocab is not None:
            text = {"features": text_features(sd, vocab).numpy(), "prompts": [p for pair in PROMPTS for p in pair]}
        else:
            raise FileNotFoundError(f"CLIP-IQA needs the text features of its prompts and {directory} has neither {FILE_PATTERNS['text'][0]} nor "
                                    f"{FILE_PATTERNS['vocab'][0]}: put CLIP's vocabulary file (it ships with the `clip` package) there, or run "
                                    "`python -m dove_amd.clipiqa text --model RN50.pt --vocab bpe_simple_vocab_16e6.txt.gz --out "
                                    f"{os.path.join(directory, 'clipiqa_text.npz')}` once")
        return cls.from_state_dict(sd, text)


# ------------------------------------------------------------------- walk -------------------------------------------------------------------
def group_size(h: int, w: int, budget: int | None = None) -> int:
    """Frames per tower group: the most whose live activations stay under the budget (32 floats per input pixel), at least one."""
    return max(1, int((ACTIVATION_BUDGET if budget is None else budget) // (4 * 32 * h * w)))


def _conv(W, name: str, x, **kw):
    w, b = W.convs[name]
    return ops.resnet_conv_f32(x, w, b, **kw)


def stem(W: ClipIqaWeights, hold: list) -> torch.Tensor:
    """Prepared images float32 [g,H,W,3] -> the stem's output [g,H/4,W/4,64].  ``hold`` is a one-element list that is emptied: the
    caller keeps no reference, so every map is freed as soon as the next one exists (``stage`` takes its input the same way)."""
    x = hold.pop()
    for conv, _, _, _, stride in STEM:
        x = _conv(W, f"visual.{conv}", x, stride=stride)
    return ops.avgpool_cl_f32(x)


def stage(W: ClipIqaWeights, hold: list, li: int) -> torch.Tensor:
    """The bottlenecks of stage ``li`` (0 to 3).  The AvgPool2d of a strided block is read on load by the two 1 x 1 convs behind it."""
    x = hold.pop()
    for p, _, _, stride, down in _blocks():
        if not p.startswith(f"visual.layer{li + 1}."):
            continue
        t = _conv(W, f"{p}.conv1", x)
        t = _conv(W, f"{p}.conv2", t)
        ident = _conv(W, f"{p}.downsample", x, pool=stride, relu=False) if down else x
        del x                                        # the sum overwrites the identity: no third 4 x planes map is live
        x = _conv(W, f"{p}.conv3", t, pool=stride, residual=ident, out=ident)
        del t, ident
    return x


def features(W: ClipIqaWeights, hold: list) -> torch.Tensor:
    """The visual tower: prepared images float32 [g,H,W,3], handed over in a one-element list -> the feature map [g,h,w,2048]."""
    hold = [stem(W, hold)]
    for li in range(len(LAYERS)):
        hold = [stage(W, hold, li)]
    return hold.pop()


def embed(W: ClipIqaWeights, images: torch.Tensor) -> torch.Tensor:
    """Image embeddings float32 [g,1024] of a group of images on W's device ([g,1|3,H,W] uint8 or float32 views)."""
    return ops.clip_attnpool_f32(features(W, [ops.percep_prep_f32(images, 1.0, 0.0, CLIP_MEAN, CLIP_STD)]), W.attn)


def _images(x: torch.Tensor, device=None) -> torch.Tensor:
    return iqa.images(x, "clipiqa", (MIN_SIDE, MIN_SIDE), FLOAT32_DTYPES, device)


def clipiqa(W: ClipIqaWeights, pred: torch.Tensor, group: int | None = None, want_embedding: bool = False):
    """CLIP-IQA per image -> float64 [N] on the device, in [0,1], higher is better.  ``pred``: [N,C,H,W] float in [0,1] or uint8 (any
    strides, C in {1, 3}; one channel is repeated), or [F,H,W,3] uint8 frames; a host tensor is uploaded.  ``group``: frames per tower
    batch (default: from the budget).  ``want_embedding``: also return the float32 [N,1024] image embeddings."""
    if not isinstance(W, ClipIqaWeights):
        raise TypeError(f"clipiqa: weights must be ClipIqaWeights, got {type(W).__name__}")
    x = _images(pred)
    W = W.to(x.device)
    emb = torch.empty(x.shape[0], OUTPUT_DIM, dtype=torch.float32, device=x.device)

    def per_group(i, j):
        emb[i:j] = embed(W, x[i:j])

    for_groups(x.shape[0], group, group_size(x.shape[2], x.shape[3]), COUNTERS, x.device, per_group)
    with torch.cuda.device(x.device):
        out = ops.clipiqa_score(emb, W.text[0], W.logit_scale)
    return (out, emb) if want_embedding else out


class ClipIqaMetric(GpuMetric):
    """pyiqa-style metric object: ``metric(pred)`` with [N,C,H,W] images in [0,1] (host or device) -> [N] fp64 CLIP-IQA scores."""

    def __init__(self, weights: ClipIqaWeights):
        super().__init__("clipiqa", False, False, clipiqa, weights, ClipIqaWeights)


# --------------------------------------------------------------- the text side ---------------------------------------------------------------
def _bytes_to_unicode() -> dict:
    """CLIP's byte -> printable character table: the printable latin-1 bytes map to themselves, the other 68 to U+0100 onwards."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xa1, 0xac + 1)) + list(range(0xae, 0xff + 1))
    table, n = {b: chr(b) for b in keep}, 0
    for b in range(256):
        if b not in table:
            table[b] = chr(256 + n)
            n += 1
    return table


_WORDS = re.compile(r"'s|'t|'re|'ve|'m|'ll|'d|[^\W\d_]+|\d|(?:[^\s\w]|_)+")


class Tokenizer:
    """CLIP's byte-level BPE, written from its description.  ``merges``: the pairs in rank order (lines 1 to 48894 of
    ``bpe_simple_vocab_16e6.txt.gz``).  Ids: the 256 byte characters, the same with ``</w>``, the merges in order, then SOT and EOT."""

    def __init__(self, merges):
        self.byte = _bytes_to_unicode()
        chars = list(self.byte.values())                         # the printable bytes first, then the remapped ones: the table's own order
        vocab = chars + [c + "</w>" for c in chars] + ["".join(m) for m in merges]
        self.ids = {t: i for i, t in enumerate(vocab)}
        self.sot, self.eot = len(vocab), len(vocab) + 1
        self.rank = {tuple(m): i for i, m in enumerate(merges)}

    @classmethod
    def from_file(cls, path: str, count: int = MERGES) -> "Tokenizer":
        opener = gzip.open if path.endswith(".gz") else open
        with opener(path, "rt", encoding="utf-8") as f:
            lines = f.read().split("\n")
        return cls([tuple(l.split()) for l in lines[1:1 + count]])      # line 0 is the file's header

    def bpe(self, word: str):
        parts = list(word[:-1]) + [word[-1] + "</w>"]
        while len(parts) > 1:
            best = min(zip(parts, parts[1:]), key=lambda p: self.rank.get(p, math.inf))
            if best not in self.rank:
                break
            out, i = [], 0
            while i < len(parts):
                if i + 1 < len(parts) and (parts[i], parts[i + 1]) == best:
                    out.append(parts[i] + parts[i + 1])
                    i += 2
                else:
                    out.append(parts[i])
                    i += 1
            parts = out
        return parts

    def encode(self, text: str):
        text = " ".join(text.split()).lower()
        ids = []
        for word in _WORDS.findall(text):
            ids += [self.ids[t] for t in self.bpe("".join(self.byte[b] for b in word.encode("utf-8")))]
        return ids

    def __call__(self, texts, context: int = CONTEXT) -> torch.Tensor:
        """-> int64 [len(texts), context]: SOT, the tokens, EOT, zero padding.  A text that does not fit is refused."""
        out = torch.zeros(len(texts), context, dtype=torch.int64)
        for i, t in enumerate(texts):
            ids = [self.sot] + self.encode(t) + [self.eot]
            if len(ids) > context:
                raise ValueError(f"prompt {t!r} has {len(ids)} tokens with SOT and EOT; the context holds {context}")
            out[i, :len(ids)] = torch.tensor(ids)
        return out


def encode_text(sd: dict, tokens: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """CLIP's text tower in plain torch on the host: tokens int64 [B,L] -> features [B,1024] (not normalised)."""
    F = torch.nn.functional
    g = lambda k: sd[k].to(dtype)
    B, Lc = tokens.shape
    x = g("token_embedding.weight")[tokens] + g("positional_embedding")[:Lc]
    mask = torch.full((Lc, Lc), float("-inf"), dtype=dtype).triu(1)
    hd = TEXT_WIDTH // TEXT_HEADS
    for i in range(TEXT_LAYERS):
        p = f"transformer.resblocks.{i}"
        h = F.layer_norm(x, (TEXT_WIDTH,), g(f"{p}.ln_1.weight"), g(f"{p}.ln_1.bias"))
        q, k, v = (F.linear(h, g(f"{p}.attn.in_proj_weight"), g(f"{p}.attn.in_proj_bias"))
                   .view(B, Lc, 3, TEXT_HEADS, hd).permute(2, 0, 3, 1, 4))
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd) + mask, dim=-1) @ v
        x = x + F.linear(a.transpose(1, 2).reshape(B, Lc, TEXT_WIDTH), g(f"{p}.attn.out_proj.weight"), g(f"{p}.attn.out_proj.bias"))
        h = F.layer_norm(x, (TEXT_WIDTH,), g(f"{p}.ln_2.weight"), g(f"{p}.ln_2.bias"))
        h = F.linear(h, g(f"{p}.mlp.c_fc.weight"), g(f"{p}.mlp.c_fc.bias"))
        x = x + F.linear(h * torch.sigmoid(1.702 * h), g(f"{p}.mlp.c_proj.weight"), g(f"{p}.mlp.c_proj.bias"))
    x = F.layer_norm(x, (TEXT_WIDTH,), g("ln_final.weight"), g("ln_final.bias"))
    return x[torch.arange(B), tokens.argmax(dim=-1)] @ g("text_projection")


def text_features(sd: dict, vocab_path: str, prompts=None) -> torch.Tensor:
    """The fp64 text features [2P,1024] (not normalised) of the prompt pairs under the checkpoint's text tower."""
    sd = checked(strip(sd), text_param_shapes(), "CLIP RN50 checkpoint (text tower)")
    flat = [p for pair in (PROMPTS if prompts is None else prompts) for p in pair]
    return encode_text(sd, Tokenizer.from_file(vocab_path)(flat))


def save_text(path: str, features, prompts, logit_scale: float) -> None:
    np.savez(path, features=np.asarray(features, dtype=np.float64), prompts=np.asarray(list(prompts)), logit_scale=np.float64(logit_scale))


def main(argv=None):
    ap = argparse.ArgumentParser(description="CLIP-IQA on the GPU (dove_amd): make the text features of the prompts, or score images")
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("text", help="run CLIP's text tower over the prompt pairs once and save the features")
    t.add_argument("--model", required=True, help="CLIP RN50 checkpoint (OpenAI's RN50.pt, or a saved state dict)")
    t.add_argument("--vocab", required=True, help="CLIP's bpe_simple_vocab_16e6.txt.gz")
    t.add_argument("--prompts", default="", help="'positive|negative;positive|negative;...' (default: pyiqa's five pairs)")
    t.add_argument("--out", required=True, help="clipiqa_text.npz to write")
    s = sub.add_parser("score", help="score every image of a folder")
    s.add_argument("--pred", required=True, help="folder of images")
    s.add_argument("--metric_weights", required=True, help="directory with RN50*.pt and clipiqa_text*.npz (or the vocabulary file)")
    args = ap.parse_args(argv)
    if args.cmd == "text":
        pairs = [tuple(p.split("|")) for p in args.prompts.split(";") if p.strip()] or list(PROMPTS)
        if any(len(p) != 2 for p in pairs):
            raise ValueError(f"--prompts {args.prompts!r}: every pair is 'positive|negative'")
        sd = strip(_load_sd(args.model))
        feats = text_features(sd, args.vocab, pairs)
        save_text(args.out, feats.numpy(), [p for pair in pairs for p in pair], float(sd["logit_scale"]))
        print(f"text features of {len(pairs)} prompt pairs -> {args.out}")
        return feats
    return score_folder(args, lambda a: ClipIqaWeights.load(a.metric_weights), clipiqa)


if __name__ == "__main__":
    main()
