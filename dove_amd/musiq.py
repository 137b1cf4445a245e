"""The no-reference metric MUSIQ (pyiqa's ``musiq``: multi-scale patches, a ResNet stem per patch, a 14-layer transformer) on the GPU in
exact fp32 (csrc/musiq.hip and the fp32 convs / GEMMs of csrc/conv_f32.hip).

The definition, restated from memory of pyiqa's ``musiq_arch.py`` and ``multiscale_trans_util.py`` (INTEGRATION.md 1k lists what is
unchecked; every such choice is a module-level constant or one small function here):

  images in [0,1] of any size from 1 x 1 (one channel is repeated) -> v' = 2 v - 1;
  three scales in this token order: longer side 224, longer side 384 (``SCALE_SIDES``; rh = round(H L / max(H, W)), bicubic without
    antialias, evaluated in fp64 and rounded once), then the original resolution;
  each scale is zero-padded to multiples of 32 (pad // 2 on top and left) and cut into 32 x 32 patches, row-major; patch (i, j) has the
    spatial index hh[i] * 10 + hw[j] with hh, hw the nearest-neighbour resize of arange(10) to the patch counts;
  per patch: conv_root 7 x 7 stride 2 'same' (2 before, 3 after), GroupNorm(32, eps ``GN_ROOT_EPS``), ReLU, zero 'same' MaxPool 3 x 3
    stride 2, one bottleneck 64 -> 256 with a projected identity (GroupNorm eps ``GN_BLOCK_EPS``); every conv is weight-standardised
    ((w - mean) / (std + 1e-5) per output channel, ``STD_UNBIASED``); the 8 x 8 x 256 map, flattened (h, w, c), goes through Linear
    16384 -> 384;
  x = emb + position_emb[spatial index] + scale_emb[scale], a cls token in front, 14 pre-LN blocks (LayerNorm eps 1e-6, 6 heads of 64,
    MLP 384 -> 1152 -> 384 with the exact-erf GELU), encoder_norm, head Linear(384 -> K) on token 0; K = 1: the score; K = 10 (AVA): the
    mean rating sum (k + 1) softmax_k.  Higher is better.

pyiqa pads the two resized scales to 49 / 144 tokens with masked zero patches.  A masked key never contributes (its softmax weight
underflows to 0) and only token 0 reaches the head, so no padding token is created here: a frame's sequence is 1 + the patches of the three
scales (1033 at 720 x 1280).  tests/musiq_ref.py keeps the padded, masked form and tests/test_musiq_cpu.py shows that the two agree.

The user supplies the checkpoint (``musiq*.pth``).  This module walks the network in Python; every operator is a kernel of the library.
Frames go through in groups sized so that the live activations stay under ``ACTIVATION_BUDGET``; a frame's value does not depend on the
grouping.
"""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import iqa, ops
from .iqa import ACTIVATION_BUDGET, GpuMetric, find_file, for_groups, load_state_dict, score_folder
from .netweights import (Weights, checked, device_tables, fan_in_normal, nearest_index, pack_conv_weight, pack_linear_weight, prenorm_mlp_f32,
                         random_tensors, strip)

PATCH, HASH_GRID = 32, 10
SCALE_SIDES = (224, 384)                            # the longer sides of the two resized scales; the third scale is the original
STEM_BEFORE, STEM_SIDE = 2, 37                      # conv_root's 'same' frame of a 32 x 32 patch: 2 zeros before, 3 after
GN_GROUPS, GN_ROOT_EPS, GN_BLOCK_EPS = 32, 1e-6, 1e-4      # (eps values from memory)
STD_EPS, STD_UNBIASED = 1e-5, True                  # StdConv: (w - mean) / (std + eps), torch's default (unbiased) std (from memory)
DIM, HEADS, MLP_DIM, NUM_LAYERS, LN_EPS = 384, 6, 1152, 14, 1e-6
STEM_CH, BLOCK_CH, MAP_SIDE = 64, 256, 8
EMBED_IN = MAP_SIDE * MAP_SIDE * BLOCK_CH           # 16384
FILE_PATTERN = "musiq*.pth"
# Live fp32 activations of one group, per patch token.  The peak is the end of the bottleneck: the pooled stem map (8 x 8 x 64), the
# projected identity and conv3's output (8 x 8 x 256 each; the sum overwrites conv3's output, which is then the embedding's 64 KiB input)
# and conv2's output (8 x 8 x 64): 4096 + 16384 + 16384 + 4096 = 40960 floats = 160 KiB.  The stem conv (its 37 x 37 x 3 frame next to the
# 16 x 16 x 64 output) needs 80 KiB, the transformer 3 K floats.  Measured with tools/musiq_bench.py (docs/kernels.md).
TOKEN_FLOATS = 40960
WEIGHT_DRAW = 0                                     # random_musiq_state's generator draw: see there
COUNTERS = {"groups": 0}                            # groups walked, for tests and tools


# ------------------------------------------------------------------ geometry ------------------------------------------------------------------
def scale_sizes(H: int, W: int):
    """[(rh, rw, resized)] of the three scales.  A resized side never drops below one pixel."""
    out = []
    for L_ in SCALE_SIDES:
        ratio = L_ / max(H, W)
        out.append((max(1, round(H * ratio)), max(1, round(W * ratio)), True))
    return out + [(H, W, False)]


def hash_index(count: int, grid: int = HASH_GRID) -> np.ndarray:
    """``nearest_index`` on the position grid (pyiqa's get_hashed_spatial_pos_emb_index)."""
    return nearest_index(count, grid)


_GEOMETRY = {}


def token_geometry(H: int, W: int) -> dict:
    """Host-side token layout of an H x W frame: ``scales`` three (rh, rw, pad_top, pad_left, resized), ``counts`` three (ch, cw),
    ``tokens`` int32 [T,4] rows (scale, patch row, patch column, spatial index) in sequence order, ``length`` = T + 1 with the cls token."""
    key = (int(H), int(W))
    if key not in _GEOMETRY:
        scales, counts, rows = [], [], []
        for s, (rh, rw, resized) in enumerate(scale_sizes(*key)):
            ch, cw = -(-rh // PATCH), -(-rw // PATCH)
            scales.append((rh, rw, (ch * PATCH - rh) // 2, (cw * PATCH - rw) // 2, resized))
            counts.append((ch, cw))
            hh, hw = hash_index(ch), hash_index(cw)
            rows += [(s, i, j, int(hh[i]) * HASH_GRID + int(hw[j])) for i in range(ch) for j in range(cw)]
        tokens = torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)
        _GEOMETRY[key] = {"scales": scales, "counts": counts, "tokens": tokens, "length": len(rows) + 1, "device": {}}
    return _GEOMETRY[key]


def group_size(h: int, w: int, budget: int | None = None) -> int:
    """Frames per group: the most whose live activations (``TOKEN_FLOATS`` per patch token) stay under the budget, at least one."""
    tokens = token_geometry(h, w)["length"] - 1
    return max(1, int((ACTIVATION_BUDGET if budget is None else budget) // (4 * TOKEN_FLOATS * tokens)))


# ------------------------------------------------------------------- weights -------------------------------------------------------------------
STEM_CONVS = (("conv_root", STEM_CH, 3, 7), ("block1.conv1", STEM_CH, STEM_CH, 1), ("block1.conv2", STEM_CH, STEM_CH, 3),
              ("block1.conv3", BLOCK_CH, STEM_CH, 1), ("block1.conv_proj", BLOCK_CH, STEM_CH, 1))        # name, cout, cin, k
STEM_NORMS = (("gn_root", STEM_CH), ("block1.gn1", STEM_CH), ("block1.gn2", STEM_CH), ("block1.gn3", BLOCK_CH), ("block1.gn_proj", BLOCK_CH))
ENC = "transformer_encoder"


def _layer(i: int) -> str:
    return f"{ENC}.transformer.encoderblock_{i:02d}"


def param_shapes(num_classes: int = 1, layers: int | None = None) -> dict:
    """name -> shape of the entries of pyiqa's MUSIQ state dict (names from memory: INTEGRATION.md 1k)."""
    s = {}
    for name, cout, cin, k in STEM_CONVS:
        s[f"{name}.weight"] = (cout, cin, k, k)
    for name, c in STEM_NORMS:
        s[f"{name}.weight"], s[f"{name}.bias"] = (c,), (c,)
    s["embedding.weight"], s["embedding.bias"] = (DIM, EMBED_IN), (DIM,)
    s[f"{ENC}.posembed_input.position_emb"] = (1, HASH_GRID * HASH_GRID, DIM)
    s[f"{ENC}.scaleembed_input.scale_emb"] = (1, 3, DIM)
    s[f"{ENC}.cls"] = (1, 1, DIM)
    for i in range(NUM_LAYERS if layers is None else layers):
        p = _layer(i)
        for n in ("norm1", "norm2"):
            s[f"{p}.{n}.weight"], s[f"{p}.{n}.bias"] = (DIM,), (DIM,)
        for n in ("query", "key", "value", "out"):
            s[f"{p}.attention.{n}.weight"], s[f"{p}.attention.{n}.bias"] = (DIM, DIM), (DIM,)
        s[f"{p}.mlp.fc1.weight"], s[f"{p}.mlp.fc1.bias"] = (MLP_DIM, DIM), (MLP_DIM,)
        s[f"{p}.mlp.fc2.weight"], s[f"{p}.mlp.fc2.bias"] = (DIM, MLP_DIM), (DIM,)
    s[f"{ENC}.encoder_norm.weight"], s[f"{ENC}.encoder_norm.bias"] = (DIM,), (DIM,)
    s["head.weight"], s["head.bias"] = (num_classes, DIM), (num_classes,)
    return s


def random_musiq_state(seed: int, num_classes: int = 1) -> dict:
    """Rule-generated state dict for tests and tools.  Conv and Linear weights are normal with std 1 / sqrt(fan-in) (the convs are
    standardised anyway), norm weights uniform in [0.5, 1.5], biases 0.05 * normal, the position and scale embeddings and cls normal with
    std 0.5, so that tokens differ by where they sit as much as by what they show.  Each tensor has its own generator keyed by (seed, name,
    WEIGHT_DRAW); tests/test_musiq_cpu.py asserts, under the fp64 restatement, that with this draw the scores of the tests' images
    separate their noise levels and that the attention's softmax is neither uniform nor one-hot."""
    def rule(name, shape, rng):
        if name.endswith(("position_emb", "scale_emb", "cls")):
            return 0.5 * rng.standard_normal(shape)
        if len(shape) >= 2:
            return fan_in_normal(rng, shape)
        return rng.uniform(0.5, 1.5, shape) if name.endswith(".weight") else 0.05 * rng.standard_normal(shape)

    return random_tensors(param_shapes(num_classes), seed, lambda name: f"musiq.{name}", rule, (WEIGHT_DRAW,))


def standardise(w: torch.Tensor) -> torch.Tensor:
    """StdConv's weight in fp64: (w - mean) / (std + STD_EPS) per output channel over (cin, kh, kw)."""
    w = w.double()
    m = w.mean(dim=(1, 2, 3), keepdim=True)
    s = w.std(dim=(1, 2, 3), keepdim=True, unbiased=STD_UNBIASED)
    return (w - m) / (s + STD_EPS)


@dataclass
class MusiqWeights(Weights):
    """``convs``: the standardised stem convs (weight [k,k,cin,cout], no bias); ``params``: every other tensor by a short name."""
    convs: dict = field(default_factory=dict)
    params: dict = field(default_factory=dict)
    num_classes: int = 1

    @classmethod
    def from_state_dict(cls, sd: dict) -> "MusiqWeights":
        sd = strip(sd["params"] if isinstance(sd.get("params"), dict) else sd)
        k = int(sd["head.weight"].shape[0]) if "head.weight" in sd and sd["head.weight"].dim() == 2 else 1
        sd = checked(sd, param_shapes(k), "MUSIQ checkpoint")
        f32 = lambda t: t.detach().float().contiguous()
        lin = pack_linear_weight                    # [out,in] -> the 1 x 1 walk's [1,1,in,out]
        convs = {name: (pack_conv_weight(standardise(sd[f"{name}.weight"])), torch.zeros(0)) for name, _, _, _ in STEM_CONVS}   # one rounding
        p = {}
        for name, _ in STEM_NORMS:
            p[f"{name}.weight"], p[f"{name}.bias"] = f32(sd[f"{name}.weight"]), f32(sd[f"{name}.bias"])
        p["embedding.weight"], p["embedding.bias"] = lin(sd["embedding.weight"]), f32(sd["embedding.bias"])
        p["pos"] = f32(sd[f"{ENC}.posembed_input.position_emb"]).reshape(HASH_GRID * HASH_GRID, DIM)
        p["scale"] = f32(sd[f"{ENC}.scaleembed_input.scale_emb"]).reshape(3, DIM)
        p["cls"] = f32(sd[f"{ENC}.cls"]).reshape(DIM)
        for i in range(NUM_LAYERS):
            src = _layer(i)
            for n in ("norm1", "norm2"):
                p[f"{i}.{n}.weight"], p[f"{i}.{n}.bias"] = f32(sd[f"{src}.{n}.weight"]), f32(sd[f"{src}.{n}.bias"])
            # query, key and value as one GEMM: each output column is still its own K-ordered chain
            p[f"{i}.qkv.weight"] = lin(torch.cat([sd[f"{src}.attention.{n}.weight"] for n in ("query", "key", "value")]))
            p[f"{i}.qkv.bias"] = f32(torch.cat([sd[f"{src}.attention.{n}.bias"] for n in ("query", "key", "value")]))
            for dst, n in (("out", "attention.out"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
                p[f"{i}.{dst}.weight"], p[f"{i}.{dst}.bias"] = lin(sd[f"{src}.{n}.weight"]), f32(sd[f"{src}.{n}.bias"])
        p["encoder_norm.weight"], p["encoder_norm.bias"] = f32(sd[f"{ENC}.encoder_norm.weight"]), f32(sd[f"{ENC}.encoder_norm.bias"])
        p["head.weight"], p["head.bias"] = f32(sd["head.weight"]), f32(sd["head.bias"])
        return cls(convs=convs, params=p, num_classes=k)

    @classmethod
    def load(cls, directory: str) -> "MusiqWeights":
        """From a ``--metric_weights`` directory: the first ``musiq*.pth`` (pyiqa's checkpoint; a top-level ``params`` is unwrapped)."""
        return cls.from_state_dict(load_state_dict(find_file(directory, FILE_PATTERN)))


# -------------------------------------------------------------------- walk --------------------------------------------------------------------
def patches(images: torch.Tensor, before: int = 0, side: int = PATCH):
    """Every token's 2 v - 1 patch of a group of images on the device -> (float32 [g T,side,side,3], geometry)."""
    geo = token_geometry(images.shape[2], images.shape[3])
    return ops.musiq_patches_f32(images, geo["scales"], device_tables(geo, images.device, ("tokens",))[0], before, side), geo


def _gn(W: MusiqWeights, name: str, x, eps, **kw):
    return ops.musiq_groupnorm_f32(x, W.params[f"{name}.weight"], W.params[f"{name}.bias"], eps, **kw)


def stem(W: MusiqWeights, hold: list) -> torch.Tensor:
    """Patch frames float32 [P,37,37,3], handed over in a one-element list that is emptied -> the bottleneck's output [P,8,8,256]."""
    conv = lambda name, x: ops.resnet_conv_f32(x, W.convs[name][0], None, relu=False)
    x = ops.convnet_conv_f32(hold.pop(), W.convs["conv_root"][0], None, stride=2, pad=(0, 0), relu=False)
    x = _gn(W, "gn_root", x, GN_ROOT_EPS, relu=True, pool=True)
    t = conv("block1.conv1", x)
    ident = conv("block1.conv_proj", x)
    del x
    t = _gn(W, "block1.gn1", t, GN_BLOCK_EPS, relu=True, out=t)
    t = conv("block1.conv2", t)
    t = _gn(W, "block1.gn2", t, GN_BLOCK_EPS, relu=True, out=t)
    y = conv("block1.conv3", t)
    del t
    return _gn(W, "block1.gn3", y, GN_BLOCK_EPS, relu=True, y=ident, gamma_y=W.params["block1.gn_proj.weight"],
               beta_y=W.params["block1.gn_proj.bias"], out=y)


def encoder(W: MusiqWeights, x: torch.Tensor) -> torch.Tensor:
    """Token rows float32 [g,T,384] (changed in place) -> the same after the pre-LN blocks."""
    g, T, _ = x.shape
    p, rows = W.params, x.view(g * T, DIM)
    for i in range(NUM_LAYERS):                     # read at call time: tests shorten the stack
        h = ops.layernorm_f32(rows, p[f"{i}.norm1.weight"], p[f"{i}.norm1.bias"], LN_EPS)
        qkv = ops.linear_f32(h, p[f"{i}.qkv.weight"], p[f"{i}.qkv.bias"]).view(g, T, 3 * DIM)
        a = ops.mha_f32(qkv[..., :DIM], qkv[..., DIM:2 * DIM], qkv[..., 2 * DIM:], 1.0 / math.sqrt(DIM // HEADS))
        del qkv
        ops.linear_f32(a.view(g * T, DIM), p[f"{i}.out.weight"], p[f"{i}.out.bias"], residual=rows, out=rows)
        prenorm_mlp_f32(rows, h, p, f"{i}.norm2", f"{i}.fc1", f"{i}.fc2", LN_EPS)
        del h, a
    return x


def features(W: MusiqWeights, images: torch.Tensor) -> torch.Tensor:
    """The normalised token 0, float32 [g,384], of a group of images on W's device."""
    frames, geo = patches(images, STEM_BEFORE, STEM_SIDE)
    y = stem(W, [frames])
    del frames
    p = W.params
    emb = ops.linear_f32(y.view(y.shape[0], EMBED_IN), p["embedding.weight"], p["embedding.bias"])
    del y
    x = encoder(W, ops.musiq_embed_f32(emb, p["pos"], p["scale"], p["cls"], device_tables(geo, images.device, ("tokens",))[0]))
    return ops.layernorm_f32(x[:, 0], p["encoder_norm.weight"], p["encoder_norm.bias"], LN_EPS)


def musiq(W: MusiqWeights, pred: torch.Tensor, group: int | None = None, want_features: bool = False):
    """MUSIQ per image -> float64 [N] on the device, higher is better.  ``pred``: [N,C,H,W] float in [0,1] or uint8 (any strides, C in
    {1, 3}; one channel is repeated), or [F,H,W,3] uint8 frames; a host tensor is uploaded.  ``group``: frames per batch (default: from
    the budget).  ``want_features``: also return the float32 [N,384] normalised token 0."""
    if not isinstance(W, MusiqWeights):
        raise TypeError(f"musiq: weights must be MusiqWeights, got {type(W).__name__}")
    x = iqa.images(pred, "musiq", dtypes=(torch.uint8, torch.float32, torch.bfloat16))      # any size from 1 x 1; the patch kernel reads bfloat16 too
    W = W.to(x.device)
    feats = torch.empty(x.shape[0], DIM, dtype=torch.float32, device=x.device)

    def per_group(i, j):
        feats[i:j] = features(W, x[i:j])

    for_groups(x.shape[0], group, group_size(x.shape[2], x.shape[3]), COUNTERS, x.device, per_group)
    with torch.cuda.device(x.device):
        out = ops.musiq_score(feats, W.params["head.weight"], W.params["head.bias"])
    return (out, feats) if want_features else out


class MusiqMetric(GpuMetric):
    """pyiqa-style metric object: ``metric(pred)`` with [N,C,H,W] images in [0,1] (host or device) -> [N] fp64 MUSIQ scores."""

    def __init__(self, weights: MusiqWeights):
        super().__init__("musiq", False, False, musiq, weights, MusiqWeights)


def main(argv=None):
    ap = argparse.ArgumentParser(description="MUSIQ on the GPU (dove_amd): score images")
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("score", help="score every image of a folder")
    s.add_argument("--pred", required=True, help="folder of images")
    s.add_argument("--metric_weights", required=True, help=f"directory with {FILE_PATTERN}")
    args = ap.parse_args(argv)
    return score_folder(args, lambda a: MusiqWeights.load(a.metric_weights), musiq)


if __name__ == "__main__":
    main()
