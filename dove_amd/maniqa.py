"""The no-reference metric MANIQA (pyiqa's ``maniqa``: a ViT-B/8 trunk, transposed "channel" attention blocks, two 2-D Swin stages and a
weighted patch head) on the GPU in exact fp32 (csrc/maniqa.hip beside the fp32 metric block of csrc/musiq.hip, csrc/conv_f32.hip and
csrc/swin3d.hip).

Neither pyiqa nor timm nor a checkpoint were at hand: the network is restated from memory of pyiqa's ``maniqa_arch.py`` and IIGROUP/MANIQA
(``maniqa.py``, ``swin.py``); tests/maniqa_ref.py is the definition that the kernels are pinned to, and agreement with the published model
is unchecked (INTEGRATION.md 1o lists every choice; each is a module-level constant, a ``cfg`` entry or one small function here).  As
remembered:

  images in [0,1] (one channel is repeated) -> v' = (v - 0.5) / 0.5; ``NUM_CROPS`` crops of 224 x 224 on pyiqa's ``uniform_crop`` grid
    (``crop_origins``); a frame's score is the mean over its crops; a frame below 224 on a side is refused (the original upsamples it);
  trunk: timm ``vit_base_patch8_224``: Conv 8 x 8 stride 8, a cls token, pos_embed [1,785,768], pre-LN blocks (LayerNorm eps 1e-6, 12
    heads of 64, qkv bias, MLP 768 -> 3072 -> 768, exact-erf GELU); the outputs of blocks 6 .. 9 without the cls row, side by side, are
    the [784,3072] feature; blocks 10, 11 and the final norm are never run (the loader accepts their keys and drops them);
  ``b (h w) c -> b c (h w)``, then ``NUM_TAB`` TABlocks of dim 784: q, k, v = Linear(784, 784) of the [C,784] channel rows, A =
    softmax(q k^T 784^-0.5) of size C x C, y = A v, then ``y.transpose(1, 2).reshape(B, C, N)`` - a reinterpretation of the dense [N,C]
    buffer as [C,N], no transpose back (``TAB_RESHAPE_QUIRK``) - and + x;
  conv1 1 x 1 3072 -> 768; swintransformer1: ``swin_layers`` BasicLayers of depth 2 (shift 0 and window // 2, window 4, 4 heads, the
    relative position bias table, the -100 shift mask, MLP hidden ``dim_mlp`` = 768, LayerNorm eps 1e-5), each applied as x =
    ``SWIN_SCALE`` layer(x) + x; two TABlocks at C = 768; conv2 1 x 1 768 -> 384; swintransformer2 at dim 384;
  per position f = ReLU(Linear(384,1)(ReLU(Linear(384,384)))), w = Sigmoid(Linear(384,1)(ReLU(Linear(384,384)))); the crop's score is
    sum f w / sum w over the 784 positions.  Higher is better.

The user supplies the checkpoint (``maniqa*.pth`` / ``ckpt_koniq10k*.pt``).  This module walks the network in Python; every operator is a
kernel of the library, and all crops of a group of frames go through each of them in one launch.  MANIQA is not in ``metrics.REGISTRY``
yet: ``ManiqaMetric`` and ``ManiqaWeights.load`` are what one ``MetricSpec`` line will need."""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import iqa, ops
from .fastvqa import geometry
from .iqa import ACTIVATION_BUDGET, GpuMetric, find_file, for_groups, load_state_dict, process_clips, score_folder
from .netweights import Weights, checked, device_tables, fan_in_normal, pack_linear_weight, prenorm_mlp_f32, random_tensors, strip

NUM_CROPS = 20                                      # pyiqa's test-time crops of its default MANIQA (from memory)
NUM_TAB = 2                                         # TABlocks per stage
TAB_RESHAPE_QUIRK = True                            # the original's ``transpose(1, 2).reshape(B, C, N)`` after A v
SWIN_SCALE = 0.8                                    # x = SWIN_SCALE layer(x) + x (the original's default; the checkpoint's value is unchecked)
VIT_LN_EPS, SWIN_LN_EPS = 1e-6, 1e-5
VIT_HEAD_DIM = 64                                   # ops.mha_f32's head width
FILE_PATTERNS = ("maniqa*.pth", "ckpt_koniq10k*.pt")
OUT_NAME = "metrics_maniqa.json"
KEYS = ("maniqa",)
COUNTERS = {"groups": 0}                            # groups walked, for tests and tools
# ``blocks``: the ViT blocks of the checkpoint; only those up to the last hook are run.  ``swin_layers``: BasicLayers per Swin stage.
CFG = {"side": 224, "patch": 8, "dim": 768, "heads": 12, "blocks": 12, "hooks": (6, 7, 8, 9), "mlp_ratio": 4, "window": 4,
       "swin_heads": (4, 4), "swin_layers": 1, "swin_depth": 2, "dim_mlp": 768, "crops": NUM_CROPS}


def check_cfg(cfg: dict) -> dict:
    side, patch, dim = cfg["side"], cfg["patch"], cfg["dim"]
    t = (side // patch) ** 2
    widths = (dim, dim // 2)
    if side % patch or dim != cfg["heads"] * VIT_HEAD_DIM or len(cfg["hooks"]) != 4 or max(cfg["hooks"]) >= cfg["blocks"] or t % 4 or \
            any(c % (32 * h) or c // h > 192 for c, h in zip(widths, cfg["swin_heads"])) or cfg["dim_mlp"] % 32 or (3 * patch * patch) % 32:
        raise ValueError(f"maniqa: unsupported configuration {cfg}: the ViT's heads are {VIT_HEAD_DIM} wide, the token count a multiple of 4, "
                         f"the Swin heads multiples of 32 up to 192, dim_mlp and 3 patch^2 multiples of 32")
    return cfg


def tokens_of(cfg: dict) -> int:
    return (cfg["side"] // cfg["patch"]) ** 2


# ------------------------------------------------------------------ geometry ------------------------------------------------------------------
def crop_origins(H: int, W: int, side: int = CFG["side"], crops: int = NUM_CROPS) -> np.ndarray:
    """int32 [crops,2] (row, column) of pyiqa's ``uniform_crop`` (from memory): steps (H - side) // int(sqrt(crops)) and likewise for W, a
    ceil(sqrt(crops))-square grid walked row-major, its first ``crops`` cells.  Every crop lies inside the frame."""
    if H < side or W < side:
        raise ValueError(f"maniqa: frames of {H} x {W} are smaller than the {side} x {side} crop; the original upsamples such a frame first, "
                         f"which is not built")
    lo, hi = int(math.sqrt(crops)), int(math.ceil(math.sqrt(crops)))
    sh, sw = (H - side) // lo, (W - side) // lo
    cells = [(i * sh, j * sw) for i in range(hi) for j in range(hi)][:crops]
    out = np.asarray(cells, dtype=np.int32).reshape(crops, 2)
    assert out.min() >= 0 and out[:, 0].max() <= H - side and out[:, 1].max() <= W - side
    return out


_ORIGINS = {}


def _origins_on(H: int, W: int, cfg: dict, device) -> torch.Tensor:
    key = (int(H), int(W), cfg["side"], cfg["crops"])
    if key not in _ORIGINS:
        _ORIGINS[key] = {"origins": crop_origins(*key), "device": {}}
    return device_tables(_ORIGINS[key], device, ("origins",))[0]


def group_size(cfg: dict = CFG, budget: int | None = None) -> int:
    """Frames per group: the most whose live fp32 activations stay under the budget, at least one.  The peak is the first TAB stage, where
    a crop holds its C x T channel rows (C = 4 dim), their q, k, v (3 C T) and the C x C score matrix: C (C + 4 T) floats, 76 MB at the
    real configuration (37.7 MB of it the scores), 20 crops per frame: two frames fit 4 GiB.  The trunk before it (the token rows, their
    QKV and the MLP's hidden rows: 9 (T + 1) dim floats beside the C T feature) and every later stage hold less."""
    C, T = 4 * cfg["dim"], tokens_of(cfg)
    return max(1, int((ACTIVATION_BUDGET if budget is None else budget) // (4 * cfg["crops"] * C * (C + 4 * T))))


# ------------------------------------------------------------------- weights -------------------------------------------------------------------
def _swin_blocks(cfg: dict):
    """(stage prefix, width, heads) of the two Swin stages, and per stage its block prefixes with their shifted flag."""
    for s, (c, h) in enumerate(zip((cfg["dim"], cfg["dim"] // 2), cfg["swin_heads"])):
        name = f"swintransformer{s + 1}"
        yield name, c, h, [[(f"{name}.layers.{l}.blocks.{j}", j % 2 == 1) for j in range(cfg["swin_depth"])] for l in range(cfg["swin_layers"])]


def param_shapes(cfg: dict = CFG, all_blocks: bool = False) -> dict:
    """name -> shape of the entries of pyiqa's MANIQA state dict that the network reads (names from memory: INTEGRATION.md 1o).
    ``all_blocks``: with the ViT blocks behind the last hook and the ViT's final norm, which a checkpoint has and the walk never needs."""
    check_cfg(cfg)
    dim, T, P = cfg["dim"], tokens_of(cfg), cfg["patch"]
    s = {"vit.patch_embed.proj.weight": (dim, 3, P, P), "vit.patch_embed.proj.bias": (dim,), "vit.cls_token": (1, 1, dim),
         "vit.pos_embed": (1, T + 1, dim)}
    for i in range(cfg["blocks"] if all_blocks else max(cfg["hooks"]) + 1):
        p = f"vit.blocks.{i}"
        for n in ("norm1", "norm2"):
            s[f"{p}.{n}.weight"], s[f"{p}.{n}.bias"] = (dim,), (dim,)
        s[f"{p}.attn.qkv.weight"], s[f"{p}.attn.qkv.bias"] = (3 * dim, dim), (3 * dim,)
        s[f"{p}.attn.proj.weight"], s[f"{p}.attn.proj.bias"] = (dim, dim), (dim,)
        s[f"{p}.mlp.fc1.weight"], s[f"{p}.mlp.fc1.bias"] = (cfg["mlp_ratio"] * dim, dim), (cfg["mlp_ratio"] * dim,)
        s[f"{p}.mlp.fc2.weight"], s[f"{p}.mlp.fc2.bias"] = (dim, cfg["mlp_ratio"] * dim), (dim,)
    if all_blocks:
        s["vit.norm.weight"], s["vit.norm.bias"] = (dim,), (dim,)
    for stage in (1, 2):
        for i in range(NUM_TAB):
            for n in ("c_q", "c_k", "c_v"):
                s[f"tablock{stage}.{i}.{n}.weight"], s[f"tablock{stage}.{i}.{n}.bias"] = (T, T), (T,)
    s["conv1.weight"], s["conv1.bias"] = (dim, 4 * dim, 1, 1), (dim,)
    s["conv2.weight"], s["conv2.bias"] = (dim // 2, dim, 1, 1), (dim // 2,)
    rows = (2 * cfg["window"] - 1) ** 2
    for _, c, h, layers in _swin_blocks(cfg):
        for p, _ in (b for layer in layers for b in layer):
            for n in ("norm1", "norm2"):
                s[f"{p}.{n}.weight"], s[f"{p}.{n}.bias"] = (c,), (c,)
            s[f"{p}.attn.relative_position_bias_table"] = (rows, h)
            s[f"{p}.attn.qkv.weight"], s[f"{p}.attn.qkv.bias"] = (3 * c, c), (3 * c,)
            s[f"{p}.attn.proj.weight"], s[f"{p}.attn.proj.bias"] = (c, c), (c,)
            s[f"{p}.mlp.fc1.weight"], s[f"{p}.mlp.fc1.bias"] = (cfg["dim_mlp"], c), (cfg["dim_mlp"],)
            s[f"{p}.mlp.fc2.weight"], s[f"{p}.mlp.fc2.bias"] = (c, cfg["dim_mlp"]), (c,)
    c2 = dim // 2
    for n in ("fc_score", "fc_weight"):
        s[f"{n}.0.weight"], s[f"{n}.0.bias"], s[f"{n}.3.weight"], s[f"{n}.3.bias"] = (c2, c2), (c2,), (1, c2), (1,)
    return s


def random_state(cfg: dict, seed: int, all_blocks: bool = False, only: tuple | None = None) -> dict:
    """Rule-generated state dict for tests and tools: matrices normal with std 1 / sqrt(fan-in), norm weights uniform in [0.5, 1.5], biases
    0.05 * normal, the bias tables normal with std 1, cls and pos_embed normal with std 0.5.  The TABlocks' c_q and c_k get std 1 / (2
    sqrt(fan-in)): their inputs are rows of the residual stream after several blocks, a few units large, and a quarter of the plain draw's
    score variance keeps the C x C softmax between uniform and one-hot (tests/test_maniqa_cpu.py asserts it under the fp64 restatement).
    Each tensor has its own generator keyed by (seed, name), so ``only`` (name prefixes) draws a part of the same state."""
    def rule(name, shape, rng):
        if name.endswith("_bias_table"):
            return rng.standard_normal(shape)
        if name.endswith(("cls_token", "pos_embed")):
            return 0.5 * rng.standard_normal(shape)
        if len(shape) >= 2:
            return fan_in_normal(rng, shape) * (0.5 if ".c_q." in name or ".c_k." in name else 1.0)
        return rng.uniform(0.5, 1.5, shape) if name.endswith(".weight") else 0.05 * rng.standard_normal(shape)

    shapes = {k: v for k, v in param_shapes(cfg, all_blocks).items() if only is None or k.startswith(tuple(only))}
    return random_tensors(shapes, seed, lambda name: f"maniqa.{name}", rule)


@dataclass
class ManiqaWeights(Weights):
    """``params``: every tensor the walk reads, by its published name where it is kept as it is.  Linear weights are transposed to the
    GEMM's [1,1,in,out]; a TABlock's c_q, c_k, c_v are one [in,3 out] matrix ``tablockS.I.qkv`` (each output column is still its own k-ordered
    chain); conv1 and conv2 stay [out,in] (they are the A operand); the two heads' hidden Linears are one GEMM ``head.hidden``."""
    cfg: dict = field(default_factory=lambda: dict(CFG))
    params: dict = field(default_factory=dict)

    @classmethod
    def from_state_dict(cls, sd: dict, cfg: dict | None = None, partial: bool = False) -> "ManiqaWeights":
        """``partial``: pack the entries that ``sd`` has (whole blocks of them) instead of refusing a missing one: for tests and tools that
        walk one stage."""
        cfg = dict(CFG if cfg is None else cfg)
        sd = strip(sd["params"] if isinstance(sd.get("params"), dict) else sd)
        want = param_shapes(cfg)
        if partial:
            want = {k: v for k, v in want.items() if k in sd}
        sd = checked(sd, want, "MANIQA checkpoint")                         # entries beyond these (blocks 10, 11, vit.norm, buffers) are dropped
        f32 = lambda t: t.detach().float().contiguous()
        lin = pack_linear_weight
        T, dim = tokens_of(cfg), cfg["dim"]
        p = {}
        if "vit.pos_embed" in want:
            p.update({"patch.weight": lin(sd["vit.patch_embed.proj.weight"]), "patch.bias": f32(sd["vit.patch_embed.proj.bias"]),
                      "cls": f32(sd["vit.cls_token"]).reshape(dim), "pos": f32(sd["vit.pos_embed"]).reshape(T + 1, dim)})
        for name in want:
            t = sd[name]
            if name.startswith("vit.blocks.") or name.startswith("swintransformer"):
                p[name] = lin(t) if t.dim() == 2 and not name.endswith("_bias_table") else f32(t)
        for stage in (1, 2):
            for i in range(NUM_TAB):
                b = f"tablock{stage}.{i}"
                if f"{b}.c_q.weight" in want:
                    p[f"{b}.qkv.weight"] = f32(torch.cat([sd[f"{b}.{n}.weight"] for n in ("c_q", "c_k", "c_v")]).float().t())   # [T,3 T]
                    p[f"{b}.qkv.bias"] = f32(torch.cat([sd[f"{b}.{n}.bias"] for n in ("c_q", "c_k", "c_v")]))
        for n in ("conv1", "conv2"):
            if f"{n}.weight" in want:
                p[f"{n}.weight"], p[f"{n}.bias"] = f32(sd[f"{n}.weight"].flatten(1)), f32(sd[f"{n}.bias"])
        if "fc_score.0.weight" in want:
            p["head.hidden.weight"] = lin(torch.cat([sd["fc_score.0.weight"], sd["fc_weight.0.weight"]]))
            p["head.hidden.bias"] = f32(torch.cat([sd["fc_score.0.bias"], sd["fc_weight.0.bias"]]))
            for short, n in (("f", "fc_score"), ("w", "fc_weight")):
                p[f"head.{short}.weight"], p[f"head.{short}.bias"] = f32(sd[f"{n}.3.weight"].flatten()), f32(sd[f"{n}.3.bias"])
        return cls(cfg=cfg, params=p)

    @classmethod
    def load(cls, directory: str, cfg: dict | None = None) -> "ManiqaWeights":
        """From a ``--metric_weights`` directory: the first ``maniqa*.pth``, else ``ckpt_koniq10k*.pt`` (a top-level ``params`` or
        ``state_dict`` is unwrapped)."""
        return cls.from_state_dict(load_state_dict(find_file(directory, FILE_PATTERNS)), cfg)


# -------------------------------------------------------------------- walk --------------------------------------------------------------------
def vit_block(W: ManiqaWeights, x: torch.Tensor, i: int) -> torch.Tensor:
    """One pre-LN ViT block on the token rows float32 [B,T + 1,dim], changed in place."""
    B, T1, dim = x.shape
    P, b, rows = W.params, f"vit.blocks.{i}", x.view(-1, dim)
    h = ops.layernorm_f32(rows, P[f"{b}.norm1.weight"], P[f"{b}.norm1.bias"], VIT_LN_EPS)
    qkv = ops.linear_f32(h, P[f"{b}.attn.qkv.weight"], P[f"{b}.attn.qkv.bias"]).view(B, T1, 3 * dim)
    a = ops.mha_f32(qkv[..., :dim], qkv[..., dim:2 * dim], qkv[..., 2 * dim:], 1.0 / math.sqrt(VIT_HEAD_DIM))
    del qkv
    ops.linear_f32(a.view(-1, dim), P[f"{b}.attn.proj.weight"], P[f"{b}.attn.proj.bias"], residual=rows, out=rows)
    del a
    prenorm_mlp_f32(rows, h, P, f"{b}.norm2", f"{b}.mlp.fc1", f"{b}.mlp.fc2", VIT_LN_EPS)
    return x


def hook_gather(x: torch.Tensor, feat: torch.Tensor, slot: int) -> None:
    """Token rows [B,T + 1,dim] without the cls row -> channel rows ``slot`` dim .. of feat [B,4 dim,T] (the transposing copy)."""
    dim = x.shape[2]
    ops.mix_f32(x[:, 1:], transpose=True, out=feat[:, slot * dim:(slot + 1) * dim])


def trunk(W: ManiqaWeights, images: torch.Tensor) -> torch.Tensor:
    """A group of frames on W's device -> the hooked blocks' features as channel rows float32 [g crops,4 dim,T]."""
    cfg, P = W.cfg, W.params
    cols = ops.maniqa_crops_f32(images, _origins_on(images.shape[2], images.shape[3], cfg, images.device), cfg["side"], cfg["patch"])
    emb = ops.linear_f32(cols, P["patch.weight"], P["patch.bias"])
    del cols
    x = ops.maniqa_tokens_f32(emb, P["cls"], P["pos"])
    del emb
    feat = torch.empty(x.shape[0], 4 * cfg["dim"], tokens_of(cfg), dtype=torch.float32, device=x.device)
    for i in range(max(cfg["hooks"]) + 1):
        vit_block(W, x, i)
        if i in cfg["hooks"]:
            hook_gather(x, feat, cfg["hooks"].index(i))
    return feat


def tablock(W: ManiqaWeights, x: torch.Tensor, name: str) -> torch.Tensor:
    """One TABlock on channel rows float32 [B,C,T], changed in place."""
    B, Cc, T = x.shape
    P = W.params
    qkv = ops.bmm_f32(x.view(B * Cc, T), P[f"{name}.qkv.weight"], bias=P[f"{name}.qkv.bias"]).view(B, Cc, 3 * T)
    s = ops.bmm_f32(qkv[..., :T], qkv[..., T:2 * T], b_transposed=True, alpha=float(T) ** -0.5)                  # [B,C,C]
    ops.softmax_rows_f32(s.view(B * Cc, Cc), out=s.view(B * Cc, Cc))
    if TAB_RESHAPE_QUIRK:           # (A v)^T stored dense as [T,C] and read back as [C,T]: the transposed store onto x's own memory
        flat = x.view(B, T, Cc)
        ops.bmm_f32(s, qkv[..., 2 * T:], store_transposed=True, residual=flat, out=flat)
    else:
        ops.bmm_f32(s, qkv[..., 2 * T:], residual=x, out=x)
    return x


def swin_block(W: ManiqaWeights, x: torch.Tensor, p: str, heads: int, shifted: bool, in_place: bool) -> torch.Tensor:
    """One Swin block on the token map float32 [B,1,H,W,C]; ``in_place``: x is changed, else a new map is returned and x kept."""
    B, _, H, Wd, Cc = x.shape
    P = W.params
    w = W.cfg["window"]
    geo = geometry((1, H, Wd), (1, w, w), (1, 1), shifted)
    index, _, region = device_tables(geo, x.device, ("index", "frag", "region"))
    h = ops.layernorm_f32(x.view(-1, Cc), P[f"{p}.norm1.weight"], P[f"{p}.norm1.bias"], SWIN_LN_EPS)
    win = ops.swin3d_window_gather_f32(h.view(x.shape), geo["window"], geo["shift"])
    qkv = ops.linear_f32(win.view(-1, Cc), P[f"{p}.attn.qkv.weight"], P[f"{p}.attn.qkv.bias"]).view(win.shape[0], geo["length"], 3 * Cc)
    a = ops.window_attention_f32(qkv, heads, P[f"{p}.attn.relative_position_bias_table"], index, region=region)
    del qkv
    ops.linear_f32(a.view(-1, Cc), P[f"{p}.attn.proj.weight"], P[f"{p}.attn.proj.bias"], out=win.view(-1, Cc))
    del a
    y = ops.swin3d_window_scatter_f32(win, x, geo["window"], geo["shift"], out=x if in_place else None)
    del win
    prenorm_mlp_f32(y.view(-1, Cc), h, P, f"{p}.norm2", f"{p}.mlp.fc1", f"{p}.mlp.fc2", SWIN_LN_EPS)
    return y


def swin_stage(W: ManiqaWeights, x: torch.Tensor, stage: int, channel_rows: bool) -> torch.Tensor:
    """Token rows float32 [B,T,C] through Swin stage ``stage`` (0, 1): per BasicLayer x = SWIN_SCALE layer(x) + x.  ``channel_rows``: the
    result is transposed to [B,C,T] by the last layer's scale-and-add."""
    B, T, Cc = x.shape
    side = W.cfg["side"] // W.cfg["patch"]
    _, _, heads, layers = list(_swin_blocks(W.cfg))[stage]
    for l, blocks in enumerate(layers):
        y = x.view(B, 1, side, side, Cc)
        for j, (p, shifted) in enumerate(blocks):
            y = swin_block(W, y, p, heads, shifted, in_place=j > 0)
        y = y.view(B, T, Cc)
        last = l == len(layers) - 1
        x = ops.mix_f32(y, x, SWIN_SCALE, transpose=True) if last and channel_rows else ops.mix_f32(y, x, SWIN_SCALE, out=y)
    return x


def conv1x1(W: ManiqaWeights, x: torch.Tensor, name: str) -> torch.Tensor:
    """Channel rows float32 [B,C,T] -> token rows [B,T,C'] of the 1 x 1 conv: the weight is the GEMM's shared A, the store is transposed."""
    return ops.bmm_f32(W.params[f"{name}.weight"], x, bias=W.params[f"{name}.bias"], bias_rows=True, store_transposed=True)


def hidden_rows(W: ManiqaWeights, feat: torch.Tensor) -> torch.Tensor:
    """The trunk's channel rows [B,4 dim,T] (consumed) -> the two heads' ReLU'd hidden units per position, float32 [B,T,dim]."""
    x = feat
    for i in range(NUM_TAB):
        tablock(W, x, f"tablock1.{i}")
    x = swin_stage(W, conv1x1(W, x, "conv1"), 0, channel_rows=True)
    for i in range(NUM_TAB):
        tablock(W, x, f"tablock2.{i}")
    x = swin_stage(W, conv1x1(W, x, "conv2"), 1, channel_rows=False)
    B, T, c2 = x.shape
    return ops.linear_f32(x.view(B * T, c2), W.params["head.hidden.weight"], W.params["head.hidden.bias"], relu=True).view(B, T, 2 * c2)


def head(W: ManiqaWeights, hidden: torch.Tensor, crops: int) -> torch.Tensor:
    """Hidden units float32 [g crops,T,2 c] -> float64 [g]: the weighted head in fp64 and the mean over each frame's crops."""
    P = W.params
    return ops.maniqa_score(hidden.view(hidden.shape[0] // crops, crops, hidden.shape[1], hidden.shape[2]), P["head.f.weight"], P["head.f.bias"],
                            P["head.w.weight"], P["head.w.bias"])


def maniqa(W: ManiqaWeights, pred: torch.Tensor, group: int | None = None) -> torch.Tensor:
    """MANIQA per image -> float64 [N] on the device, higher is better.  ``pred``: [N,C,H,W] float in [0,1] or uint8 (any strides, C in
    {1, 3}; one channel is repeated), or [F,H,W,3] uint8 frames, at least 224 x 224 (the configuration's crop side); a host tensor is
    uploaded.  ``group``: frames per batch (default: from the budget); a frame's value does not depend on it."""
    if not isinstance(W, ManiqaWeights):
        raise TypeError(f"maniqa: weights must be ManiqaWeights, got {type(W).__name__}")
    side = W.cfg["side"]
    x = iqa.images(pred, "maniqa", min_hw=(side, side), dtypes=(torch.uint8, torch.float32, torch.bfloat16))
    W = W.to(x.device)
    out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)

    def per_group(i, j):
        out[i:j] = head(W, hidden_rows(W, trunk(W, x[i:j])), W.cfg["crops"])

    for_groups(x.shape[0], group, group_size(W.cfg), COUNTERS, x.device, per_group)
    return out


class ManiqaMetric(GpuMetric):
    """pyiqa-style metric object: ``metric(pred)`` with [N,C,H,W] images in [0,1] (host or device) -> [N] fp64 MANIQA scores."""

    def __init__(self, weights: ManiqaWeights):
        super().__init__("maniqa", False, False, maniqa, weights, ManiqaWeights)


# ------------------------------------------------------------------ the tools ------------------------------------------------------------------
def evaluate(pred_root: str, out_path: str, score_fn, side: int = CFG["side"]) -> dict:
    """Every clip of ``pred_root`` -> ``metrics_maniqa.json`` in ``eval_metrics``' shape {per_sample, average, count}: a clip's value is
    the mean of ``score_fn(frames_u8)`` over its frames, rounded to 4 places.  A clip below the crop side is reported and left out."""
    def clip(name, frames):
        if frames.shape[1] < side or frames.shape[2] < side:
            raise ValueError(f"maniqa: frames of {frames.shape[1]} x {frames.shape[2]} are smaller than the {side} x {side} crop")
        vals = [float(v) for v in score_fn(frames)]
        s = 0.0
        for v in vals:                                   # frame order
            s += v
        return {"maniqa": round(s / len(vals), 4)}

    return process_clips(pred_root, out_path, OUT_NAME, KEYS, clip)


def main(argv=None, score_fn=None):
    ap = argparse.ArgumentParser(description="MANIQA on the GPU (dove_amd): score images or clips")
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("score", help="score every image of a folder")
    s.add_argument("--pred", required=True, help="folder of images")
    e = sub.add_parser("eval", help="score every clip of a root (PNG/JPG folders, .npy or .y4m files) and write metrics_maniqa.json")
    e.add_argument("--pred", required=True, help="folder of clips")
    e.add_argument("--out", default="", help="directory of the JSON output; default: --pred")
    for p in (s, e):
        p.add_argument("--metric_weights", required=True, help=f"directory with {' or '.join(FILE_PATTERNS)}")
    args = ap.parse_args(argv)
    if args.cmd == "score":
        return score_folder(args, lambda a: ManiqaWeights.load(a.metric_weights), maniqa)
    side = CFG["side"]
    if score_fn is None:
        weights = ManiqaWeights.load(args.metric_weights)
        side = weights.cfg["side"]
        score_fn = lambda frames: maniqa(weights, frames).cpu().tolist()
    return evaluate(args.pred, args.out or args.pred, score_fn, side)


if __name__ == "__main__":
    main()
