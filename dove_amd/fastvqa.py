"""The no-reference video metrics FasterVQA and FAST-VQA (the FAST-VQA repository's fragment sampling plus a Video Swin-T with gated
relative position bias, GRPB) on the GPU in exact fp32 (csrc/swin3d.hip and the fp32 GEMM of csrc/conv_f32.hip).

Neither the FAST-VQA sources nor a checkpoint were at hand: the network is restated from memory, tests/fastvqa_ref.py is the definition
that the kernels are pinned to, and agreement with the published model on real weights is unchecked (INTEGRATION.md 1m lists every
choice).  As remembered:

  sampling: a gh x gw grid of fh x fw pixel fragments per frame, cell origin H // gh * i clamped to H - fh plus a uniform integer in
    [0, H // gh - fh) per (cell, temporal group); frames (255 v - mean) / std.  ``FasterVQA``: 32 frames as 8 temporal groups of 4 at
    interval 2 (a random start inside each eighth of the clip), one clip, window (4,4,4).  ``FAST-VQA``: 4 clips of 32 frames at
    interval 2 from evenly spaced starts, one offset per clip, window (8,7,7), the clips' scores averaged.  Frame indices wrap modulo
    the clip's length.  A frame smaller than the canvas is refused (the original upsamples it).
  network: Conv3d (2,4,4) stride (2,4,4) patch embedding with a patch norm, width 96, depths [2,2,6,2], heads [3,6,12,24] of 32, MLP
    ratio 4, qkv bias, blocks alternating shift 0 and window // 2 with the -100 mask, zero padding to whole windows after norm1 (the
    padded tokens take part as keys), patch merging between stages, a final LayerNorm, no temporal downsampling; in stages 0-2 a second
    bias table (``fragment_position_bias_table``) serves token pairs from different fragments (``geometry`` makes the fragment ids; the
    exact gate of the original is the main doubt); head fc_hid 768 -> 64, exact-erf GELU, fc_last 64 -> 1, the mean over all tokens, in fp64.

Random draws come from ``numpy.random.Generator(PCG64(seed))`` in the order ``sample_draws`` documents: the original's distributions, not
its global random streams.  The user supplies the checkpoint.  This module walks the network in Python; every operator is a kernel."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import iqa, ops
from .iqa import ACTIVATION_BUDGET, for_groups, load_state_dict
from .netweights import Weights, checked, device_tables, fan_in_normal, nearest_index, pack_linear_weight, prenorm_mlp_f32, random_tensors, strip

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
LN_EPS = 1e-5
HEAD_DIM = 32
PATCH = (2, 4, 4)
PREFIX = "fragments_backbone."
# Live fp32 activations per patch-embedded token of the first stage, in units of the width: the map, its normalised copy, the MLP's
# hidden rows (4) or the window rows, their QKV (3) and the attention output: 8 widths at the peak (a later stage holds fewer).
TOKEN_WIDTHS = 8
COUNTERS = {"groups": 0}
# (mean, std) of the sigmoid rescaling 1 / (1 + exp(-(s - mean) / std)), from memory: ``--rescale_mean`` / ``--rescale_std`` override them
RESCALE = {"FasterVQA": (0.14759505, 0.03613452), "FAST-VQA": (-0.110198185, 0.04178565)}


@dataclass(frozen=True)
class VqaConfig:
    name: str = "FasterVQA"
    fragments: tuple = (7, 7)          # gh, gw
    fsize: tuple = (32, 32)            # fh, fw
    clip_len: int = 32
    t_groups: int = 8                  # temporal groups of a clip, each with its own spatial offsets; 1: consecutive frames, one offset
    frame_interval: int = 2
    num_clips: int = 1
    window: tuple = (4, 4, 4)
    width: int = 96
    depths: tuple = (2, 2, 6, 2)
    heads: tuple = (3, 6, 12, 24)
    mlp_ratio: int = 4
    frag_stages: tuple = (0, 1, 2)     # the stages whose blocks carry fragment_position_bias_table
    head_hidden: int = 64
    rescale: tuple = RESCALE["FasterVQA"]

    def __post_init__(self):
        if len(self.depths) != len(self.heads) or any(self.width * 2 ** i != h * HEAD_DIM for i, h in enumerate(self.heads)):
            raise ValueError(f"VqaConfig: every head must be {HEAD_DIM} wide (width {self.width}, heads {self.heads})")
        if self.clip_len % self.t_groups or self.clip_len % PATCH[0] or any(f % PATCH[1] for f in self.fsize) or self.width % 32:
            raise ValueError("VqaConfig: clip_len must split into t_groups and patches of 2 frames, fsize into 4 x 4 patches, width % 32 == 0")

    @property
    def canvas(self):
        return self.fragments[0] * self.fsize[0], self.fragments[1] * self.fsize[1]

    @property
    def dims(self):
        """The width of every stage."""
        return tuple(self.width * 2 ** i for i in range(len(self.depths)))


PRESETS = {"FasterVQA": VqaConfig(),
           "FAST-VQA": VqaConfig(name="FAST-VQA", t_groups=1, num_clips=4, window=(8, 7, 7), rescale=RESCALE["FAST-VQA"])}


def preset(name: str) -> VqaConfig:
    if name not in PRESETS:
        raise ValueError(f"unknown variant {name!r}: choose one of {', '.join(PRESETS)}")
    return PRESETS[name]


# ------------------------------------------------------------------ sampling ------------------------------------------------------------------
def _check_frame(H: int, W: int, cfg: VqaConfig):
    Hc, Wc = cfg.canvas
    if H < Hc or W < Wc:
        raise ValueError(f"{cfg.name}: frames of {H} x {W} are smaller than the {Hc} x {Wc} fragment canvas; the original upsamples such a "
                         f"clip first, which is not built")


def sample_draws(num_frames: int, H: int, W: int, cfg: VqaConfig, seed: int) -> list:
    """The random integers of a plan, one dict per clip, from ``numpy.random.Generator(PCG64(seed))`` in this order: per clip, ``t``
    (t_groups starts in [0, num_frames // t_groups - frames per group * interval); only when t_groups > 1), then ``h`` [gh,gw,t_groups]
    in [0, H // gh - fh), then ``w`` likewise.  A range that is empty draws nothing and gives zeros."""
    _check_frame(H, W, cfg)
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    (gh, gw), (fh, fw), tg = cfg.fragments, cfg.fsize, cfg.t_groups
    span_t = num_frames // tg - cfg.clip_len // tg * cfg.frame_interval
    out = []
    for _ in range(cfg.num_clips):
        d = {"t": rng.integers(0, span_t, size=tg) if tg > 1 and span_t > 0 else np.zeros(tg, dtype=np.int64)}
        for key, span in (("h", H // gh - fh), ("w", W // gw - fw)):
            d[key] = rng.integers(0, span, size=(gh, gw, tg)) if span > 0 else np.zeros((gh, gw, tg), dtype=np.int64)
        out.append(d)
    return out


def sample_plan(num_frames: int, H: int, W: int, cfg: VqaConfig, seed: int = 42, draws: list | None = None):
    """(frame indices int32 [num_clips,clip_len], fragment origins int32 [num_clips,gh,gw,t_groups,2] (row, column)) of a clip of
    ``num_frames`` H x W frames.  Indices wrap modulo ``num_frames``; every fragment lies inside the frame."""
    if num_frames < 1:
        raise ValueError("a clip needs at least one frame")
    if draws is None:
        draws = sample_draws(num_frames, H, W, cfg, seed)
    _check_frame(H, W, cfg)
    (gh, gw), (fh, fw), tg, L_, iv = cfg.fragments, cfg.fsize, cfg.t_groups, cfg.clip_len, cfg.frame_interval
    frames = np.zeros((cfg.num_clips, L_), dtype=np.int64)
    origins = np.zeros((cfg.num_clips, gh, gw, tg, 2), dtype=np.int64)
    oy = np.minimum(H // gh * np.arange(gh), H - fh)[:, None, None]
    ox = np.minimum(W // gw * np.arange(gw), W - fw)[None, :, None]
    per = L_ // tg
    for c, d in enumerate(draws):
        if tg > 1:
            start = num_frames // tg * np.arange(tg) + np.asarray(d["t"])
            frames[c] = (start[:, None] + iv * np.arange(per)[None, :]).reshape(-1)
        else:
            full = (L_ - 1) * iv + 1
            gap = (num_frames - full + 1) / float(cfg.num_clips)
            frames[c] = (int(c * gap + gap / 2.0) if num_frames >= full else 0) + iv * np.arange(L_)
        origins[c, ..., 0] = oy + np.asarray(d["h"])
        origins[c, ..., 1] = ox + np.asarray(d["w"])
    frames %= num_frames
    assert origins.min() >= 0 and (origins[..., 0] + fh).max() <= H and (origins[..., 1] + fw).max() <= W
    return frames.astype(np.int32), origins.astype(np.int32)


# ------------------------------------------------------------------ geometry ------------------------------------------------------------------
def clamp_window(dims, window, shift):
    """Video Swin's get_window_size: an axis no longer than its window uses its own length and shift 0."""
    ws = tuple(d if d <= w else w for d, w in zip(dims, window))
    ss = tuple(0 if d <= w else s for d, w, s in zip(dims, window, shift))
    return ws, ss


def relative_index(window) -> np.ndarray:
    """[N,N] index into the (2 wd - 1)(2 wh - 1)(2 ww - 1)-row bias table of a full window."""
    wd, wh, ww = window
    n = np.arange(wd * wh * ww)
    pos = np.stack([n // (wh * ww), (n // ww) % wh, n % ww], 1)
    rel = pos[:, None, :] - pos[None, :, :] + np.array([wd - 1, wh - 1, ww - 1])
    return (rel[..., 0] * (2 * wh - 1) + rel[..., 1]) * (2 * ww - 1) + rel[..., 2]


_GEOMETRY = {}


def geometry(dims, window, fragments, shifted: bool) -> dict:
    """Host-side tables of one block on a D x H x W map: ``window`` and ``shift`` after the clamp, ``padded``, ``index`` int32 [N,N] (the
    configured window's index cut to [:N,:N], as Video Swin cuts it), ``frag`` int32 [nW,N] (the fragment of every window token: the
    fragment grid nearest-interpolated onto the padded map, seen through the roll) and ``region`` int32 [nW,N] (the shift region of
    every slot of the rolled map; ``None`` without a shift).  ``device``: the tables uploaded, per device."""
    key = (tuple(dims), tuple(window), tuple(fragments), bool(shifted))
    if key in _GEOMETRY:
        return _GEOMETRY[key]
    ws, ss = clamp_window(dims, window, tuple(w // 2 for w in window) if shifted else (0, 0, 0))
    padded, nW, N = ops.swin3d_padded(dims, ws)
    counts = tuple(p // w for p, w in zip(padded, ws))
    a, n = np.arange(nW)[:, None], np.arange(N)[None, :]
    slot = (a // (counts[1] * counts[2]) * ws[0] + n // (ws[1] * ws[2]),
            (a // counts[2]) % counts[1] * ws[1] + (n // ws[2]) % ws[1],
            a % counts[2] * ws[2] + n % ws[2])                                   # the position of every window slot in the rolled map
    src = [(p + s) % P for p, s, P in zip(slot, ss, padded)]                     # ... and in the padded map
    frag = nearest_index(padded[1], fragments[0])[src[1]] * fragments[1] + nearest_index(padded[2], fragments[1])[src[2]]
    region = None
    if any(ss):
        band = lambda p, P, w, s: np.where(p < P - w, 0, np.where(p < P - s, 1, 2)) if s else np.zeros_like(p)
        parts = [band(p, P, w, s) for p, P, w, s in zip(slot, padded, ws, ss)]
        region = ((parts[0] * 3 + parts[1]) * 3 + parts[2]).astype(np.int32)
    geo = {"window": ws, "shift": ss, "padded": padded, "windows": nW, "length": N,
           "index": np.ascontiguousarray(relative_index(window)[:N, :N]).astype(np.int32), "frag": frag.astype(np.int32), "region": region,
           "device": {}}
    _GEOMETRY[key] = geo
    return geo


# ------------------------------------------------------------------- weights -------------------------------------------------------------------
def param_shapes(cfg: VqaConfig) -> dict:
    """name -> shape of the entries of the published state dict that the network reads (names from memory: INTEGRATION.md 1m)."""
    s = {}
    b = PREFIX
    rows = (2 * cfg.window[0] - 1) * (2 * cfg.window[1] - 1) * (2 * cfg.window[2] - 1)
    s[b + "patch_embed.proj.weight"], s[b + "patch_embed.proj.bias"] = (cfg.width, 3) + PATCH, (cfg.width,)
    s[b + "patch_embed.norm.weight"], s[b + "patch_embed.norm.bias"] = (cfg.width,), (cfg.width,)
    for i, (depth, heads, C) in enumerate(zip(cfg.depths, cfg.heads, cfg.dims)):
        for j in range(depth):
            p = f"{b}layers.{i}.blocks.{j}"
            for n in ("norm1", "norm2"):
                s[f"{p}.{n}.weight"], s[f"{p}.{n}.bias"] = (C,), (C,)
            s[f"{p}.attn.relative_position_bias_table"] = (rows, heads)
            if i in cfg.frag_stages:
                s[f"{p}.attn.fragment_position_bias_table"] = (rows, heads)
            s[f"{p}.attn.qkv.weight"], s[f"{p}.attn.qkv.bias"] = (3 * C, C), (3 * C,)
            s[f"{p}.attn.proj.weight"], s[f"{p}.attn.proj.bias"] = (C, C), (C,)
            s[f"{p}.mlp.fc1.weight"], s[f"{p}.mlp.fc1.bias"] = (cfg.mlp_ratio * C, C), (cfg.mlp_ratio * C,)
            s[f"{p}.mlp.fc2.weight"], s[f"{p}.mlp.fc2.bias"] = (C, cfg.mlp_ratio * C), (C,)
        if i < len(cfg.depths) - 1:
            s[f"{b}layers.{i}.downsample.reduction.weight"] = (2 * C, 4 * C)
            s[f"{b}layers.{i}.downsample.norm.weight"], s[f"{b}layers.{i}.downsample.norm.bias"] = (4 * C,), (4 * C,)
    s[b + "norm.weight"], s[b + "norm.bias"] = (cfg.dims[-1],), (cfg.dims[-1],)
    s["vqa_head.fc_hid.weight"], s["vqa_head.fc_hid.bias"] = (cfg.head_hidden, cfg.dims[-1], 1, 1, 1), (cfg.head_hidden,)
    s["vqa_head.fc_last.weight"], s["vqa_head.fc_last.bias"] = (1, cfg.head_hidden, 1, 1, 1), (1,)
    return s


def random_state(cfg: VqaConfig, seed: int) -> dict:
    """Rule-generated state dict for tests and tools: matrices normal with std 1 / sqrt(fan-in), norm weights uniform in [0.5, 1.5],
    biases 0.05 * normal, bias tables normal with std 1 (so that the bias and the gate matter next to the scores).  Each tensor has its
    own generator keyed by (seed, name)."""
    def rule(name, shape, rng):
        if name.endswith("_bias_table"):
            return rng.standard_normal(shape)
        if len(shape) >= 2:
            return fan_in_normal(rng, shape)
        return rng.uniform(0.5, 1.5, shape) if name.endswith(".weight") else 0.05 * rng.standard_normal(shape)

    return random_tensors(param_shapes(cfg), seed, lambda name: f"fastvqa.{name}", rule)


@dataclass
class VqaWeights(Weights):
    """``params``: every tensor by its published name without the backbone prefix; Linear weights transposed to the GEMM's [1,1,in,out]."""
    cfg: VqaConfig = field(default_factory=VqaConfig)
    params: dict = field(default_factory=dict)

    @classmethod
    def from_state_dict(cls, sd: dict, cfg: VqaConfig | str = "FasterVQA") -> "VqaWeights":
        cfg = preset(cfg) if isinstance(cfg, str) else cfg
        sd = checked(strip(sd), param_shapes(cfg), f"{cfg.name} checkpoint")
        f32 = lambda t: t.detach().float().contiguous()
        p = {}
        for name in param_shapes(cfg):
            short = name[len(PREFIX):] if name.startswith(PREFIX) else name
            t = sd[name]
            if short == "vqa_head.fc_hid.weight":
                p[short] = f32(t.flatten(1))
            elif short == "vqa_head.fc_last.weight":
                p[short] = f32(t.flatten())
            else:
                p[short] = pack_linear_weight(t) if t.dim() >= 2 and not short.endswith("_bias_table") else f32(t)
        return cls(cfg=cfg, params=p)

    @classmethod
    def load(cls, path: str, cfg: VqaConfig | str = "FasterVQA") -> "VqaWeights":
        """From a checkpoint file in the published layout (a top-level ``state_dict`` is unwrapped)."""
        return cls.from_state_dict(load_state_dict(path), cfg)


# -------------------------------------------------------------------- walk --------------------------------------------------------------------
def _ln(W, name, rows, out=None):
    return ops.layernorm_f32(rows, W.params[name + ".weight"], W.params[name + ".bias"], LN_EPS, out=out)


def block(W: VqaWeights, x: torch.Tensor, p: str, heads: int, shifted: bool, gated: bool) -> torch.Tensor:
    """One Swin block on the token map float32 [B,D,H,W,C], changed in place."""
    B, D, H, Wd, C = x.shape
    P = W.params
    geo = geometry((D, H, Wd), W.cfg.window, W.cfg.fragments, shifted)
    index, frag, region = device_tables(geo, x.device, ("index", "frag", "region"))
    rows = x.view(-1, C)
    h = _ln(W, p + ".norm1", rows)
    win = ops.swin3d_window_gather_f32(h.view(x.shape), geo["window"], geo["shift"])
    qkv = ops.linear_f32(win.view(-1, C), P[p + ".attn.qkv.weight"], P[p + ".attn.qkv.bias"]).view(win.shape[0], geo["length"], 3 * C)
    a = ops.swin3d_window_attention_f32(qkv, heads, P[p + ".attn.relative_position_bias_table"], index,
                                        table_b=P[p + ".attn.fragment_position_bias_table"] if gated else None,
                                        frag=frag if gated else None, region=region)
    del qkv
    ops.linear_f32(a.view(-1, C), P[p + ".attn.proj.weight"], P[p + ".attn.proj.bias"], out=win.view(-1, C))
    del a
    ops.swin3d_window_scatter_f32(win, x, geo["window"], geo["shift"], out=x)
    del win
    prenorm_mlp_f32(rows, h, P, p + ".norm2", p + ".mlp.fc1", p + ".mlp.fc2", LN_EPS)
    return x


def patch_merge(W: VqaWeights, x: torch.Tensor, p: str) -> torch.Tensor:
    g = ops.swin3d_patch_merge_f32(x)
    rows = _ln(W, p + ".norm", g.view(-1, g.shape[-1]))
    return ops.linear_f32(rows, W.params[p + ".reduction.weight"]).view(*g.shape[:4], g.shape[-1] // 2)


def embed(W: VqaWeights, frames: torch.Tensor, frame_idx: torch.Tensor, origins: torch.Tensor) -> torch.Tensor:
    """One clip's fragments through the patch embedding (an im2col gather and one k-ordered fp32 FMA chain of 96 terms per output) and the
    patch norm -> token map float32 [1,T/2,Hc/4,Wc/4,width]."""
    cols = ops.vqa_fragments_f32(frames, frame_idx, origins, W.cfg.fsize, MEAN, STD, cols=True)
    x = ops.linear_f32(cols.view(-1, cols.shape[-1]), W.params["patch_embed.proj.weight"], W.params["patch_embed.proj.bias"])
    return _ln(W, "patch_embed.norm", x).view(1, *cols.shape[:3], W.cfg.width)


def backbone(W: VqaWeights, x: torch.Tensor, stages: int | None = None, blocks: int | None = None) -> torch.Tensor:
    """Patch-embedded map [B,D,H,W,width] (changed in place) -> the final-normed map [B,D,H',W',8 width].  ``stages`` = s stops after the
    blocks of stage s - 1 and returns that map; ``blocks``: at most this many blocks per stage (for tests)."""
    cfg = W.cfg
    n = len(cfg.depths)
    for i in range(n if stages is None else stages):
        for j in range(cfg.depths[i] if blocks is None else min(blocks, cfg.depths[i])):
            x = block(W, x, f"layers.{i}.blocks.{j}", cfg.heads[i], j % 2 == 1, i in cfg.frag_stages)
        if stages is not None and i == stages - 1:
            return x
        if i < n - 1:
            x = patch_merge(W, x, f"layers.{i}.downsample")
    return _ln(W, "norm", x.view(-1, x.shape[-1])).view(x.shape)


def head(W: VqaWeights, feat: torch.Tensor) -> torch.Tensor:
    """Final map [B,D,H,W,C] -> float64 [B]."""
    P = W.params
    return ops.vqa_head_f64(feat.view(feat.shape[0], -1, feat.shape[-1]), P["vqa_head.fc_hid.weight"], P["vqa_head.fc_hid.bias"],
                            P["vqa_head.fc_last.weight"], P["vqa_head.fc_last.bias"])


def group_size(cfg: VqaConfig, budget: int | None = None) -> int:
    """Clips per group: the most whose live activations (``TOKEN_WIDTHS`` widths per first-stage token) stay under the budget, at least one."""
    tokens = cfg.clip_len // PATCH[0] * (cfg.canvas[0] // PATCH[1]) * (cfg.canvas[1] // PATCH[2])
    return max(1, int((ACTIVATION_BUDGET if budget is None else budget) // (4 * TOKEN_WIDTHS * cfg.width * tokens)))


def clip_view(frames: torch.Tensor, name: str = "fastvqa") -> torch.Tensor:
    """uint8 [F,H,W,3] frames or an [F,3,H,W] batch in [0,1] (host or device) -> an [F,3,H,W] view on the device."""
    x = iqa.images(frames, name, dtypes=(torch.uint8, torch.float32, torch.bfloat16))
    if x.shape[1] != 3:
        raise ValueError(f"{name}: frames must have 3 channels, got {tuple(frames.shape)}")
    return x


def score_clip(frames: torch.Tensor, weights: VqaWeights, cfg: VqaConfig | None = None, seed: int = 42, plan=None, group: int | None = None,
               rescale: tuple | None = None):
    """(raw score, rescaled score) of one video, two Python floats (fp64).  ``frames``: uint8 [F,H,W,3] or [F,3,H,W] in [0,1], host or
    device.  ``plan``: a ``sample_plan`` result (default: drawn from ``seed``).  The raw score is the mean over the plan's clips of the
    head's output; the rescaled one is 1 / (1 + exp(-(raw - mean) / std)) with ``rescale`` = (mean, std), default the preset's.
    ``group``: clips per batch (default: from the budget); the values do not depend on it."""
    if not isinstance(weights, VqaWeights):
        raise TypeError(f"score_clip: weights must be VqaWeights, got {type(weights).__name__}")
    cfg = weights.cfg if cfg is None else cfg
    if cfg != weights.cfg:
        raise ValueError(f"score_clip: the weights were loaded for {weights.cfg.name}, not for this configuration")
    x = clip_view(frames)
    _check_frame(x.shape[2], x.shape[3], cfg)
    idx, org = sample_plan(x.shape[0], x.shape[2], x.shape[3], cfg, seed) if plan is None else plan
    W = weights.to(x.device)
    raw = torch.empty(len(idx), dtype=torch.float64, device=x.device)

    def per_group(i, j):
        maps = [embed(W, x, torch.from_numpy(idx[c]).to(x.device), torch.from_numpy(np.ascontiguousarray(org[c])).to(x.device))
                for c in range(i, j)]
        raw[i:j] = head(W, backbone(W, torch.cat(maps) if len(maps) > 1 else maps[0]))

    for_groups(len(idx), group, group_size(cfg), COUNTERS, x.device, per_group)
    vals = raw.cpu().tolist()
    s = 0.0
    for v in vals:                                   # clip order
        s += v
    s /= len(vals)
    mean, std = cfg.rescale if rescale is None else rescale
    return s, 1.0 / (1.0 + math.exp(-(s - mean) / std))


def with_rescale(cfg: VqaConfig, mean: float | None, std: float | None) -> tuple:
    return (cfg.rescale[0] if mean is None else float(mean), cfg.rescale[1] if std is None else float(std))
