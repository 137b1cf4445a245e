"""The no-reference video metric DOVER (a technical branch on fragments and an aesthetic branch on a resized view, fused) on the GPU in exact
fp32: the technical branch is dove_amd.fastvqa's Video Swin-T with window (8,7,7) under DOVER's sampler and key names; the aesthetic branch
is an inflated ConvNeXt-Tiny (csrc/convnext3d.hip for the depthwise 3 x 7 x 7 conv and the resized view, the fp32 GEMM, LayerNorm, GELU,
patch merge and fp64 head that FasterVQA already uses).

Neither the DOVER sources nor a checkpoint were at hand: the network is restated from memory, tests/dover_ref.py is the definition that the
kernels are pinned to, and agreement with the published ``DOVER.pth`` is unchecked (INTEGRATION.md 1n lists every choice).  As remembered:

  sampling: ``UnifiedFrameSampler(clip_len // t_frag, t_frag, interval, num_clips)``: t_frag temporal cells of F // t_frag frames, each
    giving clip_len // t_frag frames at the interval from a start that is random inside the cell when the cell is longer than that span
    (also at test time) and 0 otherwise; indices wrap modulo F.  Technical: t_frag 1, 3 clips of 32 frames at interval 2, 7 x 7 fragments of
    32 x 32 with fastvqa's spatial offsets.  Aesthetic: t_frag 32, one clip of 32 frames, each resized to 224 x 224 (bilinear, antialiased).
    Frames are (255 v - mean) / std.  A frame smaller than 224 x 224 is refused.
  aesthetic network: Conv3d (2,4,4) stride (2,4,4) stem with a channel LayerNorm, widths 96-192-384-768, depths [3,3,9,3]; a block is a
    depthwise (3,7,7) conv, LayerNorm (eps 1e-6), Linear to 4 C, exact-erf GELU, Linear to C, the layer scale gamma, the residual; between
    stages a LayerNorm and a (1,2,2) stride-(1,2,2) conv; a final LayerNorm per position; head fc_hid 768 -> 64, GELU, fc_last 64 -> 1, the
    mean over all positions, in fp64.
  fusion: t = (technical_raw - 0.1107) / 0.07355, a = (aesthetic_raw + 0.08285) / 0.03774; the scores are the sigmoids of t, a and
    0.6104 t + 0.3896 a.

Random draws come from ``numpy.random.Generator(PCG64(seed))`` in the order ``sample_draws`` documents.  The user supplies the checkpoint.
This module walks the network in Python; every operator is a kernel."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import fastvqa, ops
from .fastvqa import MEAN, PATCH, STD, VqaConfig, VqaWeights
from .iqa import ACTIVATION_BUDGET, for_groups, load_state_dict
from .netweights import Weights, checked, fan_in_normal, pack_linear_weight, random_tensors, strip

LN_EPS = 1e-6
TECH_PREFIX, TECH_HEAD, AES_PREFIX, AES_HEAD = "technical_backbone.", "technical_head.", "aesthetic_backbone.", "aesthetic_head."
# ((mean, std) of the technical branch, (mean, std) of the aesthetic branch) and the weights of the fused score, from memory
RESCALE = ((0.1107, 0.07355), (-0.08285, 0.03774))
FUSION = (0.6104, 0.3896)
# Live fp32 activations per stem token of the aesthetic branch, in units of the width: the map, the depthwise conv's output, its normalised
# copy and the MLP's hidden rows (4)
TOKEN_WIDTHS = 7
COUNTERS = {"groups": 0}
KEYS = ("technical_raw", "aesthetic_raw", "technical", "aesthetic", "overall")


@dataclass(frozen=True)
class DoverConfig:
    """The aesthetic branch."""
    size: tuple = (224, 224)
    clip_len: int = 32
    frame_interval: int = 2
    t_frag: int = 32
    num_clips: int = 1
    width: int = 96
    depths: tuple = (3, 3, 9, 3)
    head_hidden: int = 64
    resize: str = "antialias"          # or "plain": torch's bilinear without the antialiasing filter

    def __post_init__(self):
        if self.resize not in ("antialias", "plain"):
            raise ValueError(f"DoverConfig: resize {self.resize!r}: choose antialias or plain")
        down = 2 ** (len(self.depths) - 1)
        if self.clip_len % self.t_frag or self.clip_len % PATCH[0] or self.width % 32 or \
                any(s % PATCH[1] or (s // PATCH[1]) % down for s in self.size):
            raise ValueError("DoverConfig: clip_len must split into t_frag cells and patches of 2 frames, width % 32 == 0, and the view into "
                             "4 x 4 patches whose map halves evenly at every stage")

    @property
    def dims(self):
        return tuple(self.width * 2 ** i for i in range(len(self.depths)))


DEFAULT = DoverConfig()
# DOVER's technical branch: FAST-VQA's network under another sampler (``sample_plan`` below; fastvqa's own is not used)
TECHNICAL = VqaConfig(name="DOVER-technical", fragments=(7, 7), fsize=(32, 32), clip_len=32, frame_interval=2, t_groups=1, num_clips=3,
                      window=(8, 7, 7), rescale=RESCALE[0])


# ------------------------------------------------------------------ sampling ------------------------------------------------------------------
def _check_frame(H: int, W: int, cfg: DoverConfig, tech: VqaConfig):
    if H < cfg.size[0] or W < cfg.size[1]:
        raise ValueError(f"DOVER: frames of {H} x {W} are smaller than the {cfg.size[0]} x {cfg.size[1]} aesthetic view; upsampling a clip is "
                         f"not built")
    if H < tech.canvas[0] or W < tech.canvas[1]:
        raise ValueError(f"DOVER: frames of {H} x {W} are smaller than the {tech.canvas[0]} x {tech.canvas[1]} fragment canvas of the technical "
                         f"branch; upsampling a clip is not built")


def _cell_span(num_frames: int, clip_len: int, t_frag: int, interval: int) -> int:
    """The number of admissible starts inside one temporal cell; <= 0: the start is 0."""
    return num_frames // t_frag - clip_len // t_frag * interval


def sample_draws(num_frames: int, H: int, W: int, cfg: DoverConfig, tech: VqaConfig, seed: int) -> dict:
    """The random integers of a plan from ``numpy.random.Generator(PCG64(seed))``, in this order: per technical clip ``t`` (one start in
    [0, F - clip_len * interval)), ``h`` [gh,gw,1] in [0, H // gh - fh), ``w`` likewise; then per aesthetic clip ``t`` (t_frag starts in
    [0, F // t_frag - clip_len // t_frag * interval)).  A range that is empty draws nothing and gives zeros."""
    _check_frame(H, W, cfg, tech)
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    (gh, gw), (fh, fw) = tech.fragments, tech.fsize
    out = {"technical": [], "aesthetic": []}
    span = _cell_span(num_frames, tech.clip_len, tech.t_groups, tech.frame_interval)
    for _ in range(tech.num_clips):
        d = {"t": rng.integers(0, span, size=tech.t_groups) if span > 0 else np.zeros(tech.t_groups, dtype=np.int64)}
        for key, s in (("h", H // gh - fh), ("w", W // gw - fw)):
            d[key] = rng.integers(0, s, size=(gh, gw, tech.t_groups)) if s > 0 else np.zeros((gh, gw, tech.t_groups), dtype=np.int64)
        out["technical"].append(d)
    span = _cell_span(num_frames, cfg.clip_len, cfg.t_frag, cfg.frame_interval)
    for _ in range(cfg.num_clips):
        out["aesthetic"].append({"t": rng.integers(0, span, size=cfg.t_frag) if span > 0 else np.zeros(cfg.t_frag, dtype=np.int64)})
    return out


def _unified_frames(num_frames: int, clip_len: int, t_frag: int, interval: int, starts) -> np.ndarray:
    cells = num_frames // t_frag * np.arange(t_frag)
    idx = (cells + np.asarray(starts))[:, None] + interval * np.arange(clip_len // t_frag)[None, :]
    return (idx.reshape(-1) % num_frames).astype(np.int32)


def sample_plan(num_frames: int, H: int, W: int, cfg: DoverConfig | None = None, tech: VqaConfig | None = None, seed: int = 42,
                draws: dict | None = None) -> dict:
    """{"technical": (frame indices int32 [clips,clip_len], fragment origins int32 [clips,gh,gw,t_groups,2]), "aesthetic": frame indices
    int32 [clips,clip_len]} of a clip of ``num_frames`` H x W frames: the ``plan=`` of ``score_clip``; the technical pair is a plan of
    ``fastvqa.score_clip``."""
    cfg, tech = cfg or DEFAULT, tech or TECHNICAL
    if num_frames < 1:
        raise ValueError("a clip needs at least one frame")
    _check_frame(H, W, cfg, tech)
    if draws is None:
        draws = sample_draws(num_frames, H, W, cfg, tech, seed)
    (gh, gw), (fh, fw), tg = tech.fragments, tech.fsize, tech.t_groups
    oy = np.minimum(H // gh * np.arange(gh), H - fh)[:, None, None]
    ox = np.minimum(W // gw * np.arange(gw), W - fw)[None, :, None]
    frames = np.zeros((tech.num_clips, tech.clip_len), dtype=np.int32)
    origins = np.zeros((tech.num_clips, gh, gw, tg, 2), dtype=np.int64)
    for c, d in enumerate(draws["technical"]):
        frames[c] = _unified_frames(num_frames, tech.clip_len, tg, tech.frame_interval, d["t"])
        origins[c, ..., 0] = oy + np.asarray(d["h"])
        origins[c, ..., 1] = ox + np.asarray(d["w"])
    assert origins.min() >= 0 and (origins[..., 0] + fh).max() <= H and (origins[..., 1] + fw).max() <= W
    view = np.stack([_unified_frames(num_frames, cfg.clip_len, cfg.t_frag, cfg.frame_interval, d["t"]) for d in draws["aesthetic"]])
    return {"technical": (frames, origins.astype(np.int32)), "aesthetic": view}


# ------------------------------------------------------------------- weights -------------------------------------------------------------------
def aesthetic_shapes(cfg: DoverConfig) -> dict:
    s = {}
    b, dims = AES_PREFIX, cfg.dims
    s[b + "downsample_layers.0.0.weight"], s[b + "downsample_layers.0.0.bias"] = (cfg.width, 3) + PATCH, (cfg.width,)
    s[b + "downsample_layers.0.1.weight"], s[b + "downsample_layers.0.1.bias"] = (cfg.width,), (cfg.width,)
    for i in range(1, len(dims)):
        s[f"{b}downsample_layers.{i}.0.weight"], s[f"{b}downsample_layers.{i}.0.bias"] = (dims[i - 1],), (dims[i - 1],)
        s[f"{b}downsample_layers.{i}.1.weight"], s[f"{b}downsample_layers.{i}.1.bias"] = (dims[i], dims[i - 1], 1, 2, 2), (dims[i],)
    for i, (depth, C) in enumerate(zip(cfg.depths, dims)):
        for j in range(depth):
            p = f"{b}stages.{i}.{j}"
            s[p + ".dwconv.weight"], s[p + ".dwconv.bias"] = (C, 1, 3, 7, 7), (C,)
            s[p + ".norm.weight"], s[p + ".norm.bias"] = (C,), (C,)
            s[p + ".pwconv1.weight"], s[p + ".pwconv1.bias"] = (4 * C, C), (4 * C,)
            s[p + ".pwconv2.weight"], s[p + ".pwconv2.bias"] = (C, 4 * C), (C,)
            s[p + ".gamma"] = (C,)
    s[b + "norm.weight"], s[b + "norm.bias"] = (dims[-1],), (dims[-1],)
    s[AES_HEAD + "fc_hid.weight"], s[AES_HEAD + "fc_hid.bias"] = (cfg.head_hidden, dims[-1], 1, 1, 1), (cfg.head_hidden,)
    s[AES_HEAD + "fc_last.weight"], s[AES_HEAD + "fc_last.bias"] = (1, cfg.head_hidden, 1, 1, 1), (1,)
    return s


def _technical_name(name: str) -> str:
    """fastvqa's name of a technical entry -> the published one."""
    if name.startswith(fastvqa.PREFIX):
        return TECH_PREFIX + name[len(fastvqa.PREFIX):]
    return TECH_HEAD + name[len("vqa_head."):]


def param_shapes(cfg: DoverConfig | None = None, tech: VqaConfig | None = None) -> dict:
    """name -> shape of the entries of the published state dict that the two networks read (names from memory: INTEGRATION.md 1n)."""
    s = {_technical_name(k): v for k, v in fastvqa.param_shapes(tech or TECHNICAL).items()}
    s.update(aesthetic_shapes(cfg or DEFAULT))
    return s


def random_state(cfg: DoverConfig | None = None, seed: int = 0, tech: VqaConfig | None = None) -> dict:
    """Rule-generated state dict for tests and tools.  Technical: ``fastvqa.random_state`` under the published names.  Aesthetic: matrices
    and conv kernels normal with std 1 / sqrt(fan-in), norm weights and ``gamma`` uniform in [0.5, 1.5] (the published initialisation of
    gamma, 1e-6, would leave every block an identity to fp32), biases 0.05 * normal."""
    def rule(name, shape, rng):
        if len(shape) >= 2:
            return fan_in_normal(rng, shape)
        return rng.uniform(0.5, 1.5, shape) if name.endswith((".weight", ".gamma")) else 0.05 * rng.standard_normal(shape)

    sd = {_technical_name(k): v for k, v in fastvqa.random_state(tech or TECHNICAL, seed).items()}
    sd.update(random_tensors(aesthetic_shapes(cfg or DEFAULT), seed, lambda name: f"dover.{name}", rule))
    return sd


def pack_dwconv_weight(w: torch.Tensor) -> torch.Tensor:
    """[C,1,3,7,7] -> the kernel's tap-major [3,7,7,C] float32."""
    return w.detach().float()[:, 0].permute(1, 2, 3, 0).contiguous()


def pack_downsample_weight(w: torch.Tensor) -> torch.Tensor:
    """[C',C,1,2,2] -> [1,1,4 C,C'] float32 with the rows in ``swin3d_patch_merge_f32``'s block order (0,0), (1,0), (0,1), (1,1): block
    j = kh + 2 kw."""
    Co, Ci = w.shape[:2]
    return w.detach().float()[:, :, 0].permute(3, 2, 1, 0).reshape(4 * Ci, Co).contiguous()[None, None]


@dataclass
class DoverWeights(Weights):
    """``params``: the aesthetic tensors by their published names without the backbone prefix, packed for the kernels (gamma folded into
    pwconv2); ``tech``: the technical tensors as ``VqaWeights.params`` holds them."""
    cfg: DoverConfig = field(default_factory=DoverConfig)
    tech_cfg: VqaConfig = TECHNICAL
    params: dict = field(default_factory=dict)
    tech: dict = field(default_factory=dict)

    @classmethod
    def from_state_dict(cls, sd: dict, cfg: DoverConfig | None = None, tech: VqaConfig | None = None) -> "DoverWeights":
        cfg, tech = cfg or DEFAULT, tech or TECHNICAL
        sd = checked(strip(sd), param_shapes(cfg, tech), "DOVER checkpoint")
        technical = VqaWeights.from_state_dict({k: sd[_technical_name(k)] for k in fastvqa.param_shapes(tech)}, tech)
        f32 = lambda t: t.detach().float().contiguous()
        p = {}
        for name in aesthetic_shapes(cfg):
            t = sd[name]
            short = name[len(AES_PREFIX):] if name.startswith(AES_PREFIX) else name
            if short.endswith(".gamma"):
                continue
            if short.endswith(".dwconv.weight"):
                p[short] = pack_dwconv_weight(t)
            elif short.endswith(".pwconv2.weight"):                       # gamma (x W^T + b) = x (gamma W)^T + gamma b
                p[short] = pack_linear_weight(f32(t) * f32(sd[name[:-len("pwconv2.weight")] + "gamma"])[:, None])
            elif short.endswith(".pwconv2.bias"):
                p[short] = f32(t) * f32(sd[name[:-len("pwconv2.bias")] + "gamma"])
            elif t.dim() == 5 and short.startswith("downsample_layers.") and not short.startswith("downsample_layers.0."):
                p[short] = pack_downsample_weight(t)
            elif short == AES_HEAD + "fc_hid.weight":
                p[short] = f32(t.flatten(1))
            elif short == AES_HEAD + "fc_last.weight":
                p[short] = f32(t.flatten())
            else:
                p[short] = pack_linear_weight(t) if t.dim() >= 2 else f32(t)
        return cls(cfg=cfg, tech_cfg=tech, params=p, tech=technical.params)

    @classmethod
    def load(cls, path: str, cfg: DoverConfig | None = None, tech: VqaConfig | None = None) -> "DoverWeights":
        """From a checkpoint file in the published layout (a top-level ``state_dict`` is unwrapped)."""
        return cls.from_state_dict(load_state_dict(path), cfg, tech)

    def technical(self) -> VqaWeights:
        """The technical branch as ``fastvqa``'s functions take it, on this object's device (no copy)."""
        return VqaWeights(device=self.device, cfg=self.tech_cfg, params=self.tech)


# -------------------------------------------------------------------- walk --------------------------------------------------------------------
def _ln(W, name, rows, out=None):
    return ops.layernorm_f32(rows, W.params[name + ".weight"], W.params[name + ".bias"], LN_EPS, out=out)


def embed(W: DoverWeights, frames: torch.Tensor, frame_idx: torch.Tensor) -> torch.Tensor:
    """One clip's resized view through the stem (the im2col gather, one k-ordered fp32 FMA chain of 96 terms per output, the channel
    LayerNorm) -> float32 [1,T/2,oh/4,ow/4,width]."""
    cols = ops.vqa_resized_view_f32(frames, frame_idx, W.cfg.size, MEAN, STD, antialias=W.cfg.resize == "antialias", cols=True)
    x = ops.linear_f32(cols.view(-1, cols.shape[-1]), W.params["downsample_layers.0.0.weight"], W.params["downsample_layers.0.0.bias"])
    return _ln(W, "downsample_layers.0.1", x).view(1, *cols.shape[:3], W.cfg.width)


def block(W: DoverWeights, x: torch.Tensor, p: str) -> torch.Tensor:
    """One ConvNeXt block on the map float32 [B,D,H,W,C], changed in place."""
    P, C = W.params, x.shape[-1]
    h = ops.dwconv3d_f32(x, P[p + ".dwconv.weight"], P[p + ".dwconv.bias"])
    n = _ln(W, p + ".norm", h.view(-1, C))
    del h
    m = ops.linear_f32(n, P[p + ".pwconv1.weight"], P[p + ".pwconv1.bias"])
    del n
    ops.gelu_f32(m, out=m)
    rows = x.view(-1, C)
    ops.linear_f32(m, P[p + ".pwconv2.weight"], P[p + ".pwconv2.bias"], residual=rows, out=rows)
    return x


def downsample(W: DoverWeights, x: torch.Tensor, p: str) -> torch.Tensor:
    """LayerNorm per position, then the (1,2,2) stride-(1,2,2) conv as a 2 x 2 gather and one GEMM -> [B,D,H/2,W/2,C']."""
    B, D, H, Wd, C = x.shape
    if H % 2 or Wd % 2:
        raise ValueError(f"DOVER: a {H} x {Wd} map cannot be halved by the stride-2 conv (H and W must be even)")
    g = ops.swin3d_patch_merge_f32(_ln(W, p + ".0", x.view(-1, C)).view(x.shape))
    w = W.params[p + ".1.weight"]
    return ops.linear_f32(g.view(-1, 4 * C), w, W.params[p + ".1.bias"]).view(B, D, H // 2, Wd // 2, w.shape[-1])


def backbone(W: DoverWeights, x: torch.Tensor, stages: int | None = None, first: int = 0) -> torch.Tensor:
    """Stem map [B,D,H,W,width] (changed in place) -> the final-normed map [B,D,H/8,W/8,8 width].  ``stages`` = s stops after the blocks of
    stage s - 1 and returns that map; ``first``: x is the input of the blocks of this stage (for tests)."""
    n = len(W.cfg.depths)
    for i in range(first, n if stages is None else stages):
        if i > first:
            x = downsample(W, x, f"downsample_layers.{i}")
        for j in range(W.cfg.depths[i]):
            x = block(W, x, f"stages.{i}.{j}")
    if stages is not None:
        return x
    return _ln(W, "norm", x.view(-1, x.shape[-1])).view(x.shape)


def head(W: DoverWeights, feat: torch.Tensor) -> torch.Tensor:
    """Final map [B,D,H,W,C] -> float64 [B]."""
    P = W.params
    return ops.vqa_head_f64(feat.view(feat.shape[0], -1, feat.shape[-1]), P[AES_HEAD + "fc_hid.weight"], P[AES_HEAD + "fc_hid.bias"],
                            P[AES_HEAD + "fc_last.weight"], P[AES_HEAD + "fc_last.bias"])


def group_size(cfg: DoverConfig, budget: int | None = None) -> int:
    """Aesthetic clips per group: the most whose live activations (``TOKEN_WIDTHS`` widths per stem token) stay under the budget."""
    tokens = cfg.clip_len // PATCH[0] * (cfg.size[0] // PATCH[1]) * (cfg.size[1] // PATCH[2])
    return max(1, int((ACTIVATION_BUDGET if budget is None else budget) // (4 * TOKEN_WIDTHS * cfg.width * tokens)))


def aesthetic_raw(W: DoverWeights, x: torch.Tensor, idx: np.ndarray, group: int | None = None) -> float:
    """The mean over the clips of ``idx`` [clips,clip_len] of the aesthetic head's output; ``x`` an [F,3,H,W] view and ``W`` on its device."""
    raw = torch.empty(len(idx), dtype=torch.float64, device=x.device)

    def per_group(i, j):
        maps = [embed(W, x, torch.from_numpy(np.ascontiguousarray(idx[c])).to(x.device)) for c in range(i, j)]
        raw[i:j] = head(W, backbone(W, torch.cat(maps) if len(maps) > 1 else maps[0]))

    for_groups(len(idx), group, group_size(W.cfg), COUNTERS, x.device, per_group)
    s = 0.0
    for v in raw.cpu().tolist():                     # clip order
        s += v
    return s / len(idx)


def fuse(technical_raw: float, aesthetic: float, rescale=None) -> dict:
    """The five values of ``score_clip`` from the two raw ones; ``rescale`` = ((technical mean, std), (aesthetic mean, std))."""
    (tm, ts), (am, as_) = RESCALE if rescale is None else rescale
    t, a = (technical_raw - tm) / ts, (aesthetic - am) / as_
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))
    return {"technical_raw": technical_raw, "aesthetic_raw": aesthetic, "technical": sig(t), "aesthetic": sig(a),
            "overall": sig(FUSION[0] * t + FUSION[1] * a)}


def with_rescale(technical_mean=None, technical_std=None, aesthetic_mean=None, aesthetic_std=None) -> tuple:
    pick = lambda v, d: d if v is None else float(v)
    return ((pick(technical_mean, RESCALE[0][0]), pick(technical_std, RESCALE[0][1])),
            (pick(aesthetic_mean, RESCALE[1][0]), pick(aesthetic_std, RESCALE[1][1])))


def score_clip(frames: torch.Tensor, weights: DoverWeights, seed: int = 42, plan: dict | None = None, group: int | None = None,
               rescale=None) -> dict:
    """DOVER's values of one video, Python floats (fp64): ``technical_raw`` (the mean over the technical clips), ``aesthetic_raw``,
    and ``technical``, ``aesthetic``, ``overall`` in (0, 1) (``fuse``).  ``frames``: uint8 [F,H,W,3] or [F,3,H,W] in [0,1], host or
    device.  ``plan``: a ``sample_plan`` result (default: drawn from ``seed``).  ``group``: clips per batch of either branch (default:
    from the budget); the values do not depend on it."""
    if not isinstance(weights, DoverWeights):
        raise TypeError(f"score_clip: weights must be DoverWeights, got {type(weights).__name__}")
    x = fastvqa.clip_view(frames, "dover")
    cfg, tech = weights.cfg, weights.tech_cfg
    _check_frame(x.shape[2], x.shape[3], cfg, tech)
    if plan is None:
        plan = sample_plan(x.shape[0], x.shape[2], x.shape[3], cfg, tech, seed)
    W = weights.to(x.device)
    technical_raw, _ = fastvqa.score_clip(x, W.technical(), plan=plan["technical"], group=group)
    return fuse(technical_raw, aesthetic_raw(W, x, plan["aesthetic"], group), rescale)
