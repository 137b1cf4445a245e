"""DOVER in plain torch, in the shape of the original computation (restated from memory of the DOVER repository's ``dover/datasets``
- UnifiedFrameSampler, the resized "aesthetic" view - and ``dover/models`` - conv_backbone.py's inflated ConvNeXt-Tiny, head.py, and the
fusion of evaluate_one_video.py; neither the sources nor a checkpoint were at hand): F.interpolate on the float frames, F.conv3d with
groups = C, F.layer_norm, F.gelu, gamma applied after pwconv2 (not folded).  ``dtype`` switches every tensor between float32 and float64.
Shares no code with dove_amd/dover.py; the technical backbone is tests/fastvqa_ref.py's.  Configurations are plain dicts with the field
names of ``dove_amd.dover.DoverConfig`` and ``dove_amd.fastvqa.VqaConfig``.  This file is the definition that the kernels are pinned to;
agreement with the published ``DOVER.pth`` is unchecked.

The depthwise kernel's summation order, written here because fp32 sums depend on it: every output is one fmaf chain that starts from the
bias and takes the 147 taps in (kd, kh, kw) order, kd outermost, each ascending; taps outside the map are skipped (or multiply a zero).
F.conv3d sums in an order of its own, so the two agree to rounding, not bit for bit (``dwconv_chain`` below restates the chain exactly).

Settled from memory, each a doubt:
  * Whether the aesthetic view is antialiased.  The original resizes with torchvision's ``Resize`` on a tensor; current torchvision
    antialiases tensors, releases before 0.17 did not.  Chosen: antialiased bilinear; ``resize = "plain"`` is the other reading.
  * The original resizes uint8 frames and gets uint8 back (torch's fixed-point uint8 path, rounded to 8 bits) before normalising.  Here
    the frames are resized as floating point and nothing is rounded to 8 bits.
  * LayerNorm eps 1e-6 in every ConvNeXt norm (the technical branch keeps Swin's 1e-5).
  * The final LayerNorm is applied per position of the last map, before the head (the classification ConvNeXt norms the pooled vector;
    the original's unpooled path may skip the norm altogether).
  * The key names: ``technical_backbone.*`` / ``technical_head.*`` (FAST-VQA's names under another prefix) and ``aesthetic_backbone.
    {downsample_layers, stages, norm}`` / ``aesthetic_head.{fc_hid, fc_last}``.
  * The fusion constants (0.1107, 0.07355) and (-0.08285, 0.03774), the weights 0.6104 / 0.3896, and which branch each belongs to.
  * The temporal starts are random inside each cell also at test time (UnifiedFrameSampler draws whenever the cell is longer than the
    span); the technical branch takes 3 clips with one random start each, not FAST-VQA's evenly spaced starts.
  * u8 frames are normalised as (u - mean) / std, float frames in [0,1] as (255 v - mean) / std."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import fastvqa_ref as R

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
LN_EPS = 1e-6
RESCALE = ((0.1107, 0.07355), (-0.08285, 0.03774))
FUSION = (0.6104, 0.3896)
A, AH, TB, TH = "aesthetic_backbone.", "aesthetic_head.", "technical_backbone.", "technical_head."


# ------------------------------------------------------------------ sampling ------------------------------------------------------------------
def unified_frame_indices(num_frames, fsize_t, fragments_t, interval, rnd):
    """UnifiedFrameSampler.get_frame_indices with the random starts ``rnd`` supplied (used only where the original draws)."""
    tgrids = np.array([num_frames // fragments_t * i for i in range(fragments_t)], dtype=np.int64)
    tlength = num_frames // fragments_t
    rnd_t = np.asarray(rnd, dtype=np.int64) if tlength > fsize_t * interval else np.zeros(len(tgrids), dtype=np.int64)
    ranges_t = np.arange(fsize_t)[None, :] * interval + rnd_t[:, None] + tgrids[:, None]
    return np.mod(np.concatenate(ranges_t), num_frames).astype(np.int32)


def plan_from_draws(num_frames, H, W, acfg, tcfg, draws):
    """{"technical": (frames [clips][clip_len], origins [clips][gh][gw][1][2]), "aesthetic": frames [clips][clip_len]}."""
    tg = tcfg["t_groups"]
    tech = np.stack([unified_frame_indices(num_frames, tcfg["clip_len"] // tg, tg, tcfg["frame_interval"], d["t"]) for d in draws["technical"]])
    aes = np.stack([unified_frame_indices(num_frames, acfg["clip_len"] // acfg["t_frag"], acfg["t_frag"], acfg["frame_interval"], d["t"])
                    for d in draws["aesthetic"]])
    return {"technical": (tech, R.fragment_origins(H, W, tcfg, draws["technical"])), "aesthetic": aes}


def resized_view(frames, frame_idx, size, antialias, dtype):
    """frames: uint8 [F,H,W,3] or floating [F,3,H,W] in [0,1] -> [T,oh,ow,3] in ``dtype``: F.interpolate (bilinear, align_corners False)
    of X = u or 255 v, then (X - mean) / std."""
    x = frames.permute(0, 3, 1, 2).to(dtype) if frames.dtype == torch.uint8 else 255.0 * frames.to(dtype)
    x = x[torch.as_tensor(np.asarray(frame_idx), dtype=torch.long)]
    x = F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False, antialias=bool(antialias)).permute(0, 2, 3, 1)
    return (x - torch.tensor(MEAN, dtype=dtype)) / torch.tensor(STD, dtype=dtype)


# ------------------------------------------------------------------- network -------------------------------------------------------------------
def _ln(x, sd, name, dtype):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype), LN_EPS)


def _cl(x):
    return x.permute(0, 2, 3, 4, 1)


def _cf(x):
    return x.permute(0, 4, 1, 2, 3)


def dwconv(x, w, b, dtype):
    """x channels-last [B,D,H,W,C], w [C,1,3,7,7], b [C]."""
    return _cl(F.conv3d(_cf(x.to(dtype)), w.to(dtype), b.to(dtype), padding=(1, 3, 3), groups=x.shape[-1]))


def dwconv_chain(x, w, b):
    """The kernel's own fp32 sum, bit for bit: float32 fma chain from the bias over (kd, kh, kw), emulated in fp64 (a product of two
    float32 is exact in fp64 and the sum of it with a float32 rounds to float32 as the fused operation does, but for double rounding in
    rare ties; used on small maps only, as an aid)."""
    B, D, H, W, C = x.shape
    p = F.pad(x.double(), (0, 0, 3, 3, 3, 3, 1, 1))
    acc = b.float().double().expand(B, D, H, W, C).clone()
    for kd in range(3):
        for kh in range(7):
            for kw in range(7):
                acc = (acc + p[:, kd:kd + D, kh:kh + H, kw:kw + W] * w[:, 0, kd, kh, kw].double()).float().double()
    return acc.float()


def stem(view, sd, dtype):
    """view [B,T,oh,ow,3] -> [B,T/2,oh/4,ow/4,width]."""
    x = F.conv3d(_cf(view.to(dtype)), sd[A + "downsample_layers.0.0.weight"].to(dtype), sd[A + "downsample_layers.0.0.bias"].to(dtype),
                 stride=(2, 4, 4))
    return _ln(_cl(x), sd, A + "downsample_layers.0.1", dtype)


def block(x, sd, p, dtype):
    h = dwconv(x, sd[p + ".dwconv.weight"], sd[p + ".dwconv.bias"], dtype)
    h = _ln(h, sd, p + ".norm", dtype)
    h = F.linear(h, sd[p + ".pwconv1.weight"].to(dtype), sd[p + ".pwconv1.bias"].to(dtype))
    h = F.gelu(h)
    h = F.linear(h, sd[p + ".pwconv2.weight"].to(dtype), sd[p + ".pwconv2.bias"].to(dtype))
    return x + sd[p + ".gamma"].to(dtype) * h


def downsample(x, sd, i, dtype):
    h = _ln(x, sd, f"{A}downsample_layers.{i}.0", dtype)
    return _cl(F.conv3d(_cf(h), sd[f"{A}downsample_layers.{i}.1.weight"].to(dtype), sd[f"{A}downsample_layers.{i}.1.bias"].to(dtype),
                        stride=(1, 2, 2)))


def stage(x, sd, i, depth, dtype):
    """The blocks of stage ``i`` on a channels-last map."""
    x = x.to(dtype)
    for j in range(depth):
        x = block(x, sd, f"{A}stages.{i}.{j}", dtype)
    return x


def backbone(x, sd, cfg, dtype, stages=None):
    """Stem map -> the final-normed map; ``stages`` = s: stop after the blocks of stage s - 1."""
    n = len(cfg["depths"])
    for i in range(n if stages is None else stages):
        if i > 0:
            x = downsample(x, sd, i, dtype)
        x = stage(x, sd, i, cfg["depths"][i], dtype)
    return x if stages is not None else _ln(x, sd, A + "norm", dtype)


def head(feat, sd, dtype, prefix=AH):
    """feat [B, tokens, C] -> [B]"""
    w1 = sd[prefix + "fc_hid.weight"].to(dtype).flatten(1)
    w2 = sd[prefix + "fc_last.weight"].to(dtype).flatten(1)
    h = F.gelu(F.linear(feat, w1, sd[prefix + "fc_hid.bias"].to(dtype)))
    return F.linear(h, w2, sd[prefix + "fc_last.bias"].to(dtype)).mean(dim=(1, 2))


def technical_state(sd):
    """The technical entries under FAST-VQA's names, for fastvqa_ref."""
    out = {}
    for k, v in sd.items():
        if k.startswith(TB):
            out[R.PREFIX + k[len(TB):]] = v
        elif k.startswith(TH):
            out["vqa_head." + k[len(TH):]] = v
    return out


def aesthetic_raw(sd, frames, acfg, idx, dtype):
    view = torch.stack([resized_view(frames, idx[c], acfg["size"], acfg["resize"] == "antialias", torch.float64).float() for c in range(len(idx))])
    feat = backbone(stem(view, sd, dtype), sd, acfg, dtype)
    return head(feat.flatten(1, 3), sd, dtype).mean()


def fuse(technical_raw, aesthetic, rescale=RESCALE):
    (tm, ts), (am, as_) = rescale
    t, a = (technical_raw - tm) / ts, (aesthetic - am) / as_
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))
    return {"technical_raw": technical_raw, "aesthetic_raw": aesthetic, "technical": sig(t), "aesthetic": sig(a),
            "overall": sig(FUSION[0] * t + FUSION[1] * a)}


def score(sd, frames, acfg, tcfg, plan, dtype, rescale=RESCALE):
    """Every value of the metric in ``dtype`` (the fusion itself in Python floats)."""
    t = float(R.raw_score(technical_state(sd), frames, tcfg, plan["technical"], dtype))
    return fuse(t, float(aesthetic_raw(sd, frames, acfg, plan["aesthetic"], dtype)), rescale)
