"""FasterVQA / FAST-VQA in plain torch, in the shape of the original computation (restated from memory of the FAST-VQA repository's
``fastvqa/datasets/fusion_datasets.py`` - get_spatial_fragments, FragmentSampleFrames, SampleFrames - and ``fastvqa/models/swin_backbone.py``
/ ``head.py``; neither the sources nor a checkpoint were at hand): F.pad, torch.roll, window_partition / window_reverse by view + permute,
a full score matrix with an added bias and an added -100 mask, nn.functional.layer_norm, F.interpolate for the fragment grid.  ``dtype``
switches every tensor between float32 and float64.  Shares no code with dove_amd/fastvqa.py; a configuration is a plain dict with the
field names of ``dove_amd.fastvqa.VqaConfig``.  This file is the definition that the kernels are pinned to; agreement with the published
model on real weights is unchecked.

Settled from memory, each a doubt:
  * Gated relative position bias.  Remembered: stages 0-2 carry ``fragment_position_bias_table`` beside ``relative_position_bias_table``
    and a per-pair gate mixes them.  Chosen here: a HARD gate - the ordinary table for a token pair inside one fragment, the second table
    for a pair from different fragments (bias = where(frag_q != frag_k, table_b, table_a)).  The original may instead mix the two
    with a soft or differently signed gate; the kernel takes two tables and a per-token fragment id, so swapping the tables or feeding
    pre-mixed tables is a host-side change.
  * Fragment ids: the gh x gw fragment grid (one fragment along time), nearest-interpolated onto the PADDED map (F.interpolate, mode
    'nearest'), rolled by -shift, window-partitioned.  The original may interpolate onto the unpadded map.
  * The relative position index is built for the configured window and cut to [:N, :N] where an axis clamps the window (Video Swin does
    this; it is not the geometric index of the smaller window).
  * The mask is computed on the padded map with Video Swin's three slices per axis and the value -100.
  * LayerNorm eps 1e-5; patch merging pads odd H / W with zeros and concatenates (0,0), (1,0), (0,1), (1,1); the head is fc_hid, exact-erf
    GELU, fc_last (dropout is identity at inference), then the mean over all tokens.
  * Sampling: see ``plan_from_draws``.  The original upsamples a frame smaller than the canvas; not restated.
  * u8 frames are normalised as (u - mean) / std, float frames in [0,1] as (255 v - mean) / std, in fp64, rounded once to fp32."""
import math

import numpy as np
import torch
import torch.nn.functional as F

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
MASK_VALUE = -100.0
LN_EPS = 1e-5
PREFIX = "fragments_backbone."


# ------------------------------------------------------------------ sampling ------------------------------------------------------------------
def frame_indices(num_frames, cfg, draws):
    """[num_clips][clip_len] frame indices, wrapped modulo the clip's length.  t_groups > 1: FragmentSampleFrames (t_groups grid cells of
    num_frames // t_groups frames, clip_len / t_groups frames at ``frame_interval`` from a random start inside each cell).  t_groups == 1:
    SampleFrames in test mode (num_clips evenly spaced starts, no randomness)."""
    L_, tg, iv = cfg["clip_len"], cfg["t_groups"], cfg["frame_interval"]
    out = []
    for c in range(cfg["num_clips"]):
        if tg > 1:
            fsize_t = L_ // tg
            tgrids = np.array([num_frames // tg * i for i in range(tg)])
            tlength = num_frames // tg
            rnd = np.asarray(draws[c]["t"]) if tlength > fsize_t * iv else np.zeros(tg, dtype=np.int64)
            idx = (np.arange(fsize_t)[None, :] * iv + rnd[:, None] + tgrids[:, None]).reshape(-1)
        else:
            ori = (L_ - 1) * iv + 1
            avg = (num_frames - ori + 1) / float(cfg["num_clips"])
            start = int(np.arange(cfg["num_clips"])[c] * avg + avg / 2.0) if num_frames > ori - 1 else 0
            idx = start + np.arange(L_) * iv
        out.append(np.mod(idx, num_frames))
    return np.stack(out).astype(np.int32)


def fragment_origins(H, W, cfg, draws):
    """[num_clips][gh][gw][t_groups][2]: the top-left source pixel of every fragment: grid origin H // gh * i clamped to H - fh, plus a
    uniform integer in [0, H // gh - fh) per (cell, temporal group) where that range is not empty."""
    (gh, gw), (fh, fw), tg = cfg["fragments"], cfg["fsize"], cfg["t_groups"]
    if H < gh * fh or W < gw * fw:
        raise ValueError("frame smaller than the fragment canvas")
    out = np.zeros((cfg["num_clips"], gh, gw, tg, 2), dtype=np.int32)
    hg = [min(H // gh * i, H - fh) for i in range(gh)]
    wg = [min(W // gw * j, W - fw) for j in range(gw)]
    for c in range(cfg["num_clips"]):
        rh = np.asarray(draws[c]["h"]) if H // gh > fh else np.zeros((gh, gw, tg), dtype=np.int64)
        rw = np.asarray(draws[c]["w"]) if W // gw > fw else np.zeros((gh, gw, tg), dtype=np.int64)
        for i in range(gh):
            for j in range(gw):
                for g in range(tg):
                    out[c, i, j, g] = (hg[i] + rh[i, j, g], wg[j] + rw[i, j, g])
    return out


def plan_from_draws(num_frames, H, W, cfg, draws):
    return frame_indices(num_frames, cfg, draws), fragment_origins(H, W, cfg, draws)


def fragments(frames, frame_idx, origins, cfg):
    """frames: uint8 [F,H,W,3] or floating [F,3,H,W] in [0,1]; frame_idx [T], origins [gh][gw][tg][2] of one clip -> float32 [T,gh fh,gw
    fw,3], evaluated in fp64 and rounded once."""
    (gh, gw), (fh, fw), tg = cfg["fragments"], cfg["fsize"], cfg["t_groups"]
    x = frames.double() if frames.dtype == torch.uint8 else 255.0 * frames.permute(0, 2, 3, 1).double()
    x = (x - torch.tensor(MEAN, dtype=torch.float64)) / torch.tensor(STD, dtype=torch.float64)
    T = len(frame_idx)
    out = torch.zeros(T, gh * fh, gw * fw, 3, dtype=torch.float64)
    for t in range(T):
        g = t // (T // tg)
        for i in range(gh):
            for j in range(gw):
                y0, x0 = int(origins[i][j][g][0]), int(origins[i][j][g][1])
                out[t, i * fh:(i + 1) * fh, j * fw:(j + 1) * fw] = x[int(frame_idx[t]), y0:y0 + fh, x0:x0 + fw]
    return out.float()


# ------------------------------------------------------------------ geometry ------------------------------------------------------------------
def window_partition(x, ws):
    B, D, H, W, C = x.shape
    x = x.view(B, D // ws[0], ws[0], H // ws[1], ws[1], W // ws[2], ws[2], C)
    return x.permute(0, 1, 3, 5, 2, 4, 6, 7).contiguous().view(-1, ws[0] * ws[1] * ws[2], C)


def window_reverse(windows, ws, B, D, H, W):
    x = windows.view(B, D // ws[0], H // ws[1], W // ws[2], ws[0], ws[1], ws[2], -1)
    return x.permute(0, 1, 4, 2, 5, 3, 6, 7).contiguous().view(B, D, H, W, -1)


def get_window_size(x_size, window_size, shift_size):
    ws, ss = list(window_size), list(shift_size)
    for i in range(3):
        if x_size[i] <= window_size[i]:
            ws[i], ss[i] = x_size[i], 0
    return tuple(ws), tuple(ss)


def padded_size(x_size, ws):
    return tuple(int(math.ceil(s / w)) * w for s, w in zip(x_size, ws))


def compute_mask(Dp, Hp, Wp, ws, ss):
    """[nW, N, N] float: 0 inside a shift region, -100 across (Video Swin's compute_mask)."""
    img = torch.zeros(1, Dp, Hp, Wp, 1)
    cnt = 0
    for d in (slice(-ws[0]), slice(-ws[0], -ss[0]), slice(-ss[0], None)):
        for h in (slice(-ws[1]), slice(-ws[1], -ss[1]), slice(-ss[1], None)):
            for w in (slice(-ws[2]), slice(-ws[2], -ss[2]), slice(-ss[2], None)):
                img[:, d, h, w, :] = cnt
                cnt += 1
    mw = window_partition(img, ws).squeeze(-1)
    m = mw[:, None, :] - mw[:, :, None]
    return m.masked_fill(m != 0, MASK_VALUE).masked_fill(m == 0, 0.0)


def relative_position_index(ws):
    coords = torch.stack(torch.meshgrid(torch.arange(ws[0]), torch.arange(ws[1]), torch.arange(ws[2]), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws[0] - 1
    rel[:, :, 1] += ws[1] - 1
    rel[:, :, 2] += ws[2] - 1
    rel[:, :, 0] *= (2 * ws[1] - 1) * (2 * ws[2] - 1)
    rel[:, :, 1] *= 2 * ws[2] - 1
    return rel.sum(-1)


def fragment_ids(Dp, Hp, Wp, grid, ws, ss):
    """[nW, N] long: the fragment (row * gw + column) of every window token of the padded, rolled map."""
    gh, gw = grid
    ids = (torch.arange(gh)[:, None] * gw + torch.arange(gw)[None, :]).float()[None, None, None]      # [1,1,1,gh,gw]
    m = F.interpolate(ids, size=(Dp, Hp, Wp), mode="nearest").long()[0, 0]
    m = torch.roll(m, shifts=(-ss[0], -ss[1], -ss[2]), dims=(0, 1, 2))
    return window_partition(m[None, ..., None], ws).squeeze(-1)


# ------------------------------------------------------------------- network -------------------------------------------------------------------
def _ln(x, sd, name, dtype):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype), LN_EPS)


def _lin(x, sd, name, dtype, bias=True):
    return F.linear(x, sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype) if bias else None)


def window_attention(xw, sd, p, heads, window, nW, mask, frag, dtype):
    """xw [B nW, N, C]; mask [nW,N,N] or None; frag [nW,N] or None."""
    B_, N, C = xw.shape
    qkv = _lin(xw, sd, p + ".qkv", dtype).reshape(B_, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * (C // heads) ** -0.5, qkv[1], qkv[2]
    attn = q @ k.transpose(-2, -1)                                                              # [B_, heads, N, N]
    idx = relative_position_index(window)[:N, :N].reshape(-1)
    bias = sd[p + ".relative_position_bias_table"].to(dtype)[idx].reshape(N, N, heads).permute(2, 0, 1)[None]
    if frag is not None and p + ".fragment_position_bias_table" in sd:
        bias_b = sd[p + ".fragment_position_bias_table"].to(dtype)[idx].reshape(N, N, heads).permute(2, 0, 1)[None]
        gate = (frag[:, :, None] != frag[:, None, :])[:, None]                                   # [nW,1,N,N]
        bias = torch.where(gate, bias_b, bias)                                                   # [nW,heads,N,N]
        attn = (attn.view(B_ // nW, nW, heads, N, N) + bias[None]).view(B_, heads, N, N)
    else:
        attn = attn + bias
    if mask is not None:
        attn = (attn.view(B_ // nW, nW, heads, N, N) + mask.to(dtype)[None, :, None]).view(B_, heads, N, N)
    attn = torch.softmax(attn, dim=-1)
    return _lin((attn @ v).transpose(1, 2).reshape(B_, N, C), sd, p + ".proj", dtype)


def block(x, sd, p, heads, window, shift, grid, dtype):
    B, D, H, W, C = x.shape
    ws, ss = get_window_size((D, H, W), window, shift)
    Dp, Hp, Wp = padded_size((D, H, W), ws)
    shortcut = x
    h = _ln(x, sd, p + ".norm1", dtype)
    h = F.pad(h, (0, 0, 0, Wp - W, 0, Hp - H, 0, Dp - D))
    shifted = any(s > 0 for s in ss)
    if shifted:
        h = torch.roll(h, shifts=(-ss[0], -ss[1], -ss[2]), dims=(1, 2, 3))
    mask = compute_mask(Dp, Hp, Wp, ws, ss) if shifted else None
    frag = fragment_ids(Dp, Hp, Wp, grid, ws, ss)
    xw = window_partition(h, ws)
    aw = window_attention(xw, sd, p + ".attn", heads, window, xw.shape[0] // B, mask, frag, dtype)
    h = window_reverse(aw, ws, B, Dp, Hp, Wp)
    if shifted:
        h = torch.roll(h, shifts=ss, dims=(1, 2, 3))
    x = shortcut + h[:, :D, :H, :W]
    m = _lin(F.gelu(_lin(_ln(x, sd, p + ".norm2", dtype), sd, p + ".mlp.fc1", dtype)), sd, p + ".mlp.fc2", dtype)
    return x + m


def patch_merge(x, sd, p, dtype):
    B, D, H, W, C = x.shape
    x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]], -1)
    return _lin(_ln(x, sd, p + ".norm", dtype), sd, p + ".reduction", dtype, bias=False)


def patch_embed(clip, sd, dtype):
    """clip [B,T,Hc,Wc,3] -> token map [B,T/2,Hc/4,Wc/4,width] (Conv3d (2,4,4) stride (2,4,4), then the patch norm)."""
    x = F.conv3d(clip.to(dtype).permute(0, 4, 1, 2, 3), sd[PREFIX + "patch_embed.proj.weight"].to(dtype),
                 sd[PREFIX + "patch_embed.proj.bias"].to(dtype), stride=(2, 4, 4)).permute(0, 2, 3, 4, 1)
    return _ln(x, sd, PREFIX + "patch_embed.norm", dtype)


def backbone(clip, sd, cfg, dtype, stages=None, blocks=None):
    """``stages`` = s: stop after the blocks of stage s - 1 (before its merge) and return that map; ``blocks``: at most this many blocks of a
    stage.  Default: the final-normed map [B,D,H,W,8 width]."""
    x = patch_embed(clip, sd, dtype)
    window = tuple(cfg["window"])
    n = len(cfg["depths"])
    for i in range(n if stages is None else stages):
        for j in range(cfg["depths"][i] if blocks is None else min(blocks, cfg["depths"][i])):
            shift = (0, 0, 0) if j % 2 == 0 else tuple(w // 2 for w in window)
            x = block(x, sd, f"{PREFIX}layers.{i}.blocks.{j}", cfg["heads"][i], window, shift, tuple(cfg["fragments"]), dtype)
        if stages is not None and i == stages - 1:
            return x
        if i < n - 1:
            x = patch_merge(x, sd, f"{PREFIX}layers.{i}.downsample", dtype)
    return _ln(x, sd, PREFIX + "norm", dtype)


def head(feat, sd, dtype):
    """feat [B, tokens, C] -> [B]"""
    w1 = sd["vqa_head.fc_hid.weight"].to(dtype).flatten(1)
    w2 = sd["vqa_head.fc_last.weight"].to(dtype).flatten(1)
    h = F.gelu(F.linear(feat, w1, sd["vqa_head.fc_hid.bias"].to(dtype)))
    return F.linear(h, w2, sd["vqa_head.fc_last.bias"].to(dtype)).mean(dim=(1, 2))


def raw_score(sd, frames, cfg, plan, dtype):
    """The mean over the plan's clips of the head's output, in ``dtype``."""
    idx, org = plan
    clips = torch.stack([fragments(frames, idx[c], org[c], cfg) for c in range(len(idx))])
    feat = backbone(clips, sd, cfg, dtype)
    return head(feat.flatten(1, 3), sd, dtype).mean()


def rescale(raw, mean, std):
    return 1.0 / (1.0 + math.exp(-(raw - mean) / std))
