"""MANIQA in plain torch, parameterised by dtype: the definition that dove_amd/maniqa.py and csrc/maniqa.hip are pinned to.

Restated from memory of pyiqa's ``maniqa_arch.py`` and IIGROUP/MANIQA (``maniqa.py``, ``swin.py``); neither pyiqa nor timm nor a checkpoint
were at hand, so agreement with the published model is unchecked.  It reads the state dict in the published layout
(``dove_amd.maniqa.param_shapes``) and a ``cfg`` dict (``dove_amd.maniqa.CFG``), and shares no code with the module under test.  ``dtype``
torch.float64 is the reference, torch.float32 its own fp32 run, whose deviation from the former is the yardstick of the GPU tests."""
import math

import torch
import torch.nn.functional as F


def crop_origins(H, W, side, crops):
    """pyiqa's uniform_crop: [(row, column)] of the first ``crops`` cells of a ceil(sqrt(crops))-square grid with floor steps."""
    lo, hi = int(math.sqrt(crops)), int(math.ceil(math.sqrt(crops)))
    sh, sw = (H - side) // lo, (W - side) // lo
    out = []
    for i in range(hi):
        for j in range(hi):
            out.append((i * sh, j * sw))
    return out[:crops]


def unit(img):
    """[N,C,H,W] uint8 or float images (or uint8 [N,H,W,3] frames) -> fp64 [N,3,H,W] in [0,1]."""
    if img.dtype == torch.uint8 and img.shape[3] in (1, 3) and img.shape[1] not in (1, 3):
        img = img.permute(0, 3, 1, 2)
    x = img.double() / 255.0 if img.dtype == torch.uint8 else img.double()
    return x.expand(-1, 3, -1, -1) if x.shape[1] == 1 else x


def crops(img, cfg, dtype):
    """The normalised crops [N crops,3,side,side]: (v - 0.5) / 0.5 in fp64, rounded once to ``dtype``."""
    x = (unit(img) - 0.5) / 0.5
    s = cfg["side"]
    cut = [x[:, :, r:r + s, c:c + s] for r, c in crop_origins(x.shape[2], x.shape[3], s, cfg["crops"])]
    return torch.stack(cut, 1).reshape(-1, 3, s, s).to(dtype)


def _lin(x, sd, name, dtype):
    return F.linear(x, sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype))


def _ln(x, sd, name, eps, dtype):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype), eps)


def vit_block(x, sd, i, heads, dtype, probe=None):
    """timm's pre-LN block on [B,T,dim]."""
    p = f"vit.blocks.{i}"
    B, T, dim = x.shape
    qkv = _lin(_ln(x, sd, p + ".norm1", 1e-6, dtype), sd, p + ".attn.qkv", dtype).reshape(B, T, 3, heads, dim // heads).permute(2, 0, 3, 1, 4)
    a = ((qkv[0] * (dim // heads) ** -0.5) @ qkv[1].transpose(-2, -1)).softmax(-1)
    if probe is not None:
        probe.append(a)
    x = x + _lin((a @ qkv[2]).transpose(1, 2).reshape(B, T, dim), sd, p + ".attn.proj", dtype)
    h = F.gelu(_lin(_ln(x, sd, p + ".norm2", 1e-6, dtype), sd, p + ".mlp.fc1", dtype))
    return x + _lin(h, sd, p + ".mlp.fc2", dtype)


def embed(c, sd, cfg, dtype):
    """Crops [B,3,side,side] -> [B,T + 1,dim]: the patch conv, the cls token in front, plus pos_embed."""
    x = F.conv2d(c, sd["vit.patch_embed.proj.weight"].to(dtype), sd["vit.patch_embed.proj.bias"].to(dtype), stride=cfg["patch"])
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([sd["vit.cls_token"].to(dtype).expand(x.shape[0], -1, -1), x], 1)
    return x + sd["vit.pos_embed"].to(dtype)


def trunk(c, sd, cfg, dtype):
    """Crops -> the hooked blocks' outputs without cls, side by side: [B,T,4 dim]."""
    x = embed(c, sd, cfg, dtype)
    keep = {}
    for i in range(max(cfg["hooks"]) + 1):
        x = vit_block(x, sd, i, cfg["heads"], dtype)
        if i in cfg["hooks"]:
            keep[i] = x[:, 1:]
    return torch.cat([keep[i] for i in cfg["hooks"]], 2)


def tablock(x, sd, name, dtype, quirk=True, probe=None):
    """The TABlock on channel rows [B,C,N]."""
    B, C, N = x.shape
    q, k, v = (_lin(x, sd, f"{name}.{n}", dtype) for n in ("c_q", "c_k", "c_v"))
    a = ((q @ k.transpose(-2, -1)) * N ** -0.5).softmax(-1)
    if probe is not None:
        probe.append(a)
    y = a @ v
    y = y.transpose(1, 2).reshape(B, C, N) if quirk else y
    return y + x


def _windows(x, w):
    B, H, W, C = x.shape
    return x.view(B, H // w, w, W // w, w, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, w * w, C)


def _unwindows(win, w, B, H, W):
    return win.view(B, H // w, W // w, w, w, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)


def swin_block(x, sd, p, side, window, shifted, heads, dtype, probe=None):
    """Swin's block on [B,side side,C]: a map no larger than the window uses its own side and no shift."""
    B, T, C = x.shape
    w, shift = (side, 0) if side <= window else (window, window // 2 if shifted else 0)
    h = _ln(x, sd, p + ".norm1", 1e-5, dtype).view(B, side, side, C)
    if shift:
        h = torch.roll(h, shifts=(-shift, -shift), dims=(1, 2))
    win = _windows(h, w)
    n = w * w
    qkv = _lin(win, sd, p + ".attn.qkv", dtype).reshape(-1, n, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    a = (qkv[0] * (C // heads) ** -0.5) @ qkv[1].transpose(-2, -1)
    ys, xs = torch.meshgrid(torch.arange(window), torch.arange(window), indexing="ij")
    pos = torch.stack([ys.flatten(), xs.flatten()])
    rel = pos[:, :, None] - pos[:, None, :] + (window - 1)
    index = (rel[0] * (2 * window - 1) + rel[1])[:n, :n]
    a = a + sd[p + ".attn.relative_position_bias_table"].to(dtype)[index.reshape(-1)].view(n, n, heads).permute(2, 0, 1)[None]
    if shift:
        ids = torch.zeros(1, side, side, 1)
        cnt = 0
        for hs in (slice(0, -w), slice(-w, -shift), slice(-shift, None)):
            for ws in (slice(0, -w), slice(-w, -shift), slice(-shift, None)):
                ids[:, hs, ws] = cnt
                cnt += 1
        mw = _windows(ids, w).squeeze(-1)
        mask = (mw[:, None, :] - mw[:, :, None] != 0).to(dtype) * -100.0
        nW = mask.shape[0]
        a = (a.view(B, nW, heads, n, n) + mask[None, :, None]).view(-1, heads, n, n)
    a = a.softmax(-1)
    if probe is not None:
        probe.append(a)
    y = _lin((a @ qkv[2]).transpose(1, 2).reshape(-1, n, C), sd, p + ".attn.proj", dtype)
    y = _unwindows(y, w, B, side, side)
    if shift:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    x = x + y.reshape(B, T, C)
    h = F.gelu(_lin(_ln(x, sd, p + ".norm2", 1e-5, dtype), sd, p + ".mlp.fc1", dtype))
    return x + _lin(h, sd, p + ".mlp.fc2", dtype)


def basic_layer(x, sd, name, layer, cfg, heads, dtype, probe=None):
    side = cfg["side"] // cfg["patch"]
    for j in range(cfg["swin_depth"]):
        x = swin_block(x, sd, f"{name}.layers.{layer}.blocks.{j}", side, cfg["window"], j % 2 == 1, heads, dtype, probe)
    return x


def swin_stage(x, sd, name, cfg, heads, dtype, scale=0.8, probe=None):
    """Token rows [B,T,C]: per BasicLayer x = scale layer(x) + x."""
    for l in range(cfg["swin_layers"]):
        x = scale * basic_layer(x, sd, name, l, cfg, heads, dtype, probe) + x
    return x


def conv1x1(x, sd, name, dtype):
    """Channel rows [B,C,T] -> [B,C',T]."""
    return F.conv1d(x, sd[name + ".weight"].to(dtype).flatten(1)[:, :, None], sd[name + ".bias"].to(dtype))


def head(x, sd, dtype, probe=None):
    """Token rows [B,T,c] -> the crop scores [B]."""
    f = F.relu(_lin(F.relu(_lin(x, sd, "fc_score.0", dtype)), sd, "fc_score.3", dtype))
    w = torch.sigmoid(_lin(F.relu(_lin(x, sd, "fc_weight.0", dtype)), sd, "fc_weight.3", dtype))
    if probe is not None:
        probe.append(w.sum(1).flatten())
    return (f * w).sum(1).flatten() / w.sum(1).flatten()


def after_trunk(feat, sd, cfg, dtype, quirk=True, scale=0.8, num_tab=2, probes=None):
    """[B,T,4 dim] -> the crop scores [B].  ``probes``: a dict that receives the softmax matrices (``tab``, ``swin``) and sum w (``w``)."""
    pr = (lambda k: probes.setdefault(k, [])) if probes is not None else (lambda k: None)
    x = feat.transpose(1, 2)
    for i in range(num_tab):
        x = tablock(x, sd, f"tablock1.{i}", dtype, quirk, pr("tab"))
    x = conv1x1(x, sd, "conv1", dtype).transpose(1, 2)
    x = swin_stage(x, sd, "swintransformer1", cfg, cfg["swin_heads"][0], dtype, scale, pr("swin")).transpose(1, 2)
    for i in range(num_tab):
        x = tablock(x, sd, f"tablock2.{i}", dtype, quirk, pr("tab"))
    x = conv1x1(x, sd, "conv2", dtype).transpose(1, 2)
    x = swin_stage(x, sd, "swintransformer2", cfg, cfg["swin_heads"][1], dtype, scale, pr("swin"))
    return head(x, sd, dtype, pr("w"))


def maniqa(img, sd, cfg, dtype, quirk=True, scale=0.8, num_tab=2, probes=None):
    """Images -> [N] scores in ``dtype``: the mean over each frame's crops."""
    c = crops(img, cfg, dtype)
    s = after_trunk(trunk(c, sd, cfg, dtype), sd, cfg, dtype, quirk, scale, num_tab, probes)
    return s.view(-1, cfg["crops"]).mean(1)


def short_mantissa(x, bits=12):
    """fp32 values cut to ``bits`` significant bits, so that a product of two of them has at most 2 ``bits`` <= 24."""
    return (x.float().contiguous().view(torch.int32) & ~((1 << (24 - bits)) - 1)).view(torch.float32)


def fmaf_chain(a, b):
    """[M,K] x [K,N] in fp32 as one fmaf chain over k ascending per output, emulated in fp64 for operands from ``short_mantissa``: their
    products have 24 bits, so acc + product is exact in fp64 while the two exponents are within 29 of each other (24 + 24 bits and the gap
    fit 53), and its one rounding to fp32 is the fmaf's."""
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k in range(a.shape[1]):
        acc = (acc.double() + a[:, k, None].double() * b[None, k, :].double()).float()
    return acc
