"""MUSIQ in plain torch, in the shape of pyiqa's computation (restated from memory of ``musiq_arch.py`` / ``multiscale_trans_util.py``):
F.interpolate for the resize and the spatial hash, F.unfold on the padded image, padded token rows with a mask, StdConv standardising on
every forward, nn.functional.group_norm / layer_norm, a full score matrix with masked_fill(-1e3).  ``dtype`` switches every tensor between
float32 and float64.  Shares no code with dove_amd/musiq.py."""
import math

import torch
import torch.nn.functional as F

P, GRID = 32, 10
LONGER = (224, 384)
HEADS, WIDTH = 6, 384
MASK_FILL = -1e3


def resize(img, longer):
    H, W = img.shape[-2:]
    ratio = longer / max(H, W)
    rh, rw = max(1, round(H * ratio)), max(1, round(W * ratio))
    return F.interpolate(img, size=(rh, rw), mode="bicubic", align_corners=False)


def hashed_index(count_h, count_w):
    pos = torch.arange(GRID, dtype=torch.float32)[None, None]
    hh = F.interpolate(pos, size=count_h, mode="nearest")[0, 0].long()
    hw = F.interpolate(pos, size=count_w, mode="nearest")[0, 0].long()
    return (hh[:, None] * GRID + hw[None, :]).reshape(-1)


def scale_patches(img, scale_id, max_len):
    """img [N,3,h,w] in mapped values -> (patches [N,L,3,32,32], spatial [L], scale [L], mask [L]); L = max_len when given (zero patches,
    mask 0 behind the real ones)."""
    N, C, h, w = img.shape
    ch, cw = -(-h // P), -(-w // P)
    ph, pw = ch * P - h, cw * P - w
    padded = F.pad(img, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))
    cols = F.unfold(padded, kernel_size=P, stride=P)                              # [N, 3 * 32 * 32, ch * cw], row-major patches
    pat = cols.transpose(1, 2).reshape(N, ch * cw, C, P, P)
    spatial = hashed_index(ch, cw)
    mask = torch.ones(ch * cw, dtype=torch.bool)
    if max_len is not None and max_len > ch * cw:
        extra = max_len - ch * cw
        pat = torch.cat([pat, pat.new_zeros(N, extra, C, P, P)], dim=1)
        spatial = torch.cat([spatial, spatial.new_zeros(extra)])
        mask = torch.cat([mask, mask.new_zeros(extra)])
    return pat, spatial, torch.full((pat.shape[1],), scale_id, dtype=torch.long), mask


def multiscale_patches(img01, padded=True):
    """img01 [N,1|3,H,W] in [0,1] -> patches [N,L,3,32,32] of 2 v - 1, spatial [L], scale [L], mask [L] (the same for every image)."""
    if img01.shape[1] == 1:
        img01 = img01.expand(-1, 3, -1, -1)
    x = img01 * 2 - 1
    parts = []
    for sid, longer in enumerate(LONGER):
        parts.append(scale_patches(resize(x, longer), sid, math.ceil(longer / P) ** 2 if padded else None))
    parts.append(scale_patches(x, len(LONGER), None))
    return tuple(torch.cat([p[i] for p in parts], dim=1 if i == 0 else 0) for i in range(4))


def std_conv(x, w, stride=1, padding=0):
    m = w.mean(dim=(1, 2, 3), keepdim=True)
    s = w.std(dim=(1, 2, 3), keepdim=True)
    return F.conv2d(x, (w - m) / (s + 1e-5), None, stride, padding)


def stem(sd, x, dtype):
    """x [M,3,32,32] -> [M,16384], the 8 x 8 x 256 map flattened (h, w, c)."""
    g = lambda k: sd[k].to(dtype)
    gn = lambda t, n, eps: F.group_norm(t, 32, g(f"{n}.weight"), g(f"{n}.bias"), eps)
    x = std_conv(F.pad(x, (2, 3, 2, 3)), g("conv_root.weight"), 2)
    x = F.relu(gn(x, "gn_root", 1e-6))
    x = F.max_pool2d(F.pad(x, (0, 1, 0, 1)), 3, 2)
    ident = gn(std_conv(x, g("block1.conv_proj.weight")), "block1.gn_proj", 1e-4)
    y = F.relu(gn(std_conv(x, g("block1.conv1.weight")), "block1.gn1", 1e-4))
    y = F.relu(gn(std_conv(y, g("block1.conv2.weight"), 1, 1), "block1.gn2", 1e-4))
    y = gn(std_conv(y, g("block1.conv3.weight")), "block1.gn3", 1e-4)
    return F.relu(ident + y).permute(0, 2, 3, 1).reshape(x.shape[0], -1)


def attention(q, k, v, mask=None, taps=None):
    """q, k, v [B,L,384] -> [B,L,384]; mask bool [L] of the keys (None: no masking).  taps: a list that receives the scaled scores."""
    B, L, _ = q.shape
    hd = WIDTH // HEADS
    sp = lambda t: t.view(B, L, HEADS, hd).transpose(1, 2)
    s = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(hd)
    if taps is not None:
        taps.append(s if mask is None else s[:, :, mask][:, :, :, mask])
    if mask is not None:
        s = s.masked_fill(~mask[None, None, None, :], MASK_FILL)
    return (torch.softmax(s, dim=-1) @ sp(v)).transpose(1, 2).reshape(B, L, WIDTH)


def encoder(sd, x, mask, layers, taps=None):
    g = lambda k: sd[k].to(x.dtype)
    for i in range(layers):
        p = f"transformer_encoder.transformer.encoderblock_{i:02d}"
        lin = lambda t, n: F.linear(t, g(f"{p}.{n}.weight"), g(f"{p}.{n}.bias"))
        h = F.layer_norm(x, (WIDTH,), g(f"{p}.norm1.weight"), g(f"{p}.norm1.bias"), 1e-6)
        a = attention(lin(h, "attention.query"), lin(h, "attention.key"), lin(h, "attention.value"), mask, taps)
        x = x + lin(a, "attention.out")
        h = F.layer_norm(x, (WIDTH,), g(f"{p}.norm2.weight"), g(f"{p}.norm2.bias"), 1e-6)
        x = x + lin(F.gelu(lin(h, "mlp.fc1")), "mlp.fc2")
    return F.layer_norm(x, (WIDTH,), g("transformer_encoder.encoder_norm.weight"), g("transformer_encoder.encoder_norm.bias"), 1e-6)


def musiq(sd, img01, dtype=torch.float64, padded=True, layers=14, taps=None):
    """img01 [N,1|3,H,W] in [0,1] -> (score [N], token-0 feature [N,384]).  padded: pyiqa's form with masked padding rows; otherwise the
    rows are deleted and nothing is masked."""
    g = lambda k: sd[k].to(dtype)
    pat, spatial, scale, mask = multiscale_patches(img01.to(dtype), padded)
    N, L = pat.shape[:2]
    emb = F.linear(stem(sd, pat.reshape(N * L, 3, P, P), dtype), g("embedding.weight"), g("embedding.bias")).view(N, L, WIDTH)
    x = emb + g("transformer_encoder.posembed_input.position_emb")[0, spatial] + g("transformer_encoder.scaleembed_input.scale_emb")[0, scale]
    x = torch.cat([g("transformer_encoder.cls").expand(N, 1, WIDTH), x], dim=1)
    keys = torch.cat([torch.ones(1, dtype=torch.bool), mask])
    feat = encoder(sd, x, keys if padded else None, layers, taps)[:, 0]
    row = F.linear(feat, g("head.weight"), g("head.bias"))
    if row.shape[1] == 1:
        return row[:, 0], feat
    return (torch.softmax(row, dim=-1) * torch.arange(1, row.shape[1] + 1, dtype=dtype)).sum(dim=-1), feat
