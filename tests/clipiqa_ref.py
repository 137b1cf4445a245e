"""Torch restatement of CLIP-IQA (pyiqa's ``clipiqa``: CLIP RN50 without the positional embedding of its attention pool, five prompt pairs),
written from the definition in INTEGRATION.md 1j - not from the kernels: NCHW, dtype-generic (the same code runs fp32 and fp64), BatchNorm
unfolded (``F.batch_norm``), and the attention pool in its textbook form, with keys and values projected over ALL tokens (the kernel's
one-query algebra is not used here).  It also holds the text tower and a second, naive byte-pair encoder."""
import math

import torch
import torch.nn.functional as F

MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
LAYERS, PLANES = (3, 4, 6, 3), (64, 128, 256, 512)


def _bn(sd, name, x):
    g = lambda k: sd[f"{name}.{k}"].to(x.dtype)
    return F.batch_norm(x, g("running_mean"), g("running_var"), g("weight"), g("bias"), training=False, eps=1e-5)


def _conv(sd, name, x, **kw):
    return F.conv2d(x, sd[f"{name}.weight"].to(x.dtype), None, **kw)


def bottleneck(sd, p, x, stride):
    out = F.relu(_bn(sd, f"{p}.bn1", _conv(sd, f"{p}.conv1", x)))
    out = F.relu(_bn(sd, f"{p}.bn2", _conv(sd, f"{p}.conv2", out, padding=1)))
    if stride > 1:
        out = F.avg_pool2d(out, stride)
    out = _bn(sd, f"{p}.bn3", _conv(sd, f"{p}.conv3", out))
    if f"{p}.downsample.0.weight" in sd:
        x = _bn(sd, f"{p}.downsample.1", _conv(sd, f"{p}.downsample.0", F.avg_pool2d(x, stride) if stride > 1 else x))
    return F.relu(out + x)


def visual_features(sd, img):
    """img [N,1|3,H,W] in [0,1] -> [N,2048,h,w]."""
    if img.shape[1] == 1:
        img = img.expand(-1, 3, -1, -1)
    x = (img - torch.tensor(MEAN, dtype=img.dtype)[None, :, None, None]) / torch.tensor(STD, dtype=img.dtype)[None, :, None, None]
    x = F.relu(_bn(sd, "visual.bn1", _conv(sd, "visual.conv1", x, stride=2, padding=1)))
    x = F.relu(_bn(sd, "visual.bn2", _conv(sd, "visual.conv2", x, padding=1)))
    x = F.relu(_bn(sd, "visual.bn3", _conv(sd, "visual.conv3", x, padding=1)))
    x = F.avg_pool2d(x, 2)
    for li, n in enumerate(LAYERS):
        for i in range(n):
            x = bottleneck(sd, f"visual.layer{li + 1}.{i}", x, 2 if (li > 0 and i == 0) else 1)
    return x


def attnpool(sd, feat, heads=32, want_scores=False):
    """feat [N,C,h,w] -> [N,1024]: full multi-head attention over the h w + 1 tokens (no positional embedding), token 0's output kept.
    ``want_scores``: return the pre-softmax scores [N,heads,T,T] instead."""
    g = lambda k: sd[f"visual.attnpool.{k}"].to(feat.dtype)
    N, Cc = feat.shape[:2]
    t = feat.flatten(2).permute(0, 2, 1)                                     # [N, hw, C]
    t = torch.cat([t.mean(dim=1, keepdim=True), t], dim=1)                   # [N, hw + 1, C]
    q, k, v = (F.linear(t, g(f"{n}_proj.weight"), g(f"{n}_proj.bias")) for n in "qkv")
    hd = Cc // heads
    split = lambda a: a.view(N, -1, heads, hd).transpose(1, 2)               # [N, heads, T, hd]
    scores = (split(q) * hd ** -0.5) @ split(k).transpose(-1, -2)
    if want_scores:
        return scores
    att = torch.softmax(scores, dim=-1) @ split(v)
    out = F.linear(att.transpose(1, 2).reshape(N, -1, Cc), g("c_proj.weight"), g("c_proj.bias"))
    return out[:, 0]


def score(emb, text, logit_scale):
    """emb [N,D], text [2P,D] (any scale) -> [N]: mean over the pairs of softmax(logits of the pair)[0]."""
    f = emb / emb.norm(dim=1, keepdim=True)
    t = text.to(emb.dtype)
    t = t / t.norm(dim=1, keepdim=True)
    logits = (logit_scale * f @ t.T).view(emb.shape[0], -1, 2)
    return torch.softmax(logits, dim=-1)[..., 0].mean(dim=1)


def clipiqa_ref(sd, text, img, want_parts=False):
    """-> scores [N] in img's dtype; with ``want_parts`` also the normalised embedding and the pairs' logit differences."""
    feat = visual_features(sd, img)
    if feat.shape[2] < 1 or feat.shape[3] < 1:
        raise ValueError("image too small")
    emb = attnpool(sd, feat)
    feats = torch.as_tensor(text["features"])
    scale = math.exp(float(sd["logit_scale"]))
    s = score(emb, feats, scale)
    if not want_parts:
        return s
    f = emb / emb.norm(dim=1, keepdim=True)
    t = feats.to(emb.dtype)
    t = t / t.norm(dim=1, keepdim=True)
    logits = (scale * f @ t.T).view(emb.shape[0], -1, 2)
    return s, f, logits[..., 0] - logits[..., 1]


# --------------------------------------------------------------- the text side ---------------------------------------------------------------
def text_tower(sd, tokens, dtype=torch.float64, heads=8):
    """CLIP's text transformer with nn.functional's own multi-head attention: tokens [B,L] -> [B,1024]."""
    g = lambda k: sd[k].to(dtype)
    B, Lc = tokens.shape
    width = sd["ln_final.weight"].numel()
    x = g("token_embedding.weight")[tokens] + g("positional_embedding")[:Lc]
    mask = torch.full((Lc, Lc), float("-inf"), dtype=dtype).triu(1)
    x = x.permute(1, 0, 2)                                                   # [L, B, width]
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        p = f"transformer.resblocks.{i}"
        h = F.layer_norm(x, (width,), g(f"{p}.ln_1.weight"), g(f"{p}.ln_1.bias"))
        a, _ = F.multi_head_attention_forward(h, h, h, width, heads, g(f"{p}.attn.in_proj_weight"), g(f"{p}.attn.in_proj_bias"), None, None,
                                              False, 0.0, g(f"{p}.attn.out_proj.weight"), g(f"{p}.attn.out_proj.bias"), training=False,
                                              need_weights=False, attn_mask=mask)
        x = x + a
        h = F.layer_norm(x, (width,), g(f"{p}.ln_2.weight"), g(f"{p}.ln_2.bias"))
        h = F.linear(h, g(f"{p}.mlp.c_fc.weight"), g(f"{p}.mlp.c_fc.bias"))
        x = x + F.linear(h * torch.sigmoid(1.702 * h), g(f"{p}.mlp.c_proj.weight"), g(f"{p}.mlp.c_proj.bias"))
        i += 1
    x = F.layer_norm(x.permute(1, 0, 2), (width,), g("ln_final.weight"), g("ln_final.bias"))
    return x[torch.arange(B), tokens.argmax(dim=-1)] @ g("text_projection")


def naive_bpe_step(parts, a, b):
    """One rule over the whole word, left to right."""
    i, out = 0, []
    while i < len(parts):
        if i + 1 < len(parts) and parts[i] == a and parts[i + 1] == b:
            out.append(a + b)
            i += 2
        else:
            out.append(parts[i])
            i += 1
    return out


def naive_bpe(word_chars, merges):
    """The merges applied one rule at a time in rank order, each over the whole word: for a merge list in which a rule's parts are made
    by earlier rules this is the greedy lowest-rank-first encoder in another order of work."""
    parts = list(word_chars[:-1]) + [word_chars[-1] + "</w>"]
    for a, b in merges:
        parts = naive_bpe_step(parts, a, b)
    return parts
