"""Torch restatement of LPIPS v0.1 (AlexNet / VGG16) and DISTS, written from their definitions in NCHW with
``F.conv2d`` / ``F.max_pool2d``.  Dtype-generic: the dtype of the images decides, so the same code runs in fp32 and fp64 on the host.
It takes the raw state dicts (torchvision's ``features.N.weight/bias``, ``lin{k}.model.1.weight``, ``alpha`` / ``beta``)."""
import torch
import torch.nn.functional as F

ALEX = ((0, 4, 2), (3, 1, 2), (6, 1, 1), (8, 1, 1), (10, 1, 1))                   # features.N, stride, padding
VGG = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
DISTS_CHANNELS = (3, 64, 128, 256, 512, 512)


def _rgb(x):
    return x.expand(-1, 3, -1, -1) if x.shape[1] == 1 else x


def _conv(sd, n, x, stride=1, padding=1):
    return F.relu(F.conv2d(x, sd[f"features.{n}.weight"].to(x.dtype), sd[f"features.{n}.bias"].to(x.dtype), stride=stride, padding=padding))


def l2pool_ref(x):
    """sqrt(sum_taps g x^2 + 1e-12), g the normalised outer product of (0.5, 1, 0.5), stride 2, zero padding 1, per channel."""
    a = torch.tensor([0.5, 1.0, 0.5], dtype=x.dtype)
    g = a[:, None] * a[None, :]
    g = g / g.sum()
    xp = F.pad(x * x, (1, 1, 1, 1))
    out = sum(g[i, j] * xp[:, :, i::2, j::2][:, :, :(x.shape[2] - 1) // 2 + 1, :(x.shape[3] - 1) // 2 + 1] for i in range(3) for j in range(3))
    return torch.sqrt(out + 1e-12)


def alex_taps(sd, x):
    taps = []
    for n, stride, padding in ALEX:
        if n in (3, 6):
            x = F.max_pool2d(x, 3, 2)
        x = _conv(sd, n, x, stride, padding)
        taps.append(x)
    return taps


def vgg_taps(sd, x, l2=False):
    taps = []
    for k, stage in enumerate(VGG):
        if k:
            x = l2pool_ref(x) if l2 else F.max_pool2d(x, 2, 2)
        for n in stage:
            x = _conv(sd, n, x)
        taps.append(x)
    return taps


def lpips_head_ref(fx, fy, lin):
    """fx, fy [N,C,H,W], lin [C] -> [N]."""
    nx = fx / (torch.sqrt((fx * fx).sum(1, keepdim=True)) + 1e-10)
    ny = fy / (torch.sqrt((fy * fy).sum(1, keepdim=True)) + 1e-10)
    return (lin.to(fx.dtype).view(1, -1, 1, 1) * (nx - ny) ** 2).sum(1).mean((1, 2))


def dists_head_ref(fx, fy, alpha, beta):
    """fx, fy [N,C,H,W], alpha, beta [C] already normalised -> [N] = sum_c alpha S1 + beta S2."""
    mx, my = fx.mean((2, 3), keepdim=True), fy.mean((2, 3), keepdim=True)
    vx, vy = ((fx - mx) ** 2).mean((2, 3)), ((fy - my) ** 2).mean((2, 3))
    cov = ((fx - mx) * (fy - my)).mean((2, 3))
    mx, my = mx.flatten(1), my.flatten(1)
    s1 = (2 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6)
    s2 = (2 * cov + 1e-6) / (vx + vy + 1e-6)
    return (alpha.to(fx.dtype) * s1 + beta.to(fx.dtype) * s2).sum(1)


def lpips_ref(backbone_sd, lin_sd, net, x, y):
    """x, y [N,1|3,H,W] in [0,1] -> [N] in their dtype."""
    dt = x.dtype
    shift = torch.tensor([-.030, -.088, -.188], dtype=dt).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], dtype=dt).view(1, 3, 1, 1)
    prep = lambda v: ((2 * _rgb(v) - 1) - shift) / scale
    taps = alex_taps if net == "alex" else vgg_taps
    fx, fy = taps(backbone_sd, prep(x)), taps(backbone_sd, prep(y))
    return sum(lpips_head_ref(a, b, lin_sd[f"lin{k}.model.1.weight"].reshape(-1)) for k, (a, b) in enumerate(zip(fx, fy)))


def dists_ref(backbone_sd, ab_sd, x, y):
    dt = x.dtype
    mean = torch.tensor([.485, .456, .406], dtype=dt).view(1, 3, 1, 1)
    std = torch.tensor([.229, .224, .225], dtype=dt).view(1, 3, 1, 1)
    x, y = _rgb(x), _rgb(y)
    fx = [x] + vgg_taps(backbone_sd, (x - mean) / std, l2=True)
    fy = [y] + vgg_taps(backbone_sd, (y - mean) / std, l2=True)
    a, b = ab_sd["alpha"].double().reshape(-1), ab_sd["beta"].double().reshape(-1)
    w_sum = a.sum() + b.sum()
    a, b = torch.split(a / w_sum, list(DISTS_CHANNELS)), torch.split(b / w_sum, list(DISTS_CHANNELS))
    return 1 - sum(dists_head_ref(p, q, a[k], b[k]) for k, (p, q) in enumerate(zip(fx, fy)))
