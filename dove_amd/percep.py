"""The perceptual full-reference metrics LPIPS (v0.1, AlexNet or VGG16) and DISTS on the GPU, trunks in exact fp32 (csrc/percep.hip).

The definitions are pyiqa's defaults (``pyiqa.create_metric('lpips' | 'lpips-vgg' | 'dists')``), restated from the published LPIPS v0.1
and DISTS code:

  LPIPS: images in [0,1] are mapped to 2 v - 1, then (. - shift) / scale per channel; the trunk's five ReLU outputs are tapped (AlexNet:
    64, 192, 384, 256, 256 channels, 3/2 max-pools before conv2 and conv3; VGG16: relu1_2, 2_2, 3_3, 4_3, 5_3 with 2/2 max-pools between
    the stages).  Per tap, each pixel's feature vector is divided by (its L2 norm + 1e-10), the squared difference of the two images is
    weighted by the non-negative ``lin`` vector and averaged over the pixels; the value is the sum over the five taps.
  DISTS: (v - mean) / std, the same VGG16 convs with an L2 pool (Hann window (1/4, 1/2, 1/4), stride 2) in place of each max-pool.  Six
    feature sets - the un-normalised image and the five stage outputs, 3 + 64 + 128 + 256 + 512 + 512 = 1475 channels - give per channel
    S1 = (2 mx my + c) / (mx^2 + my^2 + c) and S2 = (2 cov + c) / (vx + vy + c), c = 1e-6, and the score is
    1 - sum(alpha S1 + beta S2) / (sum(alpha) + sum(beta)).

The user supplies the checkpoints (torchvision's backbone plus the metric's own small file), as for RAFT.  This module walks the trunk in
Python; every operator is a kernel of the library.  Prediction and ground truth go through the trunk as one batch, in groups of frames
sized so that the live activations of a group stay under ``ACTIVATION_BUDGET``; a frame's value does not depend on the grouping.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

from . import iqa, ops
from .iqa import ACTIVATION_BUDGET, FLOAT32_DTYPES, GpuMetric, as_nchw, find_file, for_groups, load_state_dict
from .netweights import Weights, checked, he_normal, pack_conv_weight, random_tensors, strip

ALEX_CONVS = ((0, 64, 3, 11, 4, 2), (3, 192, 64, 5, 1, 2), (6, 384, 192, 3, 1, 1), (8, 256, 384, 3, 1, 1), (10, 256, 256, 3, 1, 1))
VGG_STAGES = (((0, 64, 3), (2, 64, 64)), ((5, 128, 64), (7, 128, 128)), ((10, 256, 128), (12, 256, 256), (14, 256, 256)),
              ((17, 512, 256), (19, 512, 512), (21, 512, 512)), ((24, 512, 512), (26, 512, 512), (28, 512, 512)))
LPIPS_CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}
DISTS_CHANNELS = (3, 64, 128, 256, 512, 512)
MIN_SIDE = {"alex": 31, "vgg": 16}                  # the last tap is 1 x 1 at this size
LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)
DISTS_MEAN, DISTS_STD = (.485, .456, .406), (.229, .224, .225)
# Live fp32 activations of one trunk group.  The peak of VGG16 is conv1_2: its 64-channel input and output at full resolution, next to the
# 3-channel images (one 720 x 1280 stage-1 map is 236 MB); of AlexNet conv1's output at 1/16 of the pixels.  4 GiB holds four 720p pairs.
FILE_PATTERNS = {"alex": "alexnet*.pth", "vgg": "vgg16*.pth", "lpips-alex": "LPIPS_v0.1_alex*.pth", "lpips-vgg": "LPIPS_v0.1_vgg*.pth",
                 "dists": "DISTS_weights*.pth"}
COUNTERS = {"groups": 0}                            # trunk groups walked, for tests and tools


def backbone_param_shapes(net: str) -> dict:
    """name -> shape of the conv entries of torchvision's ``alexnet`` / ``vgg16`` state dict that the metrics read."""
    if net == "alex":
        convs = [(n, cout, cin, k) for n, cout, cin, k, _, _ in ALEX_CONVS]
    elif net == "vgg":
        convs = [(n, cout, cin, 3) for stage in VGG_STAGES for n, cout, cin in stage]
    else:
        raise ValueError(f"net must be 'alex' or 'vgg', got {net!r}")
    s = {}
    for n, cout, cin, k in convs:
        s[f"features.{n}.weight"] = (cout, cin, k, k)
        s[f"features.{n}.bias"] = (cout,)
    return s


def _random_backbone(seed: int, net: str) -> dict:
    rule = lambda name, shape, rng: he_normal(rng, shape) if len(shape) == 4 else 0.05 * rng.standard_normal(shape)
    return random_tensors(backbone_param_shapes(net), seed, lambda name: f"{net}.{name}", rule)


def _uniform(seed: int, key: str, channels: int) -> torch.Tensor:
    rng = np.random.default_rng([int(seed), zlib.crc32(key.encode())])
    return torch.from_numpy(rng.uniform(0.05, 1.0, (1, channels, 1, 1)).astype(np.float32))


def random_lpips_state(seed: int, net: str):
    """Rule-generated (backbone_sd, lin_sd) for tests and tools: conv weights normal with He std, biases 0.05 * normal, lin uniform in
    [0.05, 1]."""
    return _random_backbone(seed, net), {f"lin{k}.model.1.weight": _uniform(seed, f"{net}.lin{k}", c) for k, c in enumerate(LPIPS_CHANNELS[net])}


def random_dists_state(seed: int):
    """Rule-generated (backbone_sd, ab_sd): the VGG16 of ``random_lpips_state`` and alpha, beta uniform in [0.05, 1]."""
    return _random_backbone(seed, "vgg"), {name: _uniform(seed, f"dists.{name}", sum(DISTS_CHANNELS)) for name in ("alpha", "beta")}


def _pack_backbone(sd: dict, net: str) -> dict:
    sd = checked(strip(sd), backbone_param_shapes(net), f"{'AlexNet' if net == 'alex' else 'VGG16'} checkpoint")
    nums = [c[0] for c in ALEX_CONVS] if net == "alex" else [c[0] for stage in VGG_STAGES for c in stage]
    return {n: (pack_conv_weight(sd[f"features.{n}.weight"]), sd[f"features.{n}.bias"].float().contiguous()) for n in nums}


@dataclass
class LpipsWeights(Weights):
    convs: dict = field(default_factory=dict)       # features.N -> (w [kh,kw,cin,cout], bias)
    net: str = "alex"
    lins: list = field(default_factory=list)        # five float32 [C]

    @classmethod
    def from_state_dicts(cls, backbone_sd: dict, lin_sd: dict, net: str) -> "LpipsWeights":
        convs = _pack_backbone(backbone_sd, net)
        want = {f"lin{k}.model.1.weight": (1, c, 1, 1) for k, c in enumerate(LPIPS_CHANNELS[net])}
        lin_sd = checked(strip(lin_sd), want, f"LPIPS v0.1 ({net}) linear layers")
        return cls(convs=convs, net=net, lins=[lin_sd[name].float().reshape(-1).contiguous() for name in want])

    @classmethod
    def load(cls, backbone_path: str, lin_path: str, net: str) -> "LpipsWeights":
        return cls.from_state_dicts(load_state_dict(backbone_path), load_state_dict(lin_path), net)


@dataclass
class DistsWeights(Weights):
    convs: dict = field(default_factory=dict)       # as LpipsWeights.convs
    alpha: list = field(default_factory=list)       # six float64 [C], divided by sum(alpha) + sum(beta)
    beta: list = field(default_factory=list)

    @classmethod
    def from_state_dicts(cls, backbone_sd: dict, ab_sd: dict) -> "DistsWeights":
        convs = _pack_backbone(backbone_sd, "vgg")
        total = sum(DISTS_CHANNELS)
        ab_sd = checked(strip(ab_sd), {"alpha": (1, total, 1, 1), "beta": (1, total, 1, 1)}, "DISTS weights")
        a, b = ab_sd["alpha"].double().reshape(-1), ab_sd["beta"].double().reshape(-1)
        w_sum = a.sum() + b.sum()
        split = lambda t: [s.contiguous() for s in torch.split(t / w_sum, list(DISTS_CHANNELS))]
        return cls(convs=convs, alpha=split(a), beta=split(b))

    @classmethod
    def load(cls, backbone_path: str, ab_path: str) -> "DistsWeights":
        return cls.from_state_dicts(load_state_dict(backbone_path), load_state_dict(ab_path))


def load_metric_weights(directory: str, name: str):
    """Weights of metric ``name`` ('lpips', 'lpips-vgg', 'dists') from a directory of checkpoints (the names torchvision and pyiqa give
    their downloads: ``FILE_PATTERNS``)."""
    file = lambda key: find_file(directory, FILE_PATTERNS[key])
    if name == "lpips":
        return LpipsWeights.load(file("alex"), file("lpips-alex"), "alex")
    if name == "lpips-vgg":
        return LpipsWeights.load(file("vgg"), file("lpips-vgg"), "vgg")
    if name == "dists":
        return DistsWeights.load(file("vgg"), file("dists"))
    raise ValueError(f"no network weights belong to metric {name!r}")


# ------------------------------------------------------------------- walk -------------------------------------------------------------------
def _inputs(pred: torch.Tensor, ref: torch.Tensor, net: str, what: str):
    p, r = as_nchw(pred, "auto"), as_nchw(ref, "auto")
    if p.shape != r.shape or p.shape[1] not in (1, 3):
        raise ValueError(f"{what}: pred {tuple(pred.shape)} and ref {tuple(ref.shape)} must be the same [N,1|3,H,W] shape")
    # device=t.device: a host tensor is not uploaded here; it is refused below, once its size has been checked
    p, r = (iqa.images(t, what, (MIN_SIDE[net],) * 2, FLOAT32_DTYPES, device=t.device) for t in (p, r))
    if not (p.is_cuda and r.is_cuda) or p.device != r.device:
        raise RuntimeError(f"{what} needs both images on the same HIP device (`cuda`); there is no CPU path")
    return p, r


def group_size(net: str, h: int, w: int, budget: int | None = None) -> int:
    """Frame pairs per trunk group: the most whose live activations (both images of each pair) stay under the budget, at least one."""
    per_pixel = 4 * (3 + 3 + 64 + 64) if net == "vgg" else 4 * (3 + 8)
    return max(1, int((ACTIVATION_BUDGET if budget is None else budget) // (2 * per_pixel * h * w)))


def _conv(W, n: int, x: torch.Tensor, stride: int = 1, pad: int = 1) -> torch.Tensor:
    w, b = W.convs[n]
    return ops.convnet_conv_f32(x, w, b, stride=stride, pad=(pad, pad), relu=True)


def _alex_taps(W, x):
    for n, _, _, _, stride, pad in ALEX_CONVS:
        if n in (3, 6):
            x = ops.maxpool_f32(x, 3, 2)
        x = _conv(W, n, x, stride, pad)
        yield x


def _vgg_taps(W, x, l2: bool):
    for k, stage in enumerate(VGG_STAGES):
        if k:
            x = ops.l2pool_f32(x) if l2 else ops.maxpool_f32(x, 2, 2)
        for n, _, _ in stage:
            x = _conv(W, n, x)
        yield x


def _walk(W, pred, ref, net: str, what: str, group, per_group):
    p, r = _inputs(pred, ref, net, what)
    W = W.to(p.device)
    out = torch.zeros(p.shape[0], dtype=torch.float64, device=p.device)
    for_groups(p.shape[0], group, group_size(net, p.shape[2], p.shape[3]), COUNTERS, p.device,
               lambda i, j: per_group(W, p[i:j], r[i:j], out[i:j]))
    return out


def _prep_pair(p, r, pre_mul, pre_add, mean, std):
    g, _, H, Wd = p.shape
    x = torch.empty(2 * g, H, Wd, 3, dtype=torch.float32, device=p.device)
    ops.percep_prep_f32(p, pre_mul, pre_add, mean, std, out=x[:g])
    ops.percep_prep_f32(r, pre_mul, pre_add, mean, std, out=x[g:])
    return x


def lpips(W: LpipsWeights, pred: torch.Tensor, ref: torch.Tensor, group: int | None = None) -> torch.Tensor:
    """LPIPS v0.1 per image -> float64 [N] on the device.  ``pred`` / ``ref``: [N,C,H,W] float in [0,1] or uint8 (any strides, C in
    {1, 3}; one channel is repeated), or [F,H,W,3] uint8 frames.  ``group``: frame pairs per trunk batch (default: from the budget)."""

    def per_group(Wd, p, r, out):
        g = p.shape[0]
        x = _prep_pair(p, r, 2.0, -1.0, LPIPS_SHIFT, LPIPS_SCALE)
        taps = _alex_taps(Wd, x) if Wd.net == "alex" else _vgg_taps(Wd, x, False)
        for lin, f in zip(Wd.lins, taps):
            ops.lpips_layer(f[:g], f[g:], lin, out)

    return _walk(W, pred, ref, W.net, "lpips", group, per_group)


def dists(W: DistsWeights, pred: torch.Tensor, ref: torch.Tensor, group: int | None = None) -> torch.Tensor:
    """DISTS per image -> float64 [N] on the device; inputs as for ``lpips``."""

    def per_group(Wd, p, r, out):
        g = p.shape[0]
        raw = _prep_pair(p, r, 1.0, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        acc = torch.zeros(g, dtype=torch.float64, device=p.device)
        ops.dists_layer(raw[:g], raw[g:], Wd.alpha[0], Wd.beta[0], acc)
        del raw
        x = _prep_pair(p, r, 1.0, 0.0, DISTS_MEAN, DISTS_STD)
        for k, f in enumerate(_vgg_taps(Wd, x, True)):
            ops.dists_layer(f[:g], f[g:], Wd.alpha[k + 1], Wd.beta[k + 1], acc)
        out.copy_(1.0 - acc)

    return _walk(W, pred, ref, "vgg", "dists", group, per_group)


class PerceptualMetric(GpuMetric):
    """pyiqa-style metric object for 'lpips', 'lpips-vgg' and 'dists': ``metric(pred, ref)`` with [N,C,H,W] images in [0,1] -> [N] fp64."""

    def __init__(self, name: str, weights):
        net = {"lpips": "alex", "lpips-vgg": "vgg"}.get(name)
        super().__init__(name, True, True, dists if net is None else lpips, weights, DistsWeights if net is None else LpipsWeights)
        if net is not None and weights.net != net:
            raise TypeError(f"create_metric('{name}'): weights must be a {__name__}.LpipsWeights of net '{net}'")
