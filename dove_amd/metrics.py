"""Full-reference metrics of the reference's evaluation step on the GPU: PSNR and SSIM (csrc/metrics.hip, ``dove_fr_metrics``).

Three surfaces:
  - ``fr_metrics(pred, ref, psnr=True, ssim=True, rgb_to_y=False)``: per-image fp64 values of a batch of strided views;
  - ``create_metric(name)``: pyiqa's ``create_metric`` surface, so the reference's metric code runs with ``import dove_amd.metrics as
    pyiqa``.  ``REGISTRY`` declares every metric once, in the order of the command lines' lists: the full-reference metrics computed from
    the images alone, and the ones made by ``create_metric(name, weights=W)`` from files the user supplies (a network metric is called as
    ``metric(pred, ref)``, a no-reference one as ``metric(pred)``); any other name, or one of these without weights, raises
    ``NotImplementedError``.  The evaluation tool and the inference command line read the same table;
  - ``clip_metrics(pred_u8, gt_u8, names, crop, test_y_channel, is_center)``: the per-clip logic of eval_metrics.py (match_resolution,
    crop_border, rgb_to_y, mean over frames), as views on the device; ``nr_clip_metrics(pred_u8, names, weights)`` is its ground-truth-free
    half (the no-reference metrics on the predictions as they are).

Definitions (pyiqa's 'psnr' / 'ssim' defaults, INTEGRATION.md 'Metrics'): values in [0,1], uint8 read as u/255.
PSNR = 10 log10(1 / (mse + 1e-8)) over C, H, W.  SSIM on the luma Y = round(255 (0.299 R + 0.587 G + 0.114 B)) (round(255 v) for one
channel), 11x11 Gaussian window (sigma 1.5), 'valid' filtering, C1 = (0.01*255)^2, C2 = (0.03*255)^2, mean of l * relu(cs).
eval_metrics.py's ``--test_y_channel`` first maps RGB to y = 0.257 r + 0.504 g + 0.098 b + 0.0625 (PSNR on that float y; SSIM takes
the one-channel branch)."""
from __future__ import annotations

import functools
import importlib
from dataclasses import dataclass
from typing import Callable

import torch

from . import lib as L
from . import ops
from .iqa import GpuMetric, find_first
from .iqa import as_nchw as _as_nchw            # the name other modules and tests know it by

FR, NETWORK, NR = "full-reference", "full-reference network", "no-reference"


@dataclass(frozen=True)
class MetricSpec:
    """One metric, declared once.  ``build(weights=W)`` (``build()`` for kind FR) makes the metric object, ``load(directory)`` its weights
    from a ``--metric_weights`` directory, ``probe(directory)`` says cheaply whether the main file is there (without one, ``load`` is the
    only check); ``patterns`` are the files ``load`` looks for and ``section`` is where INTEGRATION.md describes them."""
    name: str
    kind: str
    lower_better: bool
    build: Callable
    load: Callable | None = None
    probe: Callable | None = None
    patterns: tuple = ()
    section: str = ""


def _late(module: str, attr: str, **bound) -> Callable:
    """``dove_amd.<module>.<attr>`` (``attr`` may be dotted), imported when it is first called: this module loads without the metric
    modules."""
    def call(*args, **kwargs):
        return functools.reduce(getattr, attr.split("."), importlib.import_module(f"{__package__}.{module}"))(*args, **bound, **kwargs)
    return call


def _has(*patterns) -> Callable:
    return lambda directory: find_first(directory, patterns) is not None


_PERCEP = {"lpips": ("alexnet*.pth", "LPIPS_v0.1_alex*.pth"), "lpips-vgg": ("vgg16*.pth", "LPIPS_v0.1_vgg*.pth"),
           "dists": ("vgg16*.pth", "DISTS_weights*.pth")}
REGISTRY: dict = {s.name: s for s in (
    *(MetricSpec(n, FR, False, lambda n=n: FRMetric(n)) for n in ("psnr", "ssim")),
    *(MetricSpec(n, NETWORK, True, _late("percep", "PerceptualMetric", name=n), _late("percep", "load_metric_weights", name=n),
                 patterns=p, section="1h") for n, p in _PERCEP.items()),
    MetricSpec("niqe", NR, True, _late("niqe", "NiqeMetric"), _late("niqe", "load_model"),
               patterns=("niqe_modelparameters*.mat", "niqe*.npz"), section="1i"),
    MetricSpec("clipiqa", NR, False, _late("clipiqa", "ClipIqaMetric"), _late("clipiqa", "ClipIqaWeights.load"), _has("RN50*.pt", "RN50*.pth"),
               patterns=("RN50*.pt", "RN50*.pth", "clipiqa_text*.npz", "bpe_simple_vocab_16e6.txt*"), section="1j"),
    MetricSpec("musiq", NR, False, _late("musiq", "MusiqMetric"), _late("musiq", "MusiqWeights.load"), _has("musiq*.pth"),
               patterns=("musiq*.pth",), section="1k"),
)}


def metric_names(*kinds) -> tuple:
    """The registered names of the given kinds (all without any), in registry order."""
    return tuple(n for n, s in REGISTRY.items() if not kinds or s.kind in kinds)


FR_METRICS, NETWORK_METRICS, NR_METRICS = metric_names(FR), metric_names(NETWORK), metric_names(NR)      # as first registered


def name_list(names) -> str:
    """'a', 'a and b', 'a, b and c'."""
    names = list(names)
    return " and ".join(filter(None, (", ".join(names[:-1]), names[-1]))) if names else ""


def weights_help() -> str:
    """What a ``--metric_weights`` directory holds, for the command lines' help texts."""
    return "; ".join(f"{n}: {', '.join(s.patterns)} (INTEGRATION.md {s.section})" for n, s in REGISTRY.items() if s.kind != FR)


def _unsupported(name: str) -> NotImplementedError:
    return NotImplementedError(f"metric '{name}': dove_amd computes the full-reference metrics {', '.join(metric_names(FR))} on the GPU; "
                               f"the other pyiqa metrics ({', '.join(metric_names(NETWORK, NR))}, ...) need network weights and are "
                               "not provided - use pyiqa itself for them")


def fr_metrics(pred: torch.Tensor, ref: torch.Tensor, psnr: bool = True, ssim: bool = True, rgb_to_y: bool = False,
               layout: str = "auto"):
    """PSNR (dB) and SSIM per image -> (psnr[N], ssim[N]) as fp64 device tensors (None for a metric not asked for).

    ``pred`` / ``ref``: [N,C,H,W] tensors (any strides: crops and permuted views are read in place) or [F,H,W,3] uint8 frames
    (``layout='auto'`` takes a uint8 tensor whose last dim is 1 or 3 and whose dim 1 is not as frames; 'nchw' / 'nhwc' force it).
    dtypes: float32, bfloat16 (values in [0,1]) and uint8 (read as u/255), mixed freely."""
    if not (psnr or ssim):
        raise ValueError("fr_metrics: ask for psnr and/or ssim")
    p, r = _as_nchw(pred, layout), _as_nchw(ref, layout)
    if p.shape != r.shape:
        raise ValueError(f"fr_metrics: pred {tuple(pred.shape)} and ref {tuple(ref.shape)} differ in shape")
    flags = (L.METRIC_PSNR if psnr else 0) | (L.METRIC_SSIM if ssim else 0) | (L.METRIC_RGB_TO_Y if rgb_to_y else 0)
    out = ops.fr_metrics(p, r, flags)
    return (out[:, 0] if psnr else None), (out[:, 1] if ssim else None)


class FRMetric(GpuMetric):
    """pyiqa-style metric object for 'psnr' / 'ssim': ``metric(pred, ref)`` with [N,C,H,W] images in [0,1] -> [N] fp64 scores."""

    def __init__(self, name: str):
        def score(_, pred, ref):
            psnr, ssim = fr_metrics(pred, ref, psnr=name == "psnr", ssim=name == "ssim", layout="nchw")
            return psnr if name == "psnr" else ssim
        super().__init__(name, False, True, score)


def create_metric(name: str, weights=None, **kwargs):
    """``pyiqa.create_metric`` for the metrics of ``REGISTRY``, with pyiqa's default options: the full-reference ones as they are, the
    others given ``weights`` (what the spec's ``load`` returns).  Every metric object returns [N] fp64; ``lower_better`` says which way."""
    key = name.strip().lower()
    spec = REGISTRY.get(key)
    if weights is not None and (spec is None or spec.kind == FR):
        raise NotImplementedError(f"create_metric('{name}', weights=...): weights belong to {', '.join(metric_names(NETWORK, NR))}")
    if weights is None and (spec is None or spec.kind != FR):
        raise _unsupported(name)
    if kwargs:
        raise NotImplementedError(f"create_metric('{name}', {sorted(kwargs)}): only pyiqa's default options are implemented")
    return spec.build() if weights is None else spec.build(weights=weights)


def list_models(metric_mode=None):
    """pyiqa.list_models: the metrics this module provides without weights."""
    return list(metric_names(FR)) if metric_mode in (None, "FR") else []


def nr_clip_metrics(pred_u8: torch.Tensor, names, weights: dict) -> dict:
    """Per-clip no-reference metrics -> {metric: mean over frames}.  The reference hands these the predictions as they are: no
    match_resolution, no crop_border, no rgb_to_y.  ``pred_u8``: [F,H,W,3] uint8 frames (a host tensor is uploaded as uint8)."""
    vals = {}
    for n in names:
        if n not in metric_names(NR) or n not in weights:
            raise _unsupported(n)
        dev = pred_u8.device if pred_u8.is_cuda else torch.device("cuda")
        vals[n] = float(create_metric(n, weights=weights[n])(pred_u8.to(dev).permute(0, 3, 1, 2)).mean())
    return vals


def _crop_hw(t: torch.Tensor, th: int, tw: int, is_center: bool) -> torch.Tensor:
    """eval_metrics.py crop_img_center / crop_img_top_left on [F,H,W,C]."""
    h, w = t.shape[1], t.shape[2]
    top, left = (max((h - th) // 2, 0), max((w - tw) // 2, 0)) if is_center else (0, 0)
    return t[:, top:top + th, left:left + tw]


def match_resolution(gt: torch.Tensor, pred: torch.Tensor, is_center: bool = False, name: str | None = None):
    """eval_metrics.py match_resolution on [F,H,W,C] frames, as views: the common frame count, then a top-left (or centre) crop of
    both to the common H x W."""
    t = min(gt.shape[0], pred.shape[0])
    gt, pred = gt[:t], pred[:t]
    (h_g, w_g), (h_p, w_p) = gt.shape[1:3], pred.shape[1:3]
    th, tw = min(h_g, h_p), min(w_g, w_p)
    if (h_g != h_p or w_g != w_p) and name:
        how = "center" if is_center else "top-left"
        print(f"[{name}] Resolution mismatch detected: GT is ({h_g}, {w_g}), Pred is ({h_p}, {w_p}). Both GT and Pred were {how} "
              f"cropped to ({th}, {tw}).")
    return _crop_hw(gt, th, tw, is_center), _crop_hw(pred, th, tw, is_center)


def crop_border(t: torch.Tensor, crop: int) -> torch.Tensor:
    """eval_metrics.py crop_border (``img[:, :, crop:-crop, crop:-crop]``) on [F,H,W,C] frames; crop 0 leaves the frames as they are."""
    return t[:, crop:-crop, crop:-crop] if crop > 0 else t


def rgb_to_y(frames: torch.Tensor) -> torch.Tensor:
    """eval_metrics.py rgb_to_y on [F,H,W,3] frames (uint8 is read as u / 255) -> float32 [F,1,H,W]: 0.257 r + 0.504 g + 0.098 b + 0.0625."""
    v = frames.float() / 255.0 if frames.dtype == torch.uint8 else frames.float()
    return (0.257 * v[..., 0] + 0.504 * v[..., 1] + 0.098 * v[..., 2] + 0.0625)[:, None]


def clip_metrics(pred_u8: torch.Tensor, gt_u8: torch.Tensor, names, crop: int = 0, test_y_channel: bool = False,
                 is_center: bool = False, name: str | None = None, weights: dict | None = None) -> dict:
    """Per-clip metrics as eval_metrics.py computes them -> {metric: mean over frames of the per-frame value}: the full-reference ones,
    and the no-reference ones (given their weights in ``weights``) on the uncropped predictions (``crop`` and ``test_y_channel`` do not apply to them).

    ``pred_u8`` / ``gt_u8``: [F,H,W,3] uint8 frames (a host tensor is uploaded as uint8).  Steps of the reference: match_resolution
    (common frame count, top-left or centre crop to the common H x W), crop_border, optional rgb_to_y; all of them are views."""
    names = [n.strip().lower() for n in (names.split(",") if isinstance(names, str) else names)]
    weights = weights or {}
    for n in names:
        if n not in metric_names(FR) and n not in weights:
            raise _unsupported(n)
    dev = pred_u8.device if pred_u8.is_cuda else (gt_u8.device if gt_u8.is_cuda else torch.device("cuda"))
    pred_u8, gt_u8 = pred_u8.to(dev), gt_u8.to(dev)
    full = pred_u8                                              # the no-reference metrics see the predictions as they are
    gt, pred = match_resolution(gt_u8, pred_u8, is_center=is_center, name=name)
    gt, pred = crop_border(gt, crop), crop_border(pred, crop)
    vals = {}
    if "psnr" in names or "ssim" in names:
        vals["psnr"], vals["ssim"] = fr_metrics(pred, gt, psnr="psnr" in names, ssim="ssim" in names, rgb_to_y=test_y_channel,
                                                layout="nhwc")
    nr = nr_clip_metrics(full, [n for n in names if n in metric_names(NR)], weights)
    net = [n for n in names if n not in metric_names(FR, NR)]
    if net:
        # the reference hands the networks the same cropped (and, with --test_y_channel, one-channel) images as PSNR / SSIM;
        # ``weights`` of a user-supplied checkpoint make the metric, so ``names`` without them were refused above
        p, g = (rgb_to_y(pred), rgb_to_y(gt)) if test_y_channel else (pred.permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2))
        for n in net:
            vals[n] = create_metric(n, weights=weights[n])(p, g)
    return {n: nr[n] if n in nr else float(vals[n].mean()) for n in names}
