"""Full-reference metrics of the reference's evaluation step on the GPU: PSNR and SSIM (csrc/metrics.hip, ``dove_fr_metrics``).

Three surfaces:
  - ``fr_metrics(pred, ref, psnr=True, ssim=True, rgb_to_y=False)``: per-image fp64 values of a batch of strided views;
  - ``create_metric(name)``: pyiqa's ``create_metric`` surface for 'psnr' and 'ssim', so the reference's metric code runs with
    ``import dove_amd.metrics as pyiqa``; ``create_metric(name, weights=W)`` gives 'lpips', 'lpips-vgg' and 'dists' from user-supplied
    checkpoints (dove_amd.percep) and the no-reference 'niqe' from a user-supplied pristine model (dove_amd.niqe.NiqeModel) and 'clipiqa'
    from a user-supplied CLIP RN50 checkpoint (dove_amd.clipiqa.ClipIqaWeights) and 'musiq' from a user-supplied MUSIQ checkpoint
    (dove_amd.musiq.MusiqWeights), all called as ``metric(pred)``; any other name, or one of these without weights, raises
    ``NotImplementedError``;
  - ``clip_metrics(pred_u8, gt_u8, names, crop, test_y_channel, is_center)``: the per-clip logic of eval_metrics.py (match_resolution,
    crop_border, rgb_to_y, mean over frames), as views on the device; ``nr_clip_metrics(pred_u8, names, weights)`` is its ground-truth-free
    half (the no-reference metrics on the predictions as they are).

Definitions (pyiqa's 'psnr' / 'ssim' defaults, INTEGRATION.md 'Metrics'): values in [0,1], uint8 read as u/255.
PSNR = 10 log10(1 / (mse + 1e-8)) over C, H, W.  SSIM on the luma Y = round(255 (0.299 R + 0.587 G + 0.114 B)) (round(255 v) for one
channel), 11x11 Gaussian window (sigma 1.5), 'valid' filtering, C1 = (0.01*255)^2, C2 = (0.03*255)^2, mean of l * relu(cs).
eval_metrics.py's ``--test_y_channel`` first maps RGB to y = 0.257 r + 0.504 g + 0.098 b + 0.0625 (PSNR on that float y; SSIM takes
the one-channel branch)."""
from __future__ import annotations

import torch

from . import lib as L
from . import ops

FR_METRICS = ("psnr", "ssim")
NETWORK_METRICS = ("lpips", "lpips-vgg", "dists")       # computed by dove_amd.percep when the caller passes weights
NR_METRICS = ("niqe", "clipiqa", "musiq")               # no-reference: dove_amd.niqe (NiqeModel), .clipiqa (ClipIqaWeights), .musiq (MusiqWeights)


def _unsupported(name: str) -> NotImplementedError:
    return NotImplementedError(f"metric '{name}': dove_amd computes the full-reference metrics {', '.join(FR_METRICS)} on the GPU; "
                               "the other pyiqa metrics (lpips, dists, clipiqa, musiq, maniqa, niqe, ...) need network weights and are "
                               "not provided - use pyiqa itself for them")


def _as_nchw(t: torch.Tensor, layout: str) -> torch.Tensor:
    if t.dim() != 4:
        raise ValueError(f"expected a 4-D image batch, got shape {tuple(t.shape)}")
    if layout == "auto":
        layout = "nhwc" if t.dtype == torch.uint8 and t.shape[3] in (1, 3) and t.shape[1] not in (1, 3) else "nchw"
    if layout == "nhwc":
        return t.permute(0, 3, 1, 2)
    if layout != "nchw":
        raise ValueError(f"layout must be 'auto', 'nchw' or 'nhwc', got {layout!r}")
    return t


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


class FRMetric(torch.nn.Module):
    """pyiqa-style metric object for 'psnr' / 'ssim': ``metric(pred, ref)`` with [N,C,H,W] images in [0,1] -> [N] fp64 scores.

    Like pyiqa's InferenceModel, the inputs are moved to the metric's device first: the device given to ``.to()``, or the current HIP
    device while the metric has not been moved to one (there is no CPU path).  The reference's in-process loop passes host frames."""

    lower_better = False

    def __init__(self, name: str):
        super().__init__()
        self.metric_name = name
        self.register_buffer("_anchor", torch.empty(0), persistent=False)   # follows .to(device)

    @property
    def device(self) -> torch.device:
        return self._anchor.device if self._anchor.is_cuda else torch.device("cuda", torch.cuda.current_device())

    def forward(self, pred: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
        if pred.dim() == 3:                                         # pyiqa accepts a single [C,H,W] image too
            pred, ref = pred[None], ref[None]
        dev = self.device
        pred, ref = pred.to(dev), ref.to(dev)
        psnr, ssim = fr_metrics(pred, ref, psnr=self.metric_name == "psnr", ssim=self.metric_name == "ssim", layout="nchw")
        return psnr if self.metric_name == "psnr" else ssim


def create_metric(name: str, weights=None, **kwargs):
    """``pyiqa.create_metric`` for the full-reference metrics computed here: 'psnr' and 'ssim' with pyiqa's default options, and, given
    ``weights`` (percep.LpipsWeights / percep.DistsWeights), 'lpips', 'lpips-vgg' and 'dists' (lower is better, [N] fp64); with
    ``weights`` a niqe.NiqeModel, the no-reference 'niqe' (``metric(pred)``, lower is better, [N] fp64); with clipiqa.ClipIqaWeights, the
    no-reference 'clipiqa', and with musiq.MusiqWeights the no-reference 'musiq' (``metric(pred)``, higher is better, [N] fp64)."""
    key = name.strip().lower()
    if weights is not None:
        if key not in NETWORK_METRICS + NR_METRICS:
            raise NotImplementedError(f"create_metric('{name}', weights=...): weights belong to {', '.join(NETWORK_METRICS + NR_METRICS)}")
        if kwargs:
            raise NotImplementedError(f"create_metric('{name}', {sorted(kwargs)}): only pyiqa's default options are implemented")
        if key == "clipiqa":
            from . import clipiqa
            return clipiqa.ClipIqaMetric(weights)
        if key == "musiq":
            from . import musiq
            return musiq.MusiqMetric(weights)
        if key in NR_METRICS:
            from . import niqe
            return niqe.NiqeMetric(weights)
        from . import percep
        return percep.PerceptualMetric(key, weights)
    if key not in FR_METRICS:
        raise _unsupported(name)
    if kwargs:
        raise NotImplementedError(f"create_metric('{name}', {sorted(kwargs)}): only pyiqa's default options are implemented")
    return FRMetric(key)


def list_models(metric_mode=None):
    """pyiqa.list_models: the metrics this module provides."""
    return list(FR_METRICS) if metric_mode in (None, "FR") else []


def nr_clip_metrics(pred_u8: torch.Tensor, names, weights: dict) -> dict:
    """Per-clip no-reference metrics -> {metric: mean over frames}.  The reference hands these the predictions as they are: no
    match_resolution, no crop_border, no rgb_to_y.  ``pred_u8``: [F,H,W,3] uint8 frames (a host tensor is uploaded as uint8)."""
    vals = {}
    for n in names:
        if n not in NR_METRICS or n not in weights:
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
    and 'niqe' / 'clipiqa' / 'musiq' (given their weights in ``weights``) on the uncropped predictions (``crop`` and ``test_y_channel`` do not apply to them).

    ``pred_u8`` / ``gt_u8``: [F,H,W,3] uint8 frames (a host tensor is uploaded as uint8).  Steps of the reference: match_resolution
    (common frame count, top-left or centre crop to the common H x W), crop_border, optional rgb_to_y; all of them are views."""
    names = [n.strip().lower() for n in (names.split(",") if isinstance(names, str) else names)]
    weights = weights or {}
    for n in names:
        if n not in FR_METRICS and n not in weights:
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
    nr = nr_clip_metrics(full, [n for n in names if n in NR_METRICS], weights)
    net = [n for n in names if n not in FR_METRICS + NR_METRICS]
    if net:
        # the reference hands the networks the same cropped (and, with --test_y_channel, one-channel) images as PSNR / SSIM;
        # ``weights`` of a user-supplied checkpoint make the metric, so ``names`` without them were refused above
        p, g = (rgb_to_y(pred), rgb_to_y(gt)) if test_y_channel else (pred.permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2))
        for n in net:
            vals[n] = create_metric(n, weights=weights[n])(p, g)
    return {n: nr[n] if n in nr else float(vals[n].mean()) for n in names}
