"""What every image-quality metric shares, written once: image intake, the walk over groups of frames, the search for files in a
``--metric_weights`` directory, the state-dict loader, the pyiqa-style metric object, the ``score`` command-line loop and the per-clip
evaluation loop of the video metrics' commands.

This module imports none of the metric modules (metrics, percep, niqe, clipiqa, musiq, flow, fastvqa, maniqa); they import it.  A metric module
keeps what is its own: the network walk, its ``group_size`` formula, its ``COUNTERS``, the shapes and the packing of its checkpoint.  What
the weights classes share is in ``netweights``.  ``metrics.REGISTRY`` declares the metrics."""
from __future__ import annotations

import glob
import json
import math
import os

import numpy as np
import torch

# Live fp32 activations of one group of frames, the same for every network metric: each module's ``group_size`` says how many frames that is
# (percep: four 720p pairs through VGG16; clipiqa: 36 frames of 720 x 1280; musiq: 25; maniqa: 2).
ACTIVATION_BUDGET = 4 << 30
IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp")
FLOAT32_DTYPES = (torch.uint8, torch.float32)       # what the fp32 networks read in place; every other dtype is cast to float32


# ------------------------------------------------------------------ images ------------------------------------------------------------------
def as_nchw(t: torch.Tensor, layout: str) -> torch.Tensor:
    if t.dim() != 4:
        raise ValueError(f"expected a 4-D image batch, got shape {tuple(t.shape)}")
    if layout == "auto":
        layout = "nhwc" if t.dtype == torch.uint8 and t.shape[3] in (1, 3) and t.shape[1] not in (1, 3) else "nchw"
    if layout == "nhwc":
        return t.permute(0, 3, 1, 2)
    if layout != "nchw":
        raise ValueError(f"layout must be 'auto', 'nchw' or 'nhwc', got {layout!r}")
    return t


def images(x: torch.Tensor, name: str, min_hw=(1, 1), dtypes=None, device=None) -> torch.Tensor:
    """The images of metric ``name`` as an [N,1|3,H,W] view on the device: a [C,H,W] image gets its batch axis, uint8 [F,H,W,3] frames are
    permuted, H and W are checked against ``min_hw``, a host tensor is uploaded (to ``device``, else the current HIP device) and a dtype
    outside ``dtypes`` is cast to float32 (``None``: every dtype stays)."""
    if x.dim() == 3:                                             # one [C,H,W] image
        x = x[None]
    shape, x = tuple(x.shape), as_nchw(x, "auto")
    if x.shape[1] not in (1, 3):
        raise ValueError(f"{name}: images must have 1 or 3 channels, got shape {shape}")
    if x.shape[2] < min_hw[0] or x.shape[3] < min_hw[1]:
        raise ValueError(f"{name}: images of {x.shape[2]} x {x.shape[3]} are too small: H and W must be at least {min_hw[0]} x {min_hw[1]}; "
                         f"the minimum side is {min(min_hw)}")
    if not x.is_cuda:
        x = x.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return x if dtypes is None or x.dtype in dtypes else x.float()


def for_groups(n: int, group, default_group: int, counters: dict, device, body) -> None:
    """``body(i, j)`` for every group [i, j) of ``n`` frames, ``group`` frames each (``None``: ``default_group``, the module's
    ``group_size``), with ``device`` current; ``counters['groups']`` counts the groups walked."""
    g = default_group if group is None else max(1, int(group))
    with torch.cuda.device(device):
        for i in range(0, n, g):
            body(i, min(i + g, n))
            counters["groups"] += 1


# ------------------------------------------------------------------- files -------------------------------------------------------------------
def find_first(directory: str, patterns):
    """The first file (sorted) of the first of ``patterns`` that ``directory`` has one of, or None."""
    for pattern in ((patterns,) if isinstance(patterns, str) else patterns):
        hits = sorted(glob.glob(os.path.join(directory, pattern))) if directory else []
        if hits:
            return hits[0]
    return None


def find_file(directory: str, patterns) -> str:
    """``find_first``, or FileNotFoundError naming the patterns and the directory."""
    path = find_first(directory, patterns)
    if path is None:
        raise FileNotFoundError(f"no file matching {' or '.join((patterns,) if isinstance(patterns, str) else patterns)} in {directory}")
    return path


def load_state_dict(path: str, unwrap=("state_dict", "params"), torchscript: bool = False) -> dict:
    """The state dict of a checkpoint file, on the host; a top-level ``unwrap`` key that holds a dict is unwrapped.  ``torchscript``: a
    file that is no plain state dict (OpenAI's RN50.pt is a TorchScript archive, which ``weights_only`` refuses) is opened as an archive."""
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:
        if not torchscript:
            raise
        sd = None
    if torchscript and not isinstance(sd, dict):
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    for key in unwrap:
        if isinstance(sd, dict) and isinstance(sd.get(key), dict):
            sd = sd[key]
    return sd


# ------------------------------------------------------------------ metric ------------------------------------------------------------------
class GpuMetric(torch.nn.Module):
    """pyiqa-style metric object: ``metric(pred)`` or ``metric(pred, ref)`` with [N,C,H,W] images in [0,1] (or one [C,H,W] image) -> [N]
    fp64 scores, by ``score(weights, pred, ref)`` of a full-reference metric and ``score(weights, pred)`` of a no-reference one (which
    ignores ``ref``, as pyiqa's do).

    Like pyiqa's InferenceModel, the inputs are moved to the metric's device first: the device given to ``.to()``, or the current HIP
    device while the metric has not been moved to one (there is no CPU path).  The reference's in-process loop passes host frames.
    ``weights_type``: what ``weights`` must be an instance of."""

    def __init__(self, name: str, lower_better: bool, full_reference: bool, score, weights=None, weights_type=None):
        super().__init__()
        if weights_type is not None and not isinstance(weights, weights_type):
            raise TypeError(f"create_metric('{name}'): weights must be a {weights_type.__module__}.{weights_type.__name__}")
        self.metric_name, self.lower_better, self.full_reference, self.score, self.weights = name, lower_better, full_reference, score, weights
        self.register_buffer("_anchor", torch.empty(0), persistent=False)   # follows .to(device)

    @property
    def device(self) -> torch.device:
        return self._anchor.device if self._anchor.is_cuda else torch.device("cuda", torch.cuda.current_device())

    def forward(self, pred: torch.Tensor, ref: torch.Tensor | None = None) -> torch.Tensor:
        batch = (pred, ref) if self.full_reference else (pred,)
        if pred.dim() == 3:                                         # pyiqa accepts a single [C,H,W] image too
            batch = [t[None] for t in batch]
        dev = self.device
        return self.score(self.weights, *(t.to(dev) for t in batch))


# ------------------------------------------------------------- the score tools -------------------------------------------------------------
def list_images(directory: str):
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.lower().endswith(IMAGE_EXTENSIONS))


def load_image(path: str) -> torch.Tensor:
    from PIL import Image
    return torch.from_numpy(np.asarray(Image.open(path).convert("RGB")).copy())[None]


def score_folder(args, load_weights, score_fn) -> dict:
    """The ``score`` subcommand of a metric module: ``load_weights(args)``, then ``score_fn(weights, image)`` of every image of the
    folder ``args.pred``; prints each value and the average -> {file name: value}."""
    weights = load_weights(args)
    scores = {os.path.basename(p): float(score_fn(weights, load_image(p))[0]) for p in list_images(args.pred)}
    for name, v in scores.items():
        print(f"{name}: {v:.4f}")
    if scores:
        print(f"average: {float(np.mean(list(scores.values()))):.4f}")
    return scores


def list_clips(pred_root: str) -> dict:
    """{os.path.splitext stem: path} of the folders, ``.npy`` and ``.y4m`` entries of ``pred_root``."""
    clips = {}
    for item in sorted(os.listdir(pred_root)):
        path = os.path.join(pred_root, item)
        if os.path.isdir(path) or item.lower().endswith((".npy", ".y4m")):
            clips[os.path.splitext(item)[0]] = path
    return clips


def summarize(results: dict, keys) -> dict:
    """per_sample, per key the average of the (rounded) per-sample values that are numbers, count."""
    average = {}
    for key in keys:
        vals = [v[key] for v in results.values() if not math.isnan(v[key])]
        if results:
            average[key] = round(sum(vals) / len(vals), 4) if vals else float("nan")
    return {"per_sample": results, "average": average, "count": len(results)}


def process_clips(pred_root: str, out_path: str, out_name: str, keys, clip_fn) -> dict:
    """The loop of a per-clip evaluation command: every clip of ``pred_root`` is read by ``prepost.load_frames``; ``clip_fn(name, frames)``
    gives its rounded {key: value} (``None``: the clip is left out; an exception is reported and the clip left out); the summary is
    printed and written to ``out_path/out_name``."""
    from . import prepost
    results = {}
    for name, path in list_clips(pred_root).items():
        try:
            r = clip_fn(name, prepost.load_frames(path))
            if r is not None:
                results[name] = r
        except Exception as e:
            print(f"Error processing {name}: {e}")
    output = summarize(results, keys)
    print(f"\nProcessed {output['count']} samples.")
    print(f"Average score: {output['average']}")
    os.makedirs(out_path, exist_ok=True)
    path = os.path.join(out_path, out_name)
    with open(path, "w") as f:
        json.dump(output, f, indent=2)
    print(f"Results saved to: {path}")
    return output
