"""NIQE, the no-reference metric of the reference's evaluation step, on the GPU in fp64 (csrc/niqe.hip).

pyiqa's ``niqe`` with its defaults (a port of the MATLAB release): the luma round(255 (0.299 R + 0.587 G + 0.114 B)) is cropped to whole
96 x 96 blocks; at two scales (the second is MATLAB's antialiased bicubic half-scaling) the MSCN field (I - mu) / (sigma + 1) of a 7 x 7
Gaussian window (sigma 7/6, replicate padding) gives 18 AGGD features per block; the score is the Mahalanobis-like distance between the
Gaussian of the image's 36-vectors and a pristine model (mu, cov) that the USER supplies: pyiqa's ``niqe_modelparameters.mat``, or a
model fitted here from a folder of pristine images (``fit``, the MATLAB release's fitniqe).  Lower is better.

  - ``NiqeModel(mu, cov)`` / ``NiqeModel.load(path)``: ``.mat`` with ``mu_prisparam`` / ``cov_prisparam`` or ``.npz`` with ``mu`` / ``cov``;
  - ``features(images)`` -> (fp64 [N,B,36], block sharpness fp64 [N,B]);
  - ``niqe(model, images)`` -> fp64 [N];
  - ``fit(paths_or_tensors, sharpness=0.75)`` -> NiqeModel;
  - ``python -m dove_amd.niqe fit --images DIR --out model.npz [--sharpness T]``, ``python -m dove_amd.niqe score --model M --pred DIR``.

Images are [N,C,H,W] (C in {1, 3}; float32 / bfloat16 in [0,1] or uint8 read as u/255; any strides, read in place) or uint8 [F,H,W,3]
frames; H, W >= 96.  Everything on the device is fp64; the 36 x 36 pseudo-inverse runs in the library's host code."""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import iqa, ops
from .iqa import IMAGE_EXTENSIONS, GpuMetric, find_file, score_folder
from .iqa import list_images as _list_images
from .iqa import load_image as _load_image

FILE_PATTERNS = ("niqe_modelparameters*.mat", "niqe*.npz")       # searched in this order in a --metric_weights directory


class NiqeModel:
    """The pristine multivariate Gaussian: ``mu`` [36] and ``cov`` [36,36], float64 on the host."""

    def __init__(self, mu, cov):
        mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
        if mu.size != 36 or mu.squeeze().ndim != 1:
            raise ValueError(f"NiqeModel: mu must have 36 entries, got shape {mu.shape}")
        if cov.shape != (36, 36):
            raise ValueError(f"NiqeModel: cov must be [36,36], got shape {cov.shape}")
        self.mu, self.cov = np.ascontiguousarray(mu.reshape(36)), np.ascontiguousarray(cov)

    def to(self, device=None):                                   # the model lives on the host: nothing to move
        return self

    def save(self, path: str) -> None:
        np.savez(path, mu=self.mu, cov=self.cov)

    @classmethod
    def load(cls, path: str) -> "NiqeModel":
        """pyiqa's ``niqe_modelparameters*.mat`` (keys ``mu_prisparam`` [1,36], ``cov_prisparam`` [36,36]) or an ``.npz`` with ``mu``, ``cov``."""
        if path.lower().endswith(".mat"):
            from scipy.io import loadmat
            data, keys = loadmat(path), ("mu_prisparam", "cov_prisparam")
        else:
            data, keys = np.load(path), ("mu", "cov")
        for k in keys:
            if k not in data:
                raise KeyError(f"{path}: key '{k}' is missing (a NIQE model has {keys[0]} [36] and {keys[1]} [36,36])")
        mu, cov = np.asarray(data[keys[0]]), np.asarray(data[keys[1]])
        if mu.size != 36 or mu.squeeze().ndim != 1:
            raise ValueError(f"{path}: key '{keys[0]}' has shape {mu.shape}, expected 36 entries")
        if cov.shape != (36, 36):
            raise ValueError(f"{path}: key '{keys[1]}' has shape {cov.shape}, expected (36, 36)")
        return cls(mu, cov)


def find_model_file(directory: str) -> str:
    return find_file(directory, FILE_PATTERNS)


def load_model(directory: str) -> NiqeModel:
    """The NIQE model of a ``--metric_weights`` directory: ``niqe_modelparameters*.mat``, then ``niqe*.npz``."""
    return NiqeModel.load(find_model_file(directory))


def _images(x: torch.Tensor, device=None) -> torch.Tensor:
    return iqa.images(x, "niqe", (96, 96), device=device)           # one 96 x 96 block at least; every dtype is read as it is


def features(images: torch.Tensor, device=None):
    """-> (features fp64 [N,B,36], sharpness fp64 [N,B]) on the device; B = (H // 96) * (W // 96) blocks, row-major.  The 18 features of a
    block at scale 1, then the 18 of the same block at half scale; sharpness is the block's mean local deviation at scale 1."""
    return ops.niqe_features(_images(images, device))


def niqe(model: NiqeModel, images: torch.Tensor, device=None) -> torch.Tensor:
    """NIQE of every image against ``model`` -> fp64 [N] on the images' device.  An image with fewer than two NaN-free blocks scores NaN."""
    if not isinstance(model, NiqeModel):
        raise TypeError(f"niqe: model must be a NiqeModel, got {type(model).__name__}")
    x = _images(images, device)
    feats, _ = ops.niqe_features(x)
    mu, cov, _ = ops.niqe_stats(feats)
    mu, cov = mu.cpu().numpy(), cov.cpu().numpy()
    out = [ops.niqe_distance(model.mu, model.cov, mu[i], cov[i]) for i in range(mu.shape[0])]
    return torch.tensor(out, dtype=torch.float64, device=x.device)


def fit(paths_or_tensors, sharpness: float = 0.75, device=None) -> NiqeModel:
    """The pristine model of a set of images (paths, or tensors as ``features`` takes them; sizes may differ): of every image the blocks
    whose sharpness exceeds ``sharpness`` x that image's largest are kept; mu and cov (divisor n-1) over the kept NaN-free blocks."""
    kept = []
    for item in paths_or_tensors:
        img = _load_image(item) if isinstance(item, (str, os.PathLike)) else item
        f, s = features(img, device)
        f, s = f.cpu().numpy(), s.cpu().numpy()
        for fi, si in zip(f, s):                                 # a tensor may hold several images: each has its own maximum
            rows = fi[si > sharpness * si.max()]
            kept.append(rows[~np.isnan(rows).any(axis=1)])
    rows = np.concatenate(kept) if kept else np.zeros((0, 36))
    if rows.shape[0] < 2:
        raise ValueError(f"niqe.fit: {rows.shape[0]} usable blocks; a covariance needs at least two")
    return NiqeModel(rows.mean(axis=0), np.cov(rows, rowvar=False))


class NiqeMetric(GpuMetric):
    """pyiqa-style metric object: ``metric(pred)`` with [N,C,H,W] images in [0,1] (host or device) -> [N] fp64 NIQE scores."""

    def __init__(self, weights: NiqeModel):
        super().__init__("niqe", True, False, niqe, weights, NiqeModel)


def main(argv=None):
    ap = argparse.ArgumentParser(description="NIQE on the GPU (dove_amd): fit a pristine model, or score images against one")
    sub = ap.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("fit", help="fit a pristine model from a folder of images")
    f.add_argument("--images", required=True, help="folder of pristine images (png / jpg / bmp)")
    f.add_argument("--out", required=True, help="model file to write (.npz with mu, cov)")
    f.add_argument("--sharpness", type=float, default=0.75, help="keep the blocks sharper than this fraction of the image's sharpest")
    s = sub.add_parser("score", help="score every image of a folder against a model")
    s.add_argument("--model", required=True, help="niqe_modelparameters.mat or a fitted .npz")
    s.add_argument("--pred", required=True, help="folder of images")
    args = ap.parse_args(argv)
    if args.cmd == "fit":
        paths = _list_images(args.images)
        if not paths:
            raise FileNotFoundError(f"no images ({', '.join(IMAGE_EXTENSIONS)}) in {args.images}")
        model = fit(paths, sharpness=args.sharpness)
        model.save(args.out)
        print(f"fitted on {len(paths)} images -> {args.out}")
        return model
    return score_folder(args, lambda a: NiqeModel.load(a.model), niqe)


if __name__ == "__main__":
    main()
