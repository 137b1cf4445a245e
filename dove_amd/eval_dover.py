"""``python -m dove_amd.eval_dover``: DOVER scores of SR results on the GPU (dove_amd.dover, csrc/convnext3d.hip, csrc/swin3d.hip), the
reference's ``finetune/scripts/eval_dover.py`` step.

``--pred DIR --model FILE [--seed 42] [--out DIR] [--resize antialias|plain] [--technical_mean M --technical_std S --aesthetic_mean M
--aesthetic_std S]``.  Every entry of ``--pred`` is one clip, listed and read as ``eval_fastvqa`` does (a PNG/JPG folder, an ``.npy`` clip, a
``.y4m`` file).  Writes ``metrics_dover.json`` = {per_sample: {clip: {dover, dover_technical, dover_aesthetic, dover_technical_raw,
dover_aesthetic_raw}}, average: {...}, count}, every value rounded to 4 places: ``dover`` is the fused score in (0, 1), higher is better.
The reference converts every folder to a lossless mp4 first and assigns ``dover_results[i - 1]`` to clip ``i``; neither is reproduced:
frames are read directly and each clip gets its own score (the average is the same).  The network is restated from memory and its agreement
with the published checkpoint is unchecked; the fusion constants are remembered values too, hence the override flags."""
from __future__ import annotations

import argparse
import dataclasses
import os

from .iqa import list_clips, process_clips, summarize as _summarize  # noqa: F401  (list_clips: tests read it here)

KEYS = ("dover", "dover_technical", "dover_aesthetic", "dover_technical_raw", "dover_aesthetic_raw")
_FROM = ("overall", "technical", "aesthetic", "technical_raw", "aesthetic_raw")
OUT_NAME = "metrics_dover.json"


def summarize(results: dict) -> dict:
    """per_sample, the average of the (rounded) per-sample values, count."""
    return _summarize(results, KEYS)


def make_score_fn(model: str, seed: int = 42, resize: str = "antialias", rescale=None):
    """``frames_u8 -> dover.score_clip's dict`` with the weights of ``model``; raises what the command line refuses."""
    import torch

    from . import dover
    cfg = dataclasses.replace(dover.DEFAULT, resize=resize)
    if not torch.cuda.is_available():
        raise RuntimeError("dove_amd.eval_dover runs the networks on the GPU; no HIP device is visible")
    if not model or not os.path.isfile(model):
        raise FileNotFoundError(f"--model {model}: the DOVER checkpoint is not shipped; pass your own file")
    weights = dover.DoverWeights.load(model, cfg)
    return lambda frames: dover.score_clip(frames, weights, seed=seed, rescale=rescale)


def process(pred_root: str, out_path: str, model: str = "", seed: int = 42, score_fn=None, resize: str = "antialias", rescale=None) -> dict:
    """``score_fn(frames_u8) -> {overall, technical, aesthetic, technical_raw, aesthetic_raw}`` defaults to ``dover.score_clip`` with the
    weights of ``model``."""
    if score_fn is None:
        score_fn = make_score_fn(model, seed, resize, rescale)

    def clip(name, frames):
        s = score_fn(frames)
        return {k: round(float(s[f]), 4) for k, f in zip(KEYS, _FROM)}

    return process_clips(pred_root, out_path, OUT_NAME, KEYS, clip)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="DOVER of SR results on the GPU (dove_amd)")
    parser.add_argument("--pred", type=str, required=True, help="Folder of clips: PNG/JPG folders, .npy or .y4m files")
    parser.add_argument("--model", type=str, required=True, help="checkpoint in the published layout (not shipped)")
    parser.add_argument("--seed", type=int, default=42, help="seed of the temporal and fragment sampling")
    parser.add_argument("--out", type=str, default="", help="Path to save JSON output (as directory); default: --pred")
    parser.add_argument("--resize", type=str, default="antialias", help="the aesthetic view's bilinear resize: antialias or plain")
    for branch in ("technical", "aesthetic"):
        parser.add_argument(f"--{branch}_mean", type=float, default=None, help=f"mean of the {branch} rescaling (default: the remembered value)")
        parser.add_argument(f"--{branch}_std", type=float, default=None, help=f"std of the {branch} rescaling")
    return parser


def main(argv=None, score_fn=None):
    from .dover import with_rescale
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.resize not in ("antialias", "plain"):
        parser.error(f"--resize {args.resize}: choose antialias or plain")
    for name in ("technical_std", "aesthetic_std"):
        if getattr(args, name) is not None and not getattr(args, name) > 0:
            parser.error(f"--{name} must be positive")
    rescale = with_rescale(args.technical_mean, args.technical_std, args.aesthetic_mean, args.aesthetic_std)
    return process(args.pred, args.out or args.pred, args.model, args.seed, score_fn, args.resize, rescale)


if __name__ == "__main__":
    main()
