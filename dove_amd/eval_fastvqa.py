"""``python -m dove_amd.eval_fastvqa``: FasterVQA / FAST-VQA scores of SR results on the GPU (dove_amd.fastvqa, csrc/swin3d.hip), the
metric script that the reference's README lists as still to be added.

``--pred DIR --model FILE [--variant FasterVQA|FAST-VQA] [--seed 42] [--out DIR] [--rescale_mean M --rescale_std S]``.  Every entry of
``--pred`` is one clip, listed and read as ``eval_ewarp`` does (a PNG/JPG folder, an ``.npy`` clip, a ``.y4m`` file).  Writes
``metrics_fastervqa.json`` = {per_sample: {clip: {fastervqa: round(v, 4), fastervqa_raw: round(raw, 4)}}, average: {...}, count}:
``fastervqa`` is the sigmoid-rescaled score in (0, 1), higher is better, ``fastervqa_raw`` the network's output.  The network is restated
from memory and its agreement with the published checkpoints is unchecked; the rescaling constants are remembered
values too, hence the two override flags."""
from __future__ import annotations

import argparse
import os

from .iqa import list_clips, process_clips, summarize as _summarize  # noqa: F401  (list_clips: tests read it here)

METRIC, RAW = "fastervqa", "fastervqa_raw"
OUT_NAME = "metrics_fastervqa.json"


def summarize(results: dict) -> dict:
    """per_sample, the average of the (rounded) per-sample values, count."""
    return _summarize(results, (METRIC, RAW))


def make_score_fn(model: str, variant: str = "FasterVQA", seed: int = 42, rescale_mean=None, rescale_std=None):
    """``frames_u8 -> (raw, rescaled)`` with the weights of ``model``; raises what the command line refuses."""
    import torch

    from . import fastvqa
    cfg = fastvqa.preset(variant)
    if not torch.cuda.is_available():
        raise RuntimeError("dove_amd.eval_fastvqa runs the network on the GPU; no HIP device is visible")
    if not model or not os.path.isfile(model):
        raise FileNotFoundError(f"--model {model}: the {variant} checkpoint is not shipped; pass your own file")
    weights = fastvqa.VqaWeights.load(model, cfg)
    rescale = fastvqa.with_rescale(cfg, rescale_mean, rescale_std)
    return lambda frames: fastvqa.score_clip(frames, weights, seed=seed, rescale=rescale)


def process(pred_root: str, out_path: str, model: str = "", variant: str = "FasterVQA", seed: int = 42, score_fn=None, rescale_mean=None,
            rescale_std=None) -> dict:
    """``score_fn(frames_u8) -> (raw, rescaled)`` defaults to ``fastvqa.score_clip`` with the weights of ``model``."""
    if score_fn is None:
        score_fn = make_score_fn(model, variant, seed, rescale_mean, rescale_std)

    def clip(name, frames):
        raw, scaled = score_fn(frames)
        return {METRIC: round(float(scaled), 4), RAW: round(float(raw), 4)}

    return process_clips(pred_root, out_path, OUT_NAME, (METRIC, RAW), clip)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="FasterVQA / FAST-VQA of SR results on the GPU (dove_amd)")
    parser.add_argument("--pred", type=str, required=True, help="Folder of clips: PNG/JPG folders, .npy or .y4m files")
    parser.add_argument("--model", type=str, required=True, help="checkpoint in the published layout (not shipped)")
    parser.add_argument("--variant", type=str, default="FasterVQA", help="FasterVQA or FAST-VQA")
    parser.add_argument("--seed", type=int, default=42, help="seed of the fragment sampling")
    parser.add_argument("--out", type=str, default="", help="Path to save JSON output (as directory); default: --pred")
    parser.add_argument("--rescale_mean", type=float, default=None, help="mean of the sigmoid rescaling (default: the variant's remembered value)")
    parser.add_argument("--rescale_std", type=float, default=None, help="std of the sigmoid rescaling")
    return parser


def main(argv=None, score_fn=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.variant not in ("FasterVQA", "FAST-VQA"):
        parser.error(f"--variant {args.variant}: choose FasterVQA or FAST-VQA")
    if args.rescale_std is not None and not args.rescale_std > 0:
        parser.error("--rescale_std must be positive")
    return process(args.pred, args.out or args.pred, args.model, args.variant, args.seed, score_fn, args.rescale_mean, args.rescale_std)


if __name__ == "__main__":
    main()
