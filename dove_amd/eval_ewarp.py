"""``python -m dove_amd.eval_ewarp``: the reference's ``finetune/scripts/eval_ewarp.py`` with the flow (RAFT) and the warping error
computed on the GPU (dove_amd.flow, csrc/flow.hip).

Same flags (``--pred --metric --model --small --mixed_precision --alternate_corr --out``) plus ``--iters``.  ``--small`` is refused (the
basic model only); ``--mixed_precision`` and ``--alternate_corr`` are accepted and change nothing: the flow is fp32 on the all-pairs
volume.  Every entry of ``--pred`` is one clip, read by ``prepost.load_frames`` (a PNG/JPG folder, an ``.npy`` clip, a ``.y4m`` file); the
reference's detour through a temporary lossless mp4 is not reproduced.  Writes ``metrics_ewarp.json`` = {per_sample: {clip:
{warping_error: round(v, 4)}}, average: {warping_error: ...}, count}, the shape the reference's script gives it.  The metric itself is
defined in dove_amd.flow (the reference does not ship its ``ewarp`` module)."""
from __future__ import annotations

import argparse
import os

from .iqa import list_clips, process_clips, summarize as _summarize  # noqa: F401  (list_clips: eval_fastvqa and tests read it here)

METRIC = "warping_error"
OUT_NAME = "metrics_ewarp.json"


def summarize(results: dict) -> dict:
    """per_sample, the average of the (rounded) per-sample values that are numbers, count."""
    return _summarize(results, (METRIC,))


def process(pred_root: str, out_path: str, model: str, iters: int = 20, clip_error_fn=None) -> dict:
    """``clip_error_fn(frames_u8) -> dict`` defaults to ``flow.warping_error`` with the weights of ``model``."""
    if clip_error_fn is None:
        import torch

        from . import flow
        if not torch.cuda.is_available():
            raise RuntimeError("dove_amd.eval_ewarp computes the flow on the GPU; no HIP device is visible")
        if not os.path.isfile(model):
            raise FileNotFoundError(f"--model {model}: the RAFT checkpoint (raft-things.pth) is not shipped; pass your own file")
        weights = flow.RaftWeights.load(model)
        clip_error_fn = lambda frames: flow.warping_error(frames, weights, iters)

    def clip(name, frames):
        if frames.shape[0] < 2:
            print(f"Skipping {name}: a clip needs at least 2 frames.")
            return None
        r = clip_error_fn(frames)
        if r.get("pairs_without_valid_pixels"):
            print(f"{name}: {r['pairs_without_valid_pixels']} of {r['pairs']} pairs have no valid pixel")
        return {METRIC: round(r[METRIC], 4)}

    return process_clips(pred_root, out_path, OUT_NAME, (METRIC,), clip)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="E*warp (warping error under RAFT flow) of SR results on the GPU (dove_amd)")
    parser.add_argument("--pred", type=str, required=True, help="Folder of clips: PNG/JPG folders, .npy or .y4m files")
    parser.add_argument("--metric", type=str, default=METRIC, help="warping_error")
    parser.add_argument("--model", type=str, default="finetune/scripts/models/raft-things.pth", help="RAFT checkpoint (not shipped)")
    parser.add_argument("--small", action="store_true", help="refused: the small model is not built")
    parser.add_argument("--mixed_precision", action="store_true", help="accepted; changes nothing: the flow is fp32")
    parser.add_argument("--alternate_corr", action="store_true", help="accepted; changes nothing: the all-pairs volume is used")
    parser.add_argument("--out", type=str, default="", help="Path to save JSON output (as directory); default: --pred")
    parser.add_argument("--iters", type=int, default=20, help="RAFT update rounds")
    return parser


def main(argv=None, clip_error_fn=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.small:
        parser.error("--small: the small RAFT model is not built; dove_amd.flow runs the basic model only")
    if args.metric != METRIC:
        parser.error(f"--metric {args.metric}: only {METRIC} is computed here")
    if args.iters < 1:
        parser.error("--iters must be at least 1")
    if args.mixed_precision:
        print("--mixed_precision changes nothing: the flow is computed in fp32")
    if args.alternate_corr:
        print("--alternate_corr changes nothing: the all-pairs correlation volume is used")
    return process(args.pred, args.out or args.pred, args.model, args.iters, clip_error_fn)


if __name__ == "__main__":
    main()
