"""``python -m dove_amd.eval_metrics``: the reference's ``eval_metrics.py`` (the second command of its ``inference.sh``) with PSNR and
SSIM computed on the GPU (dove_amd.metrics, csrc/metrics.hip).

Same flags (``--gt --pred --out --metrics --batch_mode --crop --test_y_channel --is_center``), the same pairing of predictions and
ground truth by ``os.path.splitext`` stem, the same per-clip steps (match_resolution, crop_border, rgb_to_y), the same printout and the
same JSON (``metrics_<names>.json``: per_sample {clip: {metric: round(value, 4)}}, average of the rounded values, count).
Inputs are PNG/JPG folders, single images, ``.npy`` clips (uint8 [F,H,W,3]) and ``.y4m`` files (YUV4MPEG2, read as bt601 with the
stream's range tag; dove_amd.y4m); mp4 decoding is not provided.  ``--metrics``
defaults to ``psnr,ssim`` (the reference's default also lists clipiqa, which needs ``--metric_weights``).  ``--metric_weights DIR`` adds
the metrics that ``dove_amd.metrics.REGISTRY`` declares with weights, the network and the no-reference ones, each from its files in that
directory (``--help`` lists them with their INTEGRATION.md sections); a file that is absent raises FileNotFoundError.
Without ``--gt`` the no-reference metrics are computed on the predictions alone and
written to the same JSON, as in the reference (its ``--gt`` is "optional for NR-IQA"); a clip is skipped only when no no-reference metric
was asked for.  Without the flag a metric other than psnr / ssim fails to initialise with a message, as a pyiqa metric that
cannot be created does in the reference."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np
import torch

from . import metrics as M
from . import prepost


def load_sequence(path: str) -> torch.Tensor:
    """A PNG/JPG folder, a single image (one frame), an ``.npy`` clip or a ``.y4m`` file -> uint8 [F,H,W,3] (host)."""
    if os.path.isfile(path) and path.lower().endswith((".png", ".jpg", ".jpeg")):
        from PIL import Image
        return torch.from_numpy(np.asarray(Image.open(path).convert("RGB")).copy())[None]
    return prepost.load_frames(path)


def pair_files(gt_root: str, pred_root: str):
    """eval_metrics.py's pairing -> (gt_files or None, pred_files): {os.path.splitext stem: path}."""
    has_gt = bool(gt_root and os.path.exists(gt_root))
    gt_files = {os.path.splitext(f)[0]: os.path.join(gt_root, f) for f in os.listdir(gt_root)} if has_gt else None
    pred_files = {os.path.splitext(f)[0]: os.path.join(pred_root, f) for f in os.listdir(pred_root)}
    return gt_files, pred_files


def output_name(metrics) -> str:
    """``metrics_<m1>_<m2>...json`` (eval_metrics.py and inference_script.py name the file the same way)."""
    return "metrics_" + "_".join(metrics) + ".json"


def summarize(results: dict, metrics) -> dict:
    """The JSON the reference writes: per_sample, the average of the (rounded) per-sample values per metric, count.  A metric that
    could not be initialised has no values and no average (the reference would write NaN for it)."""
    aggregate = {m: [] for m in metrics}
    for scores in results.values():
        for k, v in scores.items():
            aggregate[k].append(v)
    count = len(results)
    overall = {k: round(float(np.mean(v)), 4) for k, v in aggregate.items() if v} if count > 0 else {}
    return {"per_sample": results, "average": overall, "count": count}


def init_models(metrics, device=None, weights=None):
    models = {}
    for name in metrics:
        try:
            models[name] = M.create_metric(name, **({"weights": weights[name]} if weights and name in weights else {})).to(device).eval()
        except Exception as e:
            print(f"Failed to initialize metric '{name}': {e}")
    return models


def load_weights(metrics, directory):
    """Weights of the registered metrics among ``metrics`` that need some, from ``--metric_weights`` -> {metric: weights}; without a
    directory, none (the metrics then fail to initialise, as before).  A file that is absent raises FileNotFoundError."""
    if not directory:
        return {}
    return {m: M.REGISTRY[m].load(directory) for m in metrics if m in M.metric_names(M.NETWORK, M.NR)}


def process(gt_root, pred_root, out_path, metrics, batch_mode=False, crop=0, test_y_channel=False, is_center=False,
            metric_weights=None) -> dict:
    if not torch.cuda.is_available():
        raise RuntimeError("dove_amd.eval_metrics computes PSNR / SSIM on the GPU; no HIP device is visible")
    device = torch.device("cuda")
    print(f"Using device: {device}")
    weights = load_weights(metrics, metric_weights)
    models = init_models(metrics, device, weights)
    gt_files, pred_files = pair_files(gt_root, pred_root)
    results = {}
    for name in sorted(pred_files):
        if gt_files is not None and name not in gt_files:
            print(f"Skipping {name}: no matching GT file.")
            continue
        try:
            nr = [m for m in models if m in M.metric_names(M.NR)]
            if gt_files is None:
                if not nr:
                    print(f"Skipping {name}: GT is not provided and no NR-IQA metrics found.")
                    continue
                vals = M.nr_clip_metrics(load_sequence(pred_files[name]), nr, weights)
                results[name] = {k: round(vals[k], 4) for k in nr}
                continue
            pred = load_sequence(pred_files[name])
            gt = load_sequence(gt_files[name])
            fr = [m for m in models if m in M.metric_names(M.FR) or m in weights]
            # batch_mode and per-frame mode both average the per-frame values of the clip; one launch covers all frames either way
            vals = M.clip_metrics(pred, gt, fr, crop=crop, test_y_channel=test_y_channel, is_center=is_center, name=name,
                                  weights=weights) if fr else {}
            results[name] = {k: round(vals[k], 4) for k in models}
        except Exception as e:
            print(f"Error processing {name}: {e}")

    print("\nPer-sample Results:")
    for name in sorted(results):
        print(f"{name}: " + ", ".join(f"{k}={v:.4f}" for k, v in results[name].items()))
    output = summarize(results, metrics)
    print("\nOverall Average Results:")
    if output["count"] > 0:
        for k, v in output["average"].items():
            print(f"{k.upper()}: {v:.4f}")
    else:
        print("No valid samples were processed.")
    print(f"\nProcessed {output['count']} samples.")
    os.makedirs(out_path, exist_ok=True)
    path = os.path.join(out_path, output_name(metrics))
    with open(path, "w") as f:
        json.dump(output, f, indent=2)
    print(f"Results saved to: {path}")
    return output


def main(argv=None):
    parser = argparse.ArgumentParser(description="PSNR / SSIM of SR results against ground truth on the GPU (dove_amd)")
    parser.add_argument("--gt", type=str, default="", help=f"Path to GT folder (optional for the no-reference {M.name_list(M.metric_names(M.NR))})")
    parser.add_argument("--pred", type=str, required=True, help="Path to predicted results folder")
    parser.add_argument("--out", type=str, default="", help="Path to save JSON output (as directory); default: --pred")
    parser.add_argument("--metrics", type=str, default="psnr,ssim",
                        help=f"Comma-separated list of metrics: {','.join(M.metric_names(M.FR))}; with --metric_weights also "
                             f"{','.join(M.metric_names(M.NETWORK, M.NR))}")
    parser.add_argument("--batch_mode", action="store_true", help="accepted; gives the same values as per-frame mode")
    parser.add_argument("--crop", type=int, default=0, help="Crop border size for PSNR/SSIM")
    parser.add_argument("--test_y_channel", action="store_true", help="Use Y channel for PSNR/SSIM")
    parser.add_argument("--is_center", action="store_true", help="Use center crop for PSNR/SSIM")
    parser.add_argument("--metric_weights", type=str, default="",
                        help=f"directory with the files of {M.weights_help()}; without it these metrics are not computed")
    args = parser.parse_args(argv)
    out = args.out or args.pred
    metric_list = [m.strip().lower() for m in args.metrics.split(",")]
    return process(args.gt, args.pred, out, metric_list, args.batch_mode, args.crop, args.test_y_channel, args.is_center, args.metric_weights)


if __name__ == "__main__":
    main()
