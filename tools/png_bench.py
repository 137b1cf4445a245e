"""Time the GPU PNG encoder (dove_amd.png, csrc/png.hip) on the headline clip, 33 x 720 x 1280 RGB, against the writer it replaces:

  device time   ops.png_encode on the whole clip, hipEvents around CALLS calls after warm-up (docs/measurement.md), per call and per frame;
  wall time     prepost.save_frames_as_png of the device-resident uint8 frames into a fresh folder with encoder='pil' and encoder='gpu',
                a host clock around the call (it ends with the files written; the GPU route synchronises on its downloads);
  file sizes    total bytes of both folders, and every GPU file read back by PIL and compared with its frame.

The frames are synthetic: a smooth field, a 4 x 4 texture and noise, seeded.  Per-stage device times come from a run of their own under
the profiler (tracing slows the host, so it is not mixed with the wall times), whose kernel table --stats_csv folds into the line:

    rocprofv3 --kernel-trace --stats --output-format csv -d prof_out -- python tools/png_bench.py --encode_only --calls 5
    python tools/png_bench.py --stats_csv prof_out/<...>_kernel_stats.csv [--frames 33 --height 720 --width 1280 --calls 20]

Prints one JSON line."""
import argparse
import csv
import json
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("filter_kernel", "build_kernel", "scan_kernel", "pack_kernel")


def make_frames(frames, h, w, seed=0):
    """uint8 [F,H,W,3] on the device: smooth field + 4 x 4 texture + noise."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy = torch.arange(h, device="cuda", dtype=torch.float32)[None, :, None, None]
    xx = torch.arange(w, device="cuda", dtype=torch.float32)[None, None, :, None]
    f = torch.arange(frames, device="cuda", dtype=torch.float32)[:, None, None, None]
    ch = torch.arange(3, device="cuda", dtype=torch.float32)[None, None, None, :]
    field = 128 + 90 * torch.sin(xx / 230.0 + 0.1 * f + ch) * torch.cos(yy / 170.0 - ch)
    tex = 12 * (((xx // 4) + (yy // 4)) % 2)
    noise = 4 * torch.randn(frames, h, w, 3, device="cuda", generator=g)
    return (field + tex + noise).clamp_(0, 255).to(torch.uint8)


def device_ms(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def wall_s(frames, encoder, root, reps):
    from dove_amd import prepost
    best, sizes = None, None
    for r in range(reps):
        d = os.path.join(root, f"{encoder}_{r}")
        torch.cuda.synchronize()
        t = time.perf_counter()
        prepost.save_frames_as_png(frames, d, encoder=encoder)
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
        sizes = [os.path.getsize(os.path.join(d, n)) for n in sorted(os.listdir(d))]
        if r + 1 < reps:
            shutil.rmtree(d)
    return best, sizes, d


def stage_table(path, calls_per_frame_batch):
    """rocprofv3's kernel_stats CSV -> {stage: {calls, avg_ms}} for the encoder's four kernels."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for st in STAGES:
                if st in name:
                    e = out.setdefault(st, {"calls": 0, "total_ms": 0.0})
                    e["calls"] += int(row["Calls"])
                    e["total_ms"] += float(row["TotalDurationNs"]) / 1e6
    for e in out.values():
        e["avg_ms"] = round(e["total_ms"] / max(e["calls"], 1), 4)
        e["avg_ms_per_frame"] = round(e["avg_ms"] / calls_per_frame_batch, 5)
        e["total_ms"] = round(e["total_ms"], 3)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--pil_reps", type=int, default=1)
    ap.add_argument("--gpu_reps", type=int, default=3)
    ap.add_argument("--encode_only", action="store_true", help="only the encode calls (the run to put under rocprofv3)")
    ap.add_argument("--stats_csv", type=str, default=None, help="kernel_stats CSV of such a run: adds the per-stage times")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/png_bench.py measures on the GPU; no HIP device is visible")
    from PIL import Image

    import numpy as np

    from dove_amd import ops
    frames = make_frames(args.frames, args.height, args.width)
    view = frames.permute(0, 3, 1, 2)
    raw = frames.numel()
    out = {"clip": [args.frames, args.height, args.width, 3], "raw_bytes": raw, "calls": args.calls,
           "segment_rows": ops.png_segment_rows(args.width, 3), "bound_bytes_per_frame": ops.png_bound(args.height, args.width, 3)}
    ms = device_ms(lambda: ops.png_encode(view), args.calls)
    out["encode_device_ms"] = round(ms, 4)
    out["encode_device_ms_per_frame"] = round(ms / args.frames, 5)
    out["encode_GBps_of_raw"] = round(raw / ms / 1e6, 1)
    if args.stats_csv:
        out["stages"] = stage_table(args.stats_csv, args.frames)
    if not args.encode_only:
        root = tempfile.mkdtemp(prefix="png_bench_")
        try:
            gpu_s, gpu_sizes, gpu_dir = wall_s(frames, "gpu", root, args.gpu_reps + 1)      # the first repetition warms the pinned pool
            pil_s, pil_sizes, _ = wall_s(frames, "pil", root, args.pil_reps)
            host = frames.cpu().numpy()
            for i, n in enumerate(sorted(os.listdir(gpu_dir))):
                if not np.array_equal(np.asarray(Image.open(os.path.join(gpu_dir, n))), host[i]):
                    raise RuntimeError(f"{n} does not decode to its frame")
        finally:
            shutil.rmtree(root, ignore_errors=True)
        out.update({"save_wall_s": {"pil": round(pil_s, 3), "gpu": round(gpu_s, 3)}, "save_speedup": round(pil_s / gpu_s, 1),
                    "file_bytes": {"pil": sum(pil_sizes), "gpu": sum(gpu_sizes)},
                    "gpu_over_pil_bytes": round(sum(gpu_sizes) / sum(pil_sizes), 4), "gpu_files_decode_to_frames": True})
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
