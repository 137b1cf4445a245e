"""Time the GPU JPEG encoder (dove_amd.jpeg, csrc/jpeg.hip) on production-size frames, 2880 x 5120 RGB at quality 95, in both
subsamplings, against the only baseline there is: Pillow's encoder on the host, the cost --jpg_save would otherwise have.

  device time    ops.jpeg_encode of FRAMES device-resident uint8 frames, hipEvents around CALLS calls after warm-up (docs/measurement.md),
                 per frame, and the input bytes per second that makes;
  copy rate      a device-to-device copy of the same frames, timed the same way: the rate an HBM-bound pass over the input could reach;
  download       the device-to-host copy of the files' bytes into pinned memory, timed the same way;
  Pillow         Image.save(format='JPEG', quality=95, subsampling=...) of one frame on the host, best of REPS, and its file size;
  check          every GPU file is opened by Pillow.

The frames are synthetic: a smooth field, a 4 x 4 texture and noise, seeded.  Per-kernel times come from a run of their own under the
profiler, whose kernel table --stats_csv folds into the line:

    rocprofv3 --kernel-trace --stats --output-format csv -d prof_out -- python tools/bench_jpeg.py --encode_only --calls 5
    python tools/bench_jpeg.py --stats_csv prof_out/<...>_kernel_stats.csv

Prints one JSON line."""
import argparse
import csv
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("code_kernel", "scan_kernel", "gather_kernel")


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


def stage_table(path):
    """rocprofv3's kernel_stats CSV -> {stage: {calls, avg_ms}} for the encoder's kernels."""
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
        e["total_ms"] = round(e["total_ms"], 3)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--height", type=int, default=2880)
    ap.add_argument("--width", type=int, default=5120)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2, help="Pillow encodes per subsampling (best is kept)")
    ap.add_argument("--encode_only", action="store_true", help="only the encode calls (the run to put under rocprofv3)")
    ap.add_argument("--stats_csv", type=str, default=None, help="kernel_stats CSV of such a run: adds the per-kernel times")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_jpeg.py measures on the GPU; no HIP device is visible")
    from PIL import Image

    from dove_amd import ops
    frames = make_frames(args.frames, args.height, args.width)
    view = frames.permute(0, 3, 1, 2)
    raw = frames.numel()
    out = {"frames": [args.frames, args.height, args.width, 3], "raw_bytes_per_frame": raw // args.frames, "quality": args.quality,
           "calls": args.calls, "restart_mcus": ops.jpeg_restart_mcus()}
    if not args.encode_only:
        dst = torch.empty_like(frames)
        ms = device_ms(lambda: dst.copy_(frames), args.calls)
        out["copy_GBps_of_input"] = round(raw / ms / 1e6, 1)                       # bytes read per second (as many are written)
    if args.stats_csv:
        out["stages"] = stage_table(args.stats_csv)
    for sub in ("444", "420"):
        r = {"bound_bytes_per_frame": ops.jpeg_bound(args.height, args.width, sub)}
        ms = device_ms(lambda: ops.jpeg_encode(view, args.quality, sub), args.calls)
        r["encode_device_ms_per_frame"] = round(ms / args.frames, 4)
        r["encode_GBps_of_input"] = round(raw / ms / 1e6, 1)
        if not args.encode_only:
            files, sizes = ops.jpeg_encode(view, args.quality, sub)
            sz = sizes.cpu().tolist()
            host = torch.empty(sum(sz), dtype=torch.uint8, pin_memory=True)

            def download():
                o = 0
                for i, s in enumerate(sz):
                    host[o:o + s].copy_(files[i, :s], non_blocking=True)
                    o += s
            r["download_ms_per_frame"] = round(device_ms(download, args.calls) / args.frames, 4)
            r["gpu_file_bytes"] = sz[0]
            buf, o = host.numpy(), 0
            for s in sz:
                im = Image.open(io.BytesIO(buf[o:o + s].tobytes()))
                im.load()
                if im.size != (args.width, args.height):
                    raise RuntimeError("a GPU file does not open in Pillow")
                o += s
            one = Image.fromarray(frames[0].cpu().numpy())
            best, pil_bytes = None, 0
            for _ in range(args.reps):
                b = io.BytesIO()
                t = time.perf_counter()
                one.save(b, format="JPEG", quality=args.quality, subsampling={"444": 0, "420": 2}[sub])
                dt = time.perf_counter() - t
                best = dt if best is None else min(best, dt)
                pil_bytes = b.tell()
            r["pillow_encode_ms_per_frame"] = round(best * 1e3, 1)
            r["pillow_file_bytes"] = pil_bytes
            r["gpu_over_pillow_bytes"] = round(sz[0] / pil_bytes, 4)
            r["raw_over_gpu_bytes"] = round(raw / args.frames / sz[0], 2)
            r["gpu_files_open_in_pillow"] = True
        out[sub] = r
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
