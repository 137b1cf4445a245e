"""Time the GPU colour fix (dove_amd.colorfix, csrc/colorfix.hip) on the headline clip and set it against two yardsticks that are not
the code under test:

  (a) the same operation in plain torch on the same device, as the reference's color_fix_util would run if its tensors were moved to
      the GPU: five replicate pads + dilated depthwise F.conv2d per input plus the adds (wavelet), var / mean / normalise (adain);
  (b) the traffic floor: one read of each bf16 input and one write of the uint8 frames, at the streaming rate measured for gn_apply
      (docs/measurement.md: 5.1 TB/s).

Content and style are bf16 [3,F,H,W] clips (style in [-1,1], as the CLI holds them), the output is the uint8 [F,H,W,3] frames.
hipEvents around CALLS calls after warm-up (docs/measurement.md).  Prints one JSON line.

    python tools/colorfix_bench.py [--frames 33 --height 720 --width 1280 --calls 20]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_RATE = 5.1e12      # bytes/s, gn_apply's read + write pass on the whole chip (docs/measurement.md)


def torch_wavelet(content, style):
    k = torch.tensor([[0.0625, 0.125, 0.0625], [0.125, 0.25, 0.125], [0.0625, 0.125, 0.0625]], dtype=content.dtype,
                     device=content.device)[None, None].repeat(3, 1, 1, 1)

    def decompose(x):
        high = torch.zeros_like(x)
        for i in range(5):
            r = 2 ** i
            low = F.conv2d(F.pad(x, (r, r, r, r), mode="replicate"), k, groups=3, dilation=r)
            high += x - low
            x = low
        return high, x

    return decompose(content)[0] + decompose(style)[1]


def torch_adain(content, style):
    def mean_std(x):
        flat = x.reshape(x.shape[0], x.shape[1], -1)
        return flat.mean(2)[..., None, None], (flat.var(2) + 1e-5).sqrt()[..., None, None]

    mc, sc = mean_std(content)
    ms, ss = mean_std(style)
    return (content - mc) / sc * ss + ms


def torch_path(content3, style3, mode):
    """bf16 [3,F,H,W] clips -> uint8 [F,H,W,3] frames, every step in torch (fp32)."""
    c = content3.permute(1, 0, 2, 3).float()
    s = style3.permute(1, 0, 2, 3).float() * 0.5 + 0.5
    res = torch_wavelet(c, s) if mode == "wavelet" else torch_adain(c, s)
    return (res.clamp_(0, 1) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def time_ms(fn, calls, warmup=3):
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--torch_calls", type=int, default=5)
    args = ap.parse_args(argv)
    from dove_amd import colorfix
    g = torch.Generator(device="cuda").manual_seed(0)
    shape = (3, args.frames, args.height, args.width)
    content = torch.rand(shape, device="cuda", generator=g).bfloat16()
    style = (content.float() * 0.9 + 0.05 + 0.05 * torch.randn(shape, device="cuda", generator=g)).clamp(0, 1).mul(2).sub(1).bfloat16()
    cv, sv = content.permute(1, 0, 2, 3), style.permute(1, 0, 2, 3)
    floor_bytes = content.numel() * (2 + 2 + 1)
    out = {"clip": list(shape), "calls": args.calls, "floor_bytes": floor_bytes, "floor_ms": floor_bytes / STREAM_RATE * 1e3}
    for mode in ("wavelet", "adain"):
        hip = time_ms(lambda: colorfix.color_fix(cv, sv, mode, out_dtype=torch.uint8, style_affine=(0.5, 0.5)), args.calls)
        ref = time_ms(lambda: torch_path(content, style, mode), args.torch_calls, warmup=1)
        a = colorfix.color_fix(cv, sv, mode, out_dtype=torch.uint8, style_affine=(0.5, 0.5))
        b = torch_path(content, style, mode)
        diff = (a.int() - b.int()).abs()
        out[mode] = {"hip_ms": round(hip, 4), "torch_ms": round(ref, 3), "speedup_vs_torch": round(ref / hip, 1),
                     "x_floor": round(hip / out["floor_ms"], 1), "achieved_GBps_of_floor_bytes": round(floor_bytes / hip / 1e6, 1),
                     "max_level_diff_vs_torch": int(diff.max()), "share_differing": float((diff > 0).float().mean())}
        del a, b, diff
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
