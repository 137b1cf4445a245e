"""Colour fix of restored frames against their upscaled input on the GPU (csrc/colorfix.hip, ``dove_color_fix``): the StableSR colour
fix the reference ships in ``finetune/scripts/color_fix_util.py``.  *content* is the restored frame, *style* the upscaled low-quality
frame; the result keeps the content's detail and takes the style's colour.

Surfaces:
  - ``wavelet_reconstruction(content, style)`` / ``adaptive_instance_normalization(content, style)``: the reference's names, argument
    order and convention ([N,3,H,W] in [0,1] -> float32 [N,3,H,W], not clamped), so ``from dove_amd.colorfix import
    wavelet_reconstruction, adaptive_instance_normalization`` replaces the util's two functions;
  - ``color_fix(content, style, mode, *, out_dtype=None, clamp=True)``: the same on strided views (permuted [3,F,H,W] clips, crops,
    uint8 frames), with an affine per input and any of float32 / bfloat16 / uint8 out;
  - ``python -m dove_amd.colorfix --pred DIR --source DIR --out DIR --mode wavelet|adain``: results that are already on disk.

Definitions, every frame and channel on its own:
  wavelet: out = content + low5(style - content), low5 = B_16 B_8 B_4 B_2 B_1, B_r = the 3x3 kernel [1,2,1]^T [1,2,1] / 16 with
           dilation r on its replicate-padded input (the reference's (content - low5(content)) + low5(style), by linearity);
  adain:   out = (content - mean_c) / std_c * std_s + mean_s with std = sqrt(unbiased variance + 1e-5).
uint8 out is trunc(clamp(x, 0, 1) * 255): what the reference's PIL wrappers (clamp_, ToPILImage) and ``dove_postprocess_u8`` write."""
from __future__ import annotations

import argparse
import os

import torch

from . import lib as L
from . import ops

MODES = {"wavelet": L.COLORFIX_WAVELET, "adain": L.COLORFIX_ADAIN}


def _as_nchw(t: torch.Tensor, what: str) -> torch.Tensor:
    """[N,3,H,W] as it is; [F,H,W,3] uint8 frames as a permuted view."""
    if t.dim() != 4:
        raise ValueError(f"color_fix: {what} must be a 4-D image batch, got shape {tuple(t.shape)}")
    if t.dtype == torch.uint8 and t.shape[3] == 3 and t.shape[1] != 3:
        return t.permute(0, 3, 1, 2)
    if t.shape[1] != 3:
        raise ValueError(f"color_fix: {what} must be [N,3,H,W] (or [F,H,W,3] uint8 frames), got shape {tuple(t.shape)}")
    return t


def color_fix(content: torch.Tensor, style: torch.Tensor, mode: str, *, out_dtype=None, clamp: bool = True,
              content_affine=(1.0, 0.0), style_affine=(1.0, 0.0)) -> torch.Tensor:
    """Colour fix of ``content`` towards ``style`` -> [N,3,H,W] (float32 / bfloat16) or [N,H,W,3] frames (``out_dtype=torch.uint8``).

    ``content`` / ``style``: [N,3,H,W] tensors with any strides - a [3,F,H,W] clip goes in as ``clip.permute(1, 0, 2, 3)``, a crop as a
    slice, nothing is copied - or [F,H,W,3] uint8 frames.  dtypes float32 / bfloat16 (values in [0,1]) and uint8 (read as u/255), mixed
    freely; each input is read as ``scale * raw + bias`` (``style_affine=(0.5, 0.5)`` reads a [-1,1] clip).  ``mode``: 'wavelet' or
    'adain'.  ``out_dtype``: None = the content's dtype.  ``clamp``: clamp a float result to [0,1] (uint8 always is).
    Host tensors are moved to the current HIP device; there is no CPU path."""
    if mode not in MODES:
        raise ValueError(f"color_fix: mode must be one of {sorted(MODES)}, got {mode!r}")
    dev = content.device if content.is_cuda else (style.device if style.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    c, s = _as_nchw(content.to(dev), "content"), _as_nchw(style.to(dev), "style")
    if c.shape != s.shape:
        raise ValueError(f"color_fix: content {tuple(c.shape)} and style {tuple(s.shape)} differ in shape")
    out_dtype = out_dtype or c.dtype
    N, _, H, W = c.shape
    if out_dtype == torch.uint8:
        frames = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
        ops.color_fix(c, s, MODES[mode], frames.permute(0, 3, 1, 2), clamp, content_affine, style_affine)
        return frames
    out = torch.empty(N, 3, H, W, dtype=out_dtype, device=dev)
    return ops.color_fix(c, s, MODES[mode], out, clamp, content_affine, style_affine)


def wavelet_reconstruction(content_feat: torch.Tensor, style_feat: torch.Tensor) -> torch.Tensor:
    """color_fix_util.wavelet_reconstruction: [N,3,H,W] in [0,1] -> float32 [N,3,H,W], not clamped, on the content's device."""
    return color_fix(content_feat, style_feat, "wavelet", out_dtype=torch.float32, clamp=False).to(content_feat.device)


def adaptive_instance_normalization(content_feat: torch.Tensor, style_feat: torch.Tensor) -> torch.Tensor:
    """color_fix_util.adaptive_instance_normalization: [N,3,H,W] in [0,1] -> float32 [N,3,H,W], not clamped, on the content's device."""
    return color_fix(content_feat, style_feat, "adain", out_dtype=torch.float32, clamp=False).to(content_feat.device)


# ---- python -m dove_amd.colorfix: results that are already on disk ---------------------------------------------------------------
def pair_files(source_root: str, pred_root: str):
    """(source_files, pred_files): {os.path.splitext stem: path}, as eval_metrics.pair_files pairs predictions and ground truth."""
    from .eval_metrics import pair_files as pair
    if not os.path.isdir(source_root):
        raise ValueError(f"--source {source_root}: not a folder")
    return pair(source_root, pred_root)


def upscale_factor(pred_shape, source_shape):
    """[F,H,W,3] shapes -> 1 when the sizes match, k when pred is k times the source in both H and W (k integer), else None."""
    (_, hp, wp, _), (_, hs, ws, _) = pred_shape, source_shape
    if hp % hs or wp % ws or hp // hs != wp // ws:
        return None
    return hp // hs


def fix_clip(pred_u8: torch.Tensor, source_u8: torch.Tensor, mode: str) -> torch.Tensor:
    """[F,H,W,3] uint8 prediction and its source ([F,H,W,3] or [F,H/k,W/k,3], upscaled by the bilinear kernel of the pre-processing) ->
    fixed [F,H,W,3] uint8 frames on the device."""
    k = upscale_factor(pred_u8.shape, source_u8.shape)
    if k is None or pred_u8.shape[0] != source_u8.shape[0]:
        raise ValueError(f"pred {tuple(pred_u8.shape)} is neither the size of source {tuple(source_u8.shape)} nor an integer multiple")
    if not torch.cuda.is_available():
        raise RuntimeError("dove_amd.colorfix runs on the GPU; no HIP device is visible")
    pred, src = pred_u8.cuda(), source_u8.cuda()
    if k == 1:
        return color_fix(pred, src, mode, out_dtype=torch.uint8)
    up = ops.preprocess_u8(src.contiguous(), 0, 0, 0, k, torch.float32)               # [3,F,H,W] in [-1,1]
    return color_fix(pred, up.permute(1, 0, 2, 3), mode, out_dtype=torch.uint8, style_affine=(0.5, 0.5))


def save_sequence(frames_u8: torch.Tensor, like: str, out_root: str, png_encoder: str = "pil") -> str:
    """Write the fixed frames in the form of the prediction at ``like``: a PNG folder, one image, an ``.npy`` clip or a ``.y4m`` file."""
    from . import prepost
    base = os.path.basename(like.rstrip(os.sep))
    path = os.path.join(out_root, base)
    if os.path.isdir(like):
        prepost.save_frames_as_png(frames_u8, path, encoder=png_encoder)
    elif like.lower().endswith(".npy"):
        import numpy as np
        np.save(path, frames_u8.cpu().numpy())
    elif like.lower().endswith(".y4m"):                       # the prediction's own frame rate, chroma layout and range (bt601)
        from . import y4m, yuv
        with y4m.Y4MReader(like) as rd:
            fps, chroma, full = rd.fps, rd.chroma, rd.full_range
        payload = yuv.rgb_to_yuv(frames_u8.cuda(), yuv.YuvFormat(chroma, "bt601", "full" if full else "limited"))
        with y4m.Y4MWriter(path, frames_u8.shape[2], frames_u8.shape[1], fps, chroma, full) as wr:
            wr.write(payload.cpu())
    else:
        from PIL import Image
        path = os.path.splitext(path)[0] + ".png"
        if png_encoder == "gpu":
            from . import png
            png.save_frames(frames_u8[:1], os.path.dirname(path) or ".", names=[os.path.basename(path)])
        else:
            Image.fromarray(frames_u8[0].cpu().numpy()).save(path)
    return path


def process(pred_root: str, source_root: str, out_root: str, mode: str, png_encoder: str = "pil") -> list:
    from .eval_metrics import load_sequence
    if mode not in MODES:
        raise ValueError(f"--mode must be one of {sorted(MODES)}, got {mode!r}")
    source_files, pred_files = pair_files(source_root, pred_root)
    os.makedirs(out_root, exist_ok=True)
    done = []
    for name in sorted(pred_files):
        if name not in source_files:
            print(f"Skipping {name}: no matching source file.")
            continue
        pred, src = load_sequence(pred_files[name]), load_sequence(source_files[name])       # mp4: refused by prepost.load_frames
        if pred.shape[0] != src.shape[0] or upscale_factor(pred.shape, src.shape) is None:
            print(f"Skipping {name}: pred {tuple(pred.shape)} does not match source {tuple(src.shape)} (equal size or an integer "
                  "upscale factor, and the same frame count).")
            continue
        path = save_sequence(fix_clip(pred, src, mode), pred_files[name], out_root, png_encoder)
        print(f"{name}: {mode} colour fix -> {path}")
        done.append(name)
    print(f"Processed {len(done)} samples.")
    return done


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Colour fix (wavelet / AdaIN) of SR results against their source on the GPU (dove_amd)")
    parser.add_argument("--pred", type=str, required=True, help="folder of restored results (PNG folders, images, .npy clips)")
    parser.add_argument("--source", type=str, required=True, help="folder of the inputs they were restored from (same size, or smaller "
                        "by an integer factor: upscaled bilinearly first)")
    parser.add_argument("--out", type=str, required=True, help="folder the fixed results are written to")
    parser.add_argument("--mode", type=str, choices=sorted(MODES), default="wavelet")
    parser.add_argument("--png_encoder", type=str, default="pil", choices=("pil", "gpu"),
                        help="who writes PNG results: PIL on the host, or the GPU encoder (dove_amd.png)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    return process(args.pred, args.source, args.out, args.mode, args.png_encoder)


if __name__ == "__main__":
    main()
