"""GPU-side script-level pre/post-processing and dependency-free frame I/O.

Mirrors /root/reference/inference_script.py: ``preprocess_video_match`` padding (:192-235), the bilinear upscale and
[-1,1] normalisation (:670-679), ``remove_padding_and_extra_frames`` (:238-246, called with the reference's hard-coded
``pad*4`` at :731) and the uint8 conversion of the savers (:124).  Video decoding (decord/H.264) stays outside: clips
come in as uint8 arrays ([F,H,W,3] ``.npy``), PNG folders or YUV4MPEG2 files (``.y4m``, the codec-free container of
``ffmpeg -f yuv4mpegpipe``; dove_amd.y4m, dove_amd.yuv)."""
from __future__ import annotations

import os

import torch

from . import ops, tiling


def preprocess_frames(frames_u8: torch.Tensor, upscale: int = 4, dtype=torch.bfloat16, device="cuda", upscale_mode: str = "bilinear"):
    """[F,H,W,3] uint8 -> ([1,3,F',H',W'] in [-1,1] on the GPU, pad_f, pad_h, pad_w, original_shape).

    ``upscale_mode`` is the reference's ``--upscale_mode`` (ref :672: ``F.interpolate(video, size, mode=..., align_corners=False)``).
    "bilinear" (the default of every documented run) is the fused HIP kernel ``dove_preprocess_u8``; any other mode torch accepts with
    ``align_corners=False`` ("bicubic") runs the same three script steps - pad, ``F.interpolate``, ``/255*2-1`` - with torch on
    the device: script-level pre-processing, not part of the accelerated operator."""
    F, H, W, C = frames_u8.shape
    assert C == 3 and frames_u8.dtype == torch.uint8
    pad_f, pad_h, pad_w = tiling.match_padding(F, H, W)
    if upscale_mode == "bilinear":
        video = ops.preprocess_u8(frames_u8.to(device).contiguous(), pad_f, pad_h, pad_w, upscale, dtype)
    else:
        video = preprocess_frames_torch(frames_u8.to(device), pad_f, pad_h, pad_w, upscale, upscale_mode, dtype)
    return video[None], pad_f, pad_h, pad_w, (F, H, W, C)


def preprocess_frames_torch(frames_u8, pad_f, pad_h, pad_w, upscale, upscale_mode, dtype):
    """The reference's own three steps (``preprocess_video_match`` padding :220-233, ``F.interpolate`` :672, normalise :673-676):
    [F,H,W,3] uint8 -> [3,F',H',W'] in [-1,1]."""
    v = frames_u8.permute(0, 3, 1, 2).float()                               # [F,C,H,W] like decord + permute (ref :206)
    if pad_f:
        v = torch.cat([v, v[-1:].repeat(pad_f, 1, 1, 1)], dim=0)            # repeat the last frame (ref :222-224)
    if pad_h or pad_w:
        v = torch.nn.functional.pad(v, (0, pad_w, 0, pad_h))                # zeros, bottom / right (ref :232)
    v = torch.nn.functional.interpolate(v, size=(v.shape[2] * upscale, v.shape[3] * upscale), mode=upscale_mode, align_corners=False)
    return (v / 255.0 * 2.0 - 1.0).permute(1, 0, 2, 3).contiguous().to(dtype)


def postprocess_frames(video: torch.Tensor, pad_f: int, pad_h: int, pad_w: int, crop_scale: int = 4, color_fix: str | None = None,
                       source: torch.Tensor | None = None) -> torch.Tensor:
    """[1,3,F,H,W] in [0,1] -> [F',H',W',3] uint8 with the padding removed.  ``crop_scale`` is the reference's hard-coded 4
    (ref :731 multiplies the LR pads by 4 regardless of --upscale).

    ``color_fix`` ('wavelet' / 'adain', dove_amd.colorfix) with ``source`` = the clip's upscaled input ([1,3,F,H,W] in [-1,1], what
    ``preprocess_frames`` returned): the un-padded crop of ``video`` is colour-fixed against the same crop of ``source`` and comes out
    as the uint8 frames directly.  The crop comes first, so the replicate border of the fix is the border of the frames returned - as if
    the reference's color_fix_util had been run on the saved files."""
    _, _, F, H, W = video.shape
    Fo, Ho, Wo = F - pad_f, H - pad_h * crop_scale, W - pad_w * crop_scale
    if color_fix is None:
        return ops.postprocess_u8(video[0].contiguous(), Fo, Ho, Wo)
    if source is None or source.shape != video.shape:
        raise ValueError(f"postprocess_frames(color_fix={color_fix!r}) needs source of the video's shape {tuple(video.shape)}")
    from . import colorfix
    content = video[0, :, :Fo, :Ho, :Wo].permute(1, 0, 2, 3)                 # [F',3,H',W'] views: nothing is copied
    style = source[0, :, :Fo, :Ho, :Wo].permute(1, 0, 2, 3)
    return colorfix.color_fix(content, style, color_fix, out_dtype=torch.uint8, style_affine=(0.5, 0.5))


def load_y4m(path, yuv_matrix: str = "bt601", yuv_range: str | None = None, block: int = 64) -> torch.Tensor:
    """A YUV4MPEG2 file (or binary file object) -> host uint8 [F,H,W,3]: ``y4m.Y4MReader`` -> ``yuv.yuv_to_rgb`` on the GPU, ``block``
    frames at a time.  Y4M carries no colour matrix (``yuv_matrix``); ``yuv_range`` overrides the stream's XCOLORRANGE tag."""
    from . import y4m, yuv
    if not torch.cuda.is_available():
        raise RuntimeError("a .y4m clip is converted to RGB on the GPU (csrc/yuv.hip); no HIP device is visible")
    out = []
    with y4m.Y4MReader(path) as rd:
        fmt = yuv.format_of_reader(rd, yuv_matrix, yuv_range)
        while True:
            payload = rd.read(block)
            if payload.shape[0]:
                out.append(yuv.yuv_to_rgb(payload.cuda(), rd.height, rd.width, fmt).cpu())
            if payload.shape[0] < block:
                break
    if not out:
        raise ValueError(f"no frames in {path}")
    return torch.cat(out)


def load_frames(path: str, yuv_matrix: str = "bt601", yuv_range: str | None = None) -> torch.Tensor:
    """``.npy`` ([F,H,W,3] uint8), a ``.y4m`` file (YUV4MPEG2; converted on the GPU) or a folder of PNG/JPG frames -> uint8 tensor
    [F,H,W,3] on the host."""
    import numpy as np
    if os.path.isfile(path) and path.lower().endswith(".y4m"):
        return load_y4m(path, yuv_matrix, yuv_range)
    if os.path.isdir(path):
        from PIL import Image
        names = sorted(n for n in os.listdir(path) if n.lower().endswith((".png", ".jpg", ".jpeg")))
        if not names:
            raise ValueError(f"no frames in {path}")
        arr = np.stack([np.asarray(Image.open(os.path.join(path, n)).convert("RGB")) for n in names])
    elif path.lower().endswith(".npy"):
        arr = np.load(path)
    else:
        raise ValueError(f"unsupported input {path}: H.264 decoding (decord) is outside the accelerated path; "
                         "convert the clip to a PNG folder, an .npy array or a .y4m file (ffmpeg -i clip -pix_fmt yuv420p -f yuv4mpegpipe clip.y4m)")
    if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3:
        raise ValueError(f"expected uint8 [F,H,W,3], got {arr.dtype} {arr.shape}")
    return torch.from_numpy(arr.copy())


def save_frames_as_png(frames_u8: torch.Tensor, output_dir: str, encoder: str = "pil"):
    """Same file naming as the reference's ``save_frames_as_png`` (ref :111-128).  ``encoder``: 'pil' (the default: PIL's writer on the
    host) or 'gpu' (dove_amd.png: the files are encoded on the device and only written here)."""
    if encoder == "gpu":
        from . import png
        png.save_frames(frames_u8, output_dir)
        return
    if encoder != "pil":
        raise ValueError(f"encoder must be 'pil' or 'gpu', got {encoder!r}")
    from PIL import Image
    os.makedirs(output_dir, exist_ok=True)
    for i, fr in enumerate(frames_u8.cpu().numpy()):
        Image.fromarray(fr).save(os.path.join(output_dir, f"{i:03d}.png"))


def save_frames_as_jpeg(frames_u8: torch.Tensor, output_dir: str, quality: int = 95, subsampling: str = "444"):
    """``{i:03d}.jpg`` files, the PNG saver's naming, encoded on the GPU (dove_amd.jpeg; there is no host encoder behind this)."""
    from . import jpeg
    jpeg.save_frames(frames_u8, output_dir, quality=quality, subsampling=subsampling)
