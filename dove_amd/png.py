"""PNG files written on the GPU (csrc/png.hip).

``ops.png_encode`` turns a batch of frames into complete PNG files on the device: per-scanline filters chosen by libpng's heuristic,
one literal-only dynamic-Huffman deflate block per segment of whole rows, all CRC-32s and the Adler-32.  This module adds the host
side: frame groups under a memory budget, downloads into pinned memory, and the files.  Decoding stays with PIL."""
from __future__ import annotations

import os

import torch

from . import ops

BUDGET_BYTES = 1 << 30          # device bytes one frame group may take: its out-buffer (png_bound per frame) plus the encoder's workspace


def as_nchw(frames: torch.Tensor, layout: str | None = None) -> torch.Tensor:
    """The forms ``save_frames`` accepts -> an [N,C,H,W] view (no copy): uint8 [F,H,W,3] / [F,H,W,1] / [F,H,W] frames, or a float32 /
    bfloat16 clip in [0,1] as [F,3,H,W] or [3,F,H,W] (the decoder's output; a clip of 3 frames is read as [F,3,H,W]).  ``layout`` names the
    form outright: 'fhwc', 'fchw' or 'cfhw'."""
    if layout is None:
        if frames.dtype == torch.uint8:
            layout = "fhwc"
        elif frames.dtype in (torch.float32, torch.bfloat16) and frames.dim() == 4:
            layout = "fchw" if frames.shape[1] in (1, 3) else "cfhw"
        else:
            raise TypeError(f"png: frames are uint8 [F,H,W,3] or float32 / bfloat16 [F,3,H,W] / [3,F,H,W], got {frames.dtype} "
                            f"{tuple(frames.shape)}")
    if layout == "fhwc":
        v = frames[..., None] if frames.dim() == 3 else frames
        if v.dim() != 4:
            raise ValueError(f"png: expected [F,H,W,C] frames, got {tuple(frames.shape)}")
        v = v.permute(0, 3, 1, 2)
    elif layout == "fchw":
        v = frames
    elif layout == "cfhw":
        v = frames.permute(1, 0, 2, 3)
    else:
        raise ValueError(f"png: layout must be 'fhwc', 'fchw' or 'cfhw', got {layout!r}")
    if v.dim() != 4 or v.shape[1] not in (1, 3):
        raise ValueError(f"png: frames of shape {tuple(frames.shape)} ({layout}) have {v.shape[1] if v.dim() == 4 else '?'} channels; 1 or 3 "
                         "are written")
    return v


def group_frames(h: int, w: int, channels: int, budget_bytes: int = BUDGET_BYTES) -> int:
    """Frames of one encode call so that out-buffer plus workspace stay under ``budget_bytes`` (at least 1)."""
    from . import lib as L
    per_frame = ops.png_bound(h, w, channels) + int(L.load().dove_png_workspace_bytes(1, h, w, channels))
    if per_frame == 0:
        raise ValueError(f"png: frames of {h} x {w} x {channels} cannot be encoded")
    return max(1, budget_bytes // per_frame)


def _encode_groups(frames, layout, budget_bytes):
    """Yields (first frame index, pinned host buffer, offsets) per frame group."""
    if not torch.cuda.is_available():
        raise RuntimeError("the GPU PNG encoder needs a HIP device (`cuda`); use encoder='pil' without one")
    v = as_nchw(frames, layout)
    if not v.is_cuda:
        v = v.cuda()                                                  # a host tensor is uploaded
    N, Cc, H, W = v.shape
    G = group_frames(H, W, Cc, budget_bytes)
    for f0 in range(0, N, G):
        out, sizes = ops.png_encode(v[f0:f0 + G])
        sz = sizes.cpu().tolist()                                     # synchronises: the sizes decide what is downloaded
        offs = [0]
        for s in sz:
            offs.append(offs[-1] + s)
        host = torch.empty(max(offs[-1], 1), dtype=torch.uint8, pin_memory=True)
        for i, s in enumerate(sz):
            host[offs[i]:offs[i + 1]].copy_(out[i, :s], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        yield f0, host, offs


def encode(frames: torch.Tensor, layout: str | None = None, budget_bytes: int = BUDGET_BYTES) -> list:
    """Frames (see ``as_nchw``; a host tensor is uploaded) -> one ``bytes`` object per frame, each a complete PNG file."""
    files = []
    for _, host, offs in _encode_groups(frames, layout, budget_bytes):
        buf = host.numpy()
        files.extend(buf[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1))
    return files


def save_frames(frames: torch.Tensor, output_dir: str, names=None, layout: str | None = None, budget_bytes: int = BUDGET_BYTES) -> list:
    """Encode on the GPU in frame groups and write ``output_dir/names[i]`` (default ``{i:03d}.png``, the reference's naming); returns
    the paths."""
    os.makedirs(output_dir, exist_ok=True)
    paths = []
    for f0, host, offs in _encode_groups(frames, layout, budget_bytes):
        buf = host.numpy()
        for i in range(len(offs) - 1):
            name = names[f0 + i] if names is not None else f"{f0 + i:03d}.png"
            path = os.path.join(output_dir, name)
            with open(path, "wb") as f:
                f.write(memoryview(buf[offs[i]:offs[i + 1]]))
            paths.append(path)
    return paths
