"""RGB <-> YUV on the GPU for YUV4MPEG2 video I/O (csrc/yuv.hip).

The coefficient tables live here and nowhere else: for ``bt601`` (Kr 0.299, Kb 0.114) and ``bt709`` (Kr 0.2126, Kb 0.0722), each in
``limited`` (Y 16..235, C 16..240) and ``full`` (0..255) range, the forward and inverse 3x3 matrices as ``rint(c * 65536)`` int32.  The
kernels are matrix-agnostic integer fixed point, so a conversion is defined bit for bit (tests/yuv_ref.py restates it in numpy).

The colour matrix is not part of a Y4M stream; the default is bt601 / limited, which is what swscale assumes for an RGB -> yuv444p
conversion without further flags (the reference's mp4 writer)."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import lib as L
from . import ops

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGES = ("limited", "full")
CHROMA_CODES = {"444": L.YUV_444, "422": L.YUV_422, "420": L.YUV_420, "mono": L.YUV_MONO}
SAVE_FORMATS = {"yuv444p": "444", "yuv422p": "422", "yuv420p": "420"}


def float_matrices(matrix: str, rng: str):
    """(forward rows Y,U,V; inverse rows R,G,B; offsets) as Python floats / ints."""
    if matrix not in KR_KB:
        raise ValueError(f"unknown YUV matrix {matrix!r}: one of {', '.join(KR_KB)}")
    if rng not in RANGES:
        raise ValueError(f"unknown YUV range {rng!r}: one of {', '.join(RANGES)}")
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc, oy = (219.0 / 255.0, 224.0 / 255.0, 16) if rng == "limited" else (1.0, 1.0, 0)
    fwd = [[kr * sy, kg * sy, kb * sy],
           [-0.5 * kr / (1 - kb) * sc, -0.5 * kg / (1 - kb) * sc, 0.5 * sc],
           [0.5 * sc, -0.5 * kg / (1 - kr) * sc, -0.5 * kb / (1 - kr) * sc]]
    inv = [[1 / sy, 0.0, 2 * (1 - kr) / sc],
           [1 / sy, -2 * kb * (1 - kb) / kg / sc, -2 * kr * (1 - kr) / kg / sc],
           [1 / sy, 2 * (1 - kb) / sc, 0.0]]
    return fwd, inv, (oy, 128, 128)


def int_matrices(matrix: str, rng: str):
    """The tables the kernels get: (forward, inverse) as 9 ints each, row-major, ``rint(c * 65536)``, and the offsets."""
    fwd, inv, off = float_matrices(matrix, rng)
    q = lambda m: [int(round(c * 65536)) for row in m for c in row]   # round() is round-half-even like rint; no coefficient is a tie
    return q(fwd), q(inv), off


@dataclass(frozen=True)
class YuvFormat:
    """What a Y4M payload means: chroma layout ('444', '422', '420', 'mono'), horizontal chroma siting of 4:2:0 ('centre' = C420jpeg,
    'left' = C420mpeg2 / C420paldv), colour matrix and range."""
    chroma: str = "444"
    matrix: str = "bt601"
    range: str = "limited"
    siting_h: str = "centre"

    def frame_bytes(self, h: int, w: int) -> int:
        from . import y4m
        return y4m.frame_bytes(h, w, self.chroma)

    def _c(self, inverse: bool) -> L.YuvFormat:
        if self.chroma not in CHROMA_CODES:
            raise ValueError(f"unknown chroma layout {self.chroma!r}: one of {', '.join(CHROMA_CODES)}")
        if self.siting_h not in ("centre", "left"):
            raise ValueError(f"unknown chroma siting {self.siting_h!r}: 'centre' or 'left'")
        fwd, inv, off = int_matrices(self.matrix, self.range)
        f = L.YuvFormat()
        f.coef[:] = inv if inverse else fwd
        f.offset[:] = off
        f.chroma = CHROMA_CODES[self.chroma]
        f.siting_h = L.YUV_SITING_CENTRE if self.siting_h == "centre" else L.YUV_SITING_LEFT
        return f


def format_of_reader(reader, matrix: str = "bt601", rng: str | None = None) -> YuvFormat:
    """The format of a ``y4m.Y4MReader``'s payloads; ``rng`` overrides the stream's XCOLORRANGE tag."""
    return YuvFormat(reader.chroma, matrix, rng or ("full" if reader.full_range else "limited"), reader.siting_h)


def save_format_to_chroma(save_format: str) -> str:
    """``--save_format`` (an ffmpeg pixel format, ref :541) -> chroma layout of the Y4M file written."""
    if save_format not in SAVE_FORMATS:
        raise ValueError(f"--save_format {save_format}: a Y4M file is written as one of {', '.join(SAVE_FORMATS)}")
    return SAVE_FORMATS[save_format]


def rgb_to_yuv(frames_or_video: torch.Tensor, fmt: YuvFormat, crop=None) -> torch.Tensor:
    """RGB on the device -> [F, frame_bytes] uint8 Y4M frame payloads on the device, without a copy of the input:

    * ``[F,H,W,3]`` uint8 frames (colour-fix output, ``.npy``, PNG), or
    * ``[3,F,H,W]`` / ``[1,3,F,H,W]`` float32 / bfloat16 decoder output in [0,1], quantised as ``postprocess_u8`` does.

    ``crop = (F', H', W')`` keeps the leading part of each axis (what removes the padding)."""
    t = frames_or_video
    if t.dtype == torch.uint8:
        if t.dim() != 4 or t.shape[3] != 3:
            raise ValueError(f"rgb_to_yuv: uint8 input must be [F,H,W,3] frames, got {tuple(t.shape)}")
        v = t.permute(0, 3, 1, 2)
    elif t.dtype in (torch.float32, torch.bfloat16):
        if t.dim() == 5 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 4 or t.shape[0] != 3:
            raise ValueError(f"rgb_to_yuv: float input must be a [3,F,H,W] video, got {tuple(frames_or_video.shape)}")
        v = t.permute(1, 0, 2, 3)
    else:
        raise TypeError(f"rgb_to_yuv: uint8, float32 or bfloat16 input, got {t.dtype}")
    if crop is not None:
        Fo, Ho, Wo = crop
        if not (0 < Fo <= v.shape[0] and 0 < Ho <= v.shape[2] and 0 < Wo <= v.shape[3]):
            raise ValueError(f"rgb_to_yuv: crop {tuple(crop)} does not fit inside {(v.shape[0], v.shape[2], v.shape[3])}")
        v = v[:Fo, :, :Ho, :Wo]
    return ops.rgb_to_yuv_u8(v, fmt._c(False))


def yuv_to_rgb(payload: torch.Tensor, h: int, w: int, fmt: YuvFormat) -> torch.Tensor:
    """[F, frame_bytes] uint8 payloads on the device -> [F,h,w,3] uint8 RGB frames on the device."""
    return ops.yuv_to_rgb_u8(payload.contiguous(), h, w, fmt._c(True))
