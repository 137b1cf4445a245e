"""JPEG files and Motion-JPEG AVI clips written on the GPU (csrc/jpeg.hip).

``ops.jpeg_encode`` turns a batch of frames into complete baseline JFIF files on the device: colour conversion, 4:4:4 or 4:2:0, integer
DCT, Annex-K quantisation under libjpeg's quality rule, Huffman coding with the Annex-K tables in restart intervals, byte stuffing and all
markers.  This module adds the host side: frame groups under a memory budget, downloads of only the bytes a file takes, the files, and the
``.avi`` container (dove_amd.avi).  Decoding stays with PIL.

    python -m dove_amd.jpeg SRC (--out DIR | --avi FILE) [--quality Q] [--fps N] [--subsampling 444|420]

converts a PNG folder, ``.npy`` or ``.y4m`` clip (as ``prepost.load_frames`` reads them) to a folder of ``.jpg`` files or one ``.avi``."""
from __future__ import annotations

import os

import torch

from . import ops
from .png import as_nchw

BUDGET_BYTES = 1 << 30          # device bytes one frame group may take: its out-buffer (jpeg_bound per frame) plus the encoder's workspace


def group_frames(h: int, w: int, subsampling: str = "444", budget_bytes: int = BUDGET_BYTES) -> int:
    """Frames of one encode call so that out-buffer plus workspace stay under ``budget_bytes`` (at least 1)."""
    from . import lib as L
    sub = ops.jpeg_subsampling_code(subsampling)
    per_frame = ops.jpeg_bound(h, w, sub) + int(L.load().dove_jpeg_workspace_bytes(1, h, w, sub))
    if per_frame == 0:
        raise ValueError(f"jpeg: frames of {h} x {w} cannot be encoded (a JPEG file holds at most 65535 x 65535 pixels)")
    return max(1, budget_bytes // per_frame)


def _rgb_nchw(frames: torch.Tensor, layout) -> torch.Tensor:
    v = as_nchw(frames, layout)
    if v.shape[1] != 3:
        raise ValueError(f"jpeg: frames of shape {tuple(frames.shape)} are not RGB; grey JPEG files are not written")
    return v


def _encode_groups(frames, quality, subsampling, layout, budget_bytes):
    """Yields (first frame index, pinned host buffer, offsets) per frame group."""
    if not torch.cuda.is_available():
        raise RuntimeError("the GPU JPEG encoder needs a HIP device (`cuda`)")
    v = _rgb_nchw(frames, layout)
    if not v.is_cuda:
        v = v.cuda()                                                  # a host tensor is uploaded
    N, _, H, W = v.shape
    q = [int(quality)] * N if isinstance(quality, (int, float)) else [int(x) for x in quality]
    if len(q) != N:
        raise ValueError(f"jpeg: {len(q)} qualities for {N} frames")
    G = group_frames(H, W, subsampling, budget_bytes)
    for f0 in range(0, N, G):
        out, sizes = ops.jpeg_encode(v[f0:f0 + G], q[f0:f0 + G], subsampling)
        sz = sizes.cpu().tolist()                                     # synchronises: the sizes decide what is downloaded
        offs = [0]
        for s in sz:
            offs.append(offs[-1] + s)
        host = torch.empty(max(offs[-1], 1), dtype=torch.uint8, pin_memory=True)
        for i, s in enumerate(sz):
            host[offs[i]:offs[i + 1]].copy_(out[i, :s], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        yield f0, host, offs


def encode(frames: torch.Tensor, quality=95, subsampling: str = "444", layout: str | None = None, budget_bytes: int = BUDGET_BYTES) -> list:
    """Frames (the forms ``png.as_nchw`` accepts, RGB only; a host tensor is uploaded) -> one ``bytes`` object per frame, each a complete
    JPEG file.  ``quality``: 1..100, a number or one per frame."""
    files = []
    for _, host, offs in _encode_groups(frames, quality, subsampling, layout, budget_bytes):
        buf = host.numpy()
        files.extend(buf[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1))
    return files


def save_frames(frames: torch.Tensor, output_dir: str, names=None, quality=95, subsampling: str = "444", layout: str | None = None,
                budget_bytes: int = BUDGET_BYTES) -> list:
    """Encode on the GPU in frame groups and write ``output_dir/names[i]`` (default ``{i:03d}.jpg``, the PNG saver's naming); returns the
    paths."""
    os.makedirs(output_dir, exist_ok=True)
    paths = []
    for f0, host, offs in _encode_groups(frames, quality, subsampling, layout, budget_bytes):
        buf = host.numpy()
        for i in range(len(offs) - 1):
            name = names[f0 + i] if names is not None else f"{f0 + i:03d}.jpg"
            path = os.path.join(output_dir, name)
            with open(path, "wb") as f:
                f.write(memoryview(buf[offs[i]:offs[i + 1]]))
            paths.append(path)
    return paths


def save_avi(frames, path: str, fps: int = 16, quality=95, subsampling: str = "444", layout: str | None = None,
             budget_bytes: int = BUDGET_BYTES) -> int:
    """One Motion-JPEG ``.avi`` from ``frames``: a tensor, or an iterable of tensors (groups of frames of one size, in order), so a long
    clip need not be held at once.  Returns the number of frames written."""
    from . import avi
    if path == "-":
        raise avi.AviError("an AVI file has its sizes patched when it is closed: it needs a seekable file, not '-'")
    groups = [frames] if isinstance(frames, torch.Tensor) else frames
    writer, size = None, None
    try:
        for grp in groups:
            v = _rgb_nchw(grp, layout)
            if size is None:
                size = (int(v.shape[2]), int(v.shape[3]))
                writer = avi.MjpegAviWriter(path, size[1], size[0], fps)
            elif tuple(v.shape[2:]) != size:
                raise ValueError(f"save_avi: a group of {tuple(v.shape[2:])} frames in a clip of {size}")
            for _, host, offs in _encode_groups(v, quality, subsampling, "fchw", budget_bytes):
                buf = host.numpy()
                for i in range(len(offs) - 1):
                    writer.write(memoryview(buf[offs[i]:offs[i + 1]]))
        if writer is None:
            raise ValueError("save_avi: no frames")
        return writer.frames
    finally:
        if writer is not None:
            writer.close()


def main(argv=None):
    import argparse

    from . import prepost
    ap = argparse.ArgumentParser(description="PNG folders, .npy or .y4m clips -> .jpg folders or a Motion-JPEG .avi, encoded on the GPU")
    ap.add_argument("src", help="a PNG folder, an .npy clip (uint8 [F,H,W,3]) or a .y4m file")
    dst = ap.add_mutually_exclusive_group(required=True)
    dst.add_argument("--out", help="folder for 000.jpg, 001.jpg, ...")
    dst.add_argument("--avi", help="the .avi file to write")
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--fps", type=int, default=16)
    ap.add_argument("--subsampling", default="444", choices=("444", "420"))
    ap.add_argument("--yuv_matrix", default="bt601", choices=("bt601", "bt709"))
    ap.add_argument("--yuv_range", default=None, choices=("limited", "full"))
    args = ap.parse_args(argv)
    if not 1 <= args.quality <= 100:
        ap.error(f"--quality {args.quality} is not in 1..100")
    frames = prepost.load_frames(args.src, yuv_matrix=args.yuv_matrix, yuv_range=args.yuv_range)
    if args.out:
        paths = save_frames(frames, args.out, quality=args.quality, subsampling=args.subsampling)
        print(f"[dove_amd.jpeg] {len(paths)} files in {args.out}")
    else:
        n = save_avi(frames, args.avi, fps=args.fps, quality=args.quality, subsampling=args.subsampling)
        print(f"[dove_amd.jpeg] {n} frames in {args.avi} ({os.path.getsize(args.avi)} bytes)")


if __name__ == "__main__":
    main()
