"""numpy / zlib restatement of what csrc/png.hip writes: the bit-exact definition of the filtered stream, a chunk
parser that checks every CRC, and the size bounds the GPU tests hold the encoder to."""
import math
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def filtered_rows(img: np.ndarray):
    """img uint8 [H,W,C] -> (filter id per row [H], filtered bytes [H, W*C]).  Per scanline the filter (0 None, 1 Sub, 2 Up, 3 Average,
    4 Paeth; left / upper / upper-left neighbours outside the image are 0) with the smallest sum of |filtered byte read as int8|; ties go
    to the lower id (libpng's heuristic)."""
    H, W, C = img.shape
    x = img.reshape(H, W * C).astype(np.int32)
    a = np.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, C:] = x[:-1, :-C]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255            # [5,H,rb]
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)                          # [5,H]
    best = np.argmin(cost, axis=0)                                                     # the first minimum: ties to the lower id
    rows = np.take_along_axis(cand, best[None, :, None], axis=0)[0]
    return best.astype(np.uint8), rows.astype(np.uint8)


def filtered_stream(img: np.ndarray) -> bytes:
    """img uint8 [H,W,C] (or [H,W]) -> the bytes a PNG's zlib stream inflates to: per row the filter-type byte, then the filtered bytes."""
    if img.ndim == 2:
        img = img[:, :, None]
    best, rows = filtered_rows(img)
    return np.concatenate([best[:, None], rows], axis=1).tobytes()


def chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def wrap(filtered: bytes, h: int, w: int, channels: int) -> bytes:
    """A PNG file around a filtered stream, deflated by zlib itself."""
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if channels == 3 else 0, 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(filtered)) + chunk(b"IEND", b"")


def parse(data: bytes):
    """A PNG file -> (IHDR fields dict, concatenated IDAT data, number of IDAT chunks); every CRC is checked, the chunk order too."""
    assert data[:8] == SIGNATURE, "bad signature"
    pos, kinds, idat, ihdr = 8, [], [], None
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert len(body) == n, "truncated chunk"
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body), f"bad CRC in {kind!r} chunk at {pos}"
        kinds.append(kind)
        if kind == b"IHDR":
            w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            ihdr = dict(width=w, height=h, depth=depth, colour_type=ctype, compression=comp, filter=filt, interlace=lace)
        elif kind == b"IDAT":
            idat.append(body)
        pos += 12 + n
    assert pos == len(data), "bytes after the last chunk"
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"}, kinds
    return ihdr, b"".join(idat), len(idat)


def segments(filtered: bytes, R: int, row_bytes: int):
    """The filtered stream cut into segments of R whole rows (row_bytes includes the filter byte)."""
    step = R * row_bytes
    return [filtered[i:i + step] for i in range(0, len(filtered), step)]


def segment_entropy_bytes(seg: bytes) -> float:
    """(H0 n + n) / 8 + 256: n = the segment's symbols including end-of-block, H0 their zeroth-order entropy in bits per symbol.  A Huffman
    code is within one bit per symbol of H0; 256 covers the block header (<= 235 bytes), the 5-byte flush and a 12-byte chunk frame."""
    counts = np.bincount(np.frombuffer(seg, np.uint8), minlength=256).astype(np.float64)
    counts = np.append(counts[counts > 0], 1.0)
    n = counts.sum()
    h0 = float(-(counts / n * np.log2(counts / n)).sum())
    return (h0 * n + n) / 8 + 256


def entropy_bound(filtered: bytes, R: int, row_bytes: int) -> float:
    return sum(segment_entropy_bytes(s) for s in segments(filtered, R, row_bytes)) + 64


def flat_code_size(filtered: bytes, R: int, row_bytes: int) -> int:
    """The most bytes a file takes when every segment uses the flat code (8 bits for 0..254, 9 for 255 and end-of-block): per segment a
    header of at most 235 bytes, the codes, the 3-bit stored-block header padded to a byte, 4 bytes LEN / NLEN and the 12-byte chunk frame;
    per file the signature, IHDR, IEND, the 2-byte stream header and the 6-byte tail."""
    total = 8 + 25 + 12 + 2 + 6
    for s in segments(filtered, R, row_bytes):
        bits = 235 * 8 + 8 * len(s) + s.count(b"\xff") + 9 + 3
        total += math.ceil(bits / 8) + 4 + 12
    return total


def images(h: int, w: int, c: int, kind: str, frames: int = 3, seed: int = 0) -> np.ndarray:
    """uint8 [frames,h,w,c] test content: 'smooth' (a smooth field plus a 4 x 4 texture plus noise), 'noise' (uniform), 'zeros', 'ones'
    (all 255), 'hramp', 'vramp'."""
    g = np.random.default_rng(seed * 7919 + h * 131 + w * 17 + c)
    if kind == "noise":
        return g.integers(0, 256, size=(frames, h, w, c), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((frames, h, w, c), np.uint8)
    if kind == "ones":
        return np.full((frames, h, w, c), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "hramp":
        v = np.broadcast_to((xx * 3)[None, :, :, None] + np.arange(frames)[:, None, None, None], (frames, h, w, c))
        return (v.astype(np.int64) & 255).astype(np.uint8)
    if kind == "vramp":
        v = np.broadcast_to((yy * 5)[None, :, :, None] + np.arange(c)[None, None, None, :] * 40, (frames, h, w, c))
        return (v.astype(np.int64) & 255).astype(np.uint8)
    if kind == "smooth":
        out = np.empty((frames, h, w, c), np.uint8)
        for f in range(frames):
            for ch in range(c):
                field = 128 + 90 * np.sin(xx / 23.0 + f + ch) * np.cos(yy / 17.0 - ch)
                tex = 12 * (((xx.astype(int) // 4) + (yy.astype(int) // 4)) % 2)
                out[f, :, :, ch] = np.clip(field + tex + g.normal(0, 4, size=(h, w)), 0, 255).astype(np.uint8)
        return out
    raise ValueError(kind)


KINDS = ("smooth", "noise", "zeros", "ones", "hramp", "vramp")
