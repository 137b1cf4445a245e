"""NumPy restatement of the library's counter-based normal generator (csrc/video.hip: dove_philox_u32, dove_randn; include/dove_hip.h
has the definition in words).  The integer part is exact; the normals are evaluated in float64, which the float32 kernel is held
against with the tolerance tests/test_randn_gpu.py documents."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(block: np.ndarray, stream_id: int, seed: int) -> np.ndarray:
    """uint64 block indices [n] -> uint32 words [n, 4].  Key = (seed low, seed high); counter = (block low, block high, stream low,
    stream high)."""
    block = np.asarray(block, dtype=np.uint64)
    c0, c1 = block & MASK, block >> np.uint64(32)
    c2 = np.full_like(block, stream_id & 0xFFFFFFFF)
    c3 = np.full_like(block, (stream_id >> 32) & 0xFFFFFFFF)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def _blocks(n: int, offset: int):
    first, last = offset // 4, (offset + n - 1) // 4
    # np.arange in uint64 keeps block indices above 2^53 exact
    return np.arange(last - first + 1, dtype=np.uint64) + np.uint64(first), offset - 4 * first


def words(n: int, seed: int, stream_id: int = 0, offset: int = 0) -> np.ndarray:
    """The uint32 elements [offset, offset + n) of stream (seed, stream_id): element e is word e % 4 of block e // 4."""
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    blocks, skip = _blocks(n, offset)
    return philox4x32_10(blocks, stream_id, seed).reshape(-1)[skip:skip + n]


def box_muller(w: np.ndarray) -> np.ndarray:
    """uint32 words [n, 4] -> float64 normals [n, 4]: (x0, x1) and (x2, x3) are one pair each, u1 = (xa + 1) 2^-32, u2 = xb 2^-32,
    (r cos 2 pi u2, r sin 2 pi u2) with r = sqrt(-2 ln u1)."""
    w = w.astype(np.float64)
    out = np.empty_like(w)
    for a in (0, 2):
        u1, u2 = (w[:, a] + 1.0) / 2.0 ** 32, w[:, a + 1] / 2.0 ** 32
        r = np.sqrt(-2.0 * np.log(u1))
        out[:, a], out[:, a + 1] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return out


def randn(n: int, seed: int, stream_id: int = 0, offset: int = 0) -> np.ndarray:
    """float64 normals: the elements [offset, offset + n) of stream (seed, stream_id)."""
    if n == 0:
        return np.zeros(0)
    blocks, skip = _blocks(n, offset)
    return box_muller(philox4x32_10(blocks, stream_id, seed)).reshape(-1)[skip:skip + n]
