"""NumPy definitions of the degradation operators (csrc/degrade.hip; include/dove_hip.h has them in words): float64 for blur, resize and
the noise arithmetic, integers for JPEG, where this file fixes every output byte.  Frames are [N,H,W,3] in the 0..255 scale."""
import numpy as np

import randn_ref

RESIZE_BILINEAR, RESIZE_BICUBIC, RESIZE_AREA = 0, 1, 2


# ---- blur -------------------------------------------------------------------------------------------------------------------------
def blur2d(x: np.ndarray, kernel: np.ndarray) -> np.ndarray:
    """cv2.filter2D(x, -1, kernel): correlation, centre anchor, BORDER_REFLECT_101.  kernel [k,k] or [N,k,k]."""
    x = np.asarray(x, dtype=np.float64)
    kernel = np.asarray(kernel, dtype=np.float64)
    N, H, W, _ = x.shape
    k = kernel.shape[-1]
    r = k // 2
    assert H > r and W > r
    kn = np.broadcast_to(kernel, (N, k, k))
    xp = np.pad(x, ((0, 0), (r, r), (r, r), (0, 0)), mode="reflect")          # numpy's "reflect" is dcb|abcd|cba
    out = np.zeros_like(x)
    for dy in range(k):
        for dx in range(k):
            out += kn[:, dy, dx, None, None, None] * xp[:, dy:dy + H, dx:dx + W]
    return out


def blur_tolerance(kernel: np.ndarray) -> float:
    """k*k fp32 FMAs of products bounded by sum|w| * 255, against the float64 sum: twice the first-order bound."""
    k = kernel.shape[-1]
    return 2 * k * k * 2.0 ** -24 * float(np.abs(np.asarray(kernel, dtype=np.float64)).reshape(-1, k * k).sum(1).max()) * 255


# ---- resize -----------------------------------------------------------------------------------------------------------------------
def cubic_weights(t: float):
    """Keys' cubic convolution, A = -0.75, at distances 1 + t, t, 1 - t, 2 - t."""
    A = -0.75

    def near(d):
        return ((A + 2) * d - (A + 3)) * d * d + 1

    def far(d):
        return ((A * d - 5 * A) * d + 8 * A) * d - 4 * A
    return [far(1 + t), near(t), near(1 - t), far(2 - t)]


def axis_matrix(n: int, on: int, mode: int) -> np.ndarray:
    """[on, n] float64 weights of one axis."""
    M = np.zeros((on, n))
    for i in range(on):
        if mode == RESIZE_AREA:
            lo, hi = i * n, (i + 1) * n                                        # the span in units of 1 / on
            for s in range(lo // on, -(-hi // on)):
                M[i, s] += (min(hi, (s + 1) * on) - max(lo, s * on)) / n
        else:
            num, den = (2 * i + 1) * n - on, 2 * on                            # half-pixel centre: exact floor and remainder
            i0, rem = num // den, num % den
            t = rem / den
            if mode == RESIZE_BILINEAR:
                taps = [(i0, 1 - t), (i0 + 1, t)]
            else:
                taps = list(zip(range(i0 - 1, i0 + 3), cubic_weights(t)))
            for s, wgt in taps:
                M[i, min(max(s, 0), n - 1)] += wgt                             # indices clamped at the border
    return M


def resize(x: np.ndarray, oh: int, ow: int, mode: int) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    if (oh, ow) == x.shape[1:3]:
        return x.copy()
    return np.einsum("ah,nhwc,bw->nabc", axis_matrix(x.shape[1], oh, mode), x, axis_matrix(x.shape[2], ow, mode))


def resize_tolerance(h: int, w: int, oh: int, ow: int, mode: int) -> float:
    """2 * (taps + 4) * 2^-24 * sum|w| * 255: the taps' FMAs plus the rounding of the fraction and the weights (the + 4)."""
    if mode == RESIZE_AREA:
        taps, sumw = (-(-h // oh) + 1) * (-(-w // ow) + 1), 1.0
    elif mode == RESIZE_BILINEAR:
        taps, sumw = 4, 1.0
    else:
        taps, sumw = 16, 1.375 ** 2                                            # sum|w| of one axis peaks at t = 1/2: 2 (0.59375 + 0.09375)
    return 2 * (taps + 4) * 2.0 ** -24 * sumw * 255


# ---- noise ------------------------------------------------------------------------------------------------------------------------
def gaussian_z(n: int, h: int, w: int, gray: bool, seed: int, stream_id: int, frame0: int) -> np.ndarray:
    """float64 normals [n,h,w,3]: colour - stream element = row-major index of (frame0 + i, y, x, c); gray - of (frame0 + i, y, x)."""
    per = h * w * (1 if gray else 3)
    z = randn_ref.randn(n * per, seed, stream_id, frame0 * per)
    return np.repeat(z.reshape(n, h, w, 1), 3, axis=3) if gray else z.reshape(n, h, w, 3)


def poisson_values(x: np.ndarray, gray: bool) -> np.ndarray:
    """clip(rint(x), 0, 255) as int - gray: of the float32 luma, products and sums rounded one by one, [N,H,W,1]."""
    x = np.asarray(x, dtype=np.float32)
    if gray:
        x = (np.float32(0.299) * x[..., 0] + np.float32(0.587) * x[..., 1] + np.float32(0.114) * x[..., 2])[..., None]
    return np.clip(np.rint(x), 0, 255).astype(np.int64)


def poisson_U(v_frame: np.ndarray) -> int:
    return int(2 ** np.ceil(np.log2(len(np.unique(v_frame)))))


# ---- JPEG -------------------------------------------------------------------------------------------------------------------------
# ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance)
JPEG_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
                      103, 99], dtype=np.int64).reshape(8, 8)
JPEG_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32, dtype=np.int64).reshape(8, 8)


def quant_table(base: np.ndarray, quality: int) -> np.ndarray:
    """libjpeg's quality rule."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * s + 50) // 100, 1, 255)


def dct_matrix() -> np.ndarray:
    """C[u][x] = rint(8192 s(u) cos((2x + 1) u pi / 16)), s(0) = 1 / sqrt(8), s(u) = 1 / 2."""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    s = np.where(u == 0, 1 / np.sqrt(8.0), 0.5)
    return np.rint(8192 * s * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


def _codec(plane: np.ndarray, Q: np.ndarray) -> np.ndarray:
    """8x8 blocks of an int plane (multiples of 8) through DCT, quantisation, dequantisation, IDCT; two passes each way, the first keeps
    two fractional bits, the second result carries 2^15."""
    C = dct_matrix()
    h, w = plane.shape
    f = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128                       # [by, bx, y, x]
    t = (np.einsum("abyx,ux->abyu", f, C) + 1024) >> 11
    F = np.einsum("abyu,vy->abvu", t, C)
    Qs = Q << 15
    coef = np.sign(F) * ((np.abs(F) + (Qs >> 1)) // Qs) * Q                                  # round half away from zero
    t = (np.einsum("abvu,ux->abvx", coef, C) + 1024) >> 11
    out = np.clip(((np.einsum("abvx,vy->abyx", t, C) + 16384) >> 15) + 128, 0, 255)
    assert max(np.abs(F).max(), np.abs(t).max()) < 2 ** 30                                   # the kernel's 32-bit accumulators
    return out.transpose(0, 2, 1, 3).reshape(h, w)


def _fancy_upsample(c: np.ndarray, H: int, W: int) -> np.ndarray:
    """libjpeg's h2v2 fancy upsampling of the real chroma extent [ceil(H/2), ceil(W/2)] -> [H, W]: 3:1 towards the nearer sample on each axis,
    the farther index clamped; (sum of 16ths + 8) >> 4 at even columns, + 7 at odd ones."""
    ch, cw = c.shape
    y, x = np.arange(H), np.arange(W)
    cy, cx = y >> 1, x >> 1
    oy = np.clip(np.where(y & 1, cy + 1, cy - 1), 0, ch - 1)
    ox = np.clip(np.where(x & 1, cx + 1, cx - 1), 0, cw - 1)
    v = 3 * c[cy] + c[oy]                                                                     # [H, cw]
    return (3 * v[:, cx] + v[:, ox] + np.where(x & 1, 7, 8)[None, :]) >> 4


def jpeg_frame(x: np.ndarray, quality: int) -> np.ndarray:
    p = np.clip(np.asarray(x, dtype=np.float32), 0, 255).astype(np.uint8).astype(np.int64)   # truncation, as the reference's astype
    H, W, _ = p.shape
    p = np.pad(p, ((0, -H % 16), (0, -W % 16), (0, 0)), mode="edge")
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16

    def down(c):                                     # 2x2 mean with libjpeg's alternating bias: + 1 at even columns, + 2 at odd ones
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        return (s + np.where(np.arange(s.shape[1]) & 1, 2, 1)[None, :]) >> 2
    ql, qc = quant_table(JPEG_LUMA, quality), quant_table(JPEG_CHROMA, quality)
    Y = _codec(Y, ql)[:H, :W]
    ch, cw = (H + 1) // 2, (W + 1) // 2
    cb = _fancy_upsample(_codec(down(cb), qc)[:ch, :cw], H, W) - 128
    cr = _fancy_upsample(_codec(down(cr), qc)[:ch, :cw], H, W) - 128
    out = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(out, 0, 255).astype(np.uint8)


def jpeg_roundtrip(x: np.ndarray, quality) -> np.ndarray:
    q = [quality] * len(x) if np.isscalar(quality) else list(quality)
    return np.stack([jpeg_frame(f, int(qi)) for f, qi in zip(x, q)])
