"""float64 numpy restatement of the colour fix, written from the definitions - not from the kernel and not from the
reference's code: the yardstick of tests/test_colorfix_cpu.py (pinned there to the reference's recorded fp32 outputs) and of
tests/test_colorfix_gpu.py.

  B_r(x)[y, x] = sum_{i,j in -1,0,1} k[i] k[j] x[clamp(y + i r), clamp(x + j r)],  k = [1, 2, 1] / 4   (replicate padding by r)
  low5 = B_16 B_8 B_4 B_2 B_1
  wavelet(content, style) = (content - low5(content)) + low5(style) = content + low5(style - content)
  adain(content, style)   = (content - mean_c) / std_c * std_s + mean_s,  std = sqrt(unbiased variance + 1e-5), per image and channel
"""
import numpy as np

RADII = (1, 2, 4, 8, 16)


def blur_axis(x: np.ndarray, r: int, axis: int) -> np.ndarray:
    """[1,2,1]/4 along ``axis`` with taps at -r, 0, +r read at the clamped index."""
    n = x.shape[axis]
    i = np.arange(n)
    lo, hi = np.clip(i - r, 0, n - 1), np.clip(i + r, 0, n - 1)
    return 0.25 * np.take(x, lo, axis=axis) + 0.5 * x + 0.25 * np.take(x, hi, axis=axis)


def blur(x: np.ndarray, r: int) -> np.ndarray:
    """B_r on the last two axes."""
    return blur_axis(blur_axis(x, r, -1), r, -2)


def low5(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    for r in RADII:
        x = blur(x, r)
    return x


def wavelet(content, style) -> np.ndarray:
    """The difference form: one pyramid."""
    c, s = np.asarray(content, dtype=np.float64), np.asarray(style, dtype=np.float64)
    return c + low5(s - c)


def wavelet_two_pyramids(content, style) -> np.ndarray:
    """The reference's form: the content's high band as a running sum of five differences, plus the style's low band."""
    c, s = np.asarray(content, dtype=np.float64), np.asarray(style, dtype=np.float64)
    high, x = np.zeros_like(c), c
    for r in RADII:
        nxt = blur(x, r)
        high += x - nxt
        x = nxt
    return high + low5(s)


def mean_std(x: np.ndarray, eps: float = 1e-5):
    x = np.asarray(x, dtype=np.float64)
    flat = x.reshape(x.shape[0], x.shape[1], -1)
    mean = flat.mean(axis=2)
    var = ((flat - mean[..., None]) ** 2).sum(axis=2) / (flat.shape[2] - 1)
    return mean[..., None, None], np.sqrt(var + eps)[..., None, None]


def adain(content, style) -> np.ndarray:
    c = np.asarray(content, dtype=np.float64)
    mc, sc = mean_std(c)
    ms, ss = mean_std(style)
    return (c - mc) / sc * ss + ms


def fix(content, style, mode: str) -> np.ndarray:
    return {"wavelet": wavelet, "adain": adain}[mode](content, style)


def to_u8(x: np.ndarray) -> np.ndarray:
    """trunc(clamp(x, 0, 1) * 255), the rule of the savers."""
    return np.floor(np.clip(x, 0.0, 1.0) * 255.0).astype(np.uint8)


def u8_gate(got_u8: np.ndarray, want_u8: np.ndarray):
    """(largest level difference, share of pixels that differ at all)."""
    d = np.abs(got_u8.astype(np.int32) - want_u8.astype(np.int32))
    return int(d.max()), float((d > 0).mean())


def bf16_round(x: np.ndarray) -> np.ndarray:
    """float32 values rounded to the nearest bfloat16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def make_pair(rng, n: int, h: int, w: int):
    """content: a smooth random field plus noise; style: a tone-shifted, noisier copy.  Both in about [0,1] and rounded to bfloat16, so
    the same arrays feed a kernel as bf16 or fp32 without input error.  -> float32 [n,3,h,w] x 2"""
    gy, gx = max(h // 8, 2), max(w // 8, 2)
    coarse = rng.random((n, 3, gy, gx))
    yi = np.linspace(0, gy - 1, h)
    xi = np.linspace(0, gx - 1, w)
    y0, x0 = np.floor(yi).astype(int).clip(0, gy - 2), np.floor(xi).astype(int).clip(0, gx - 2)
    fy, fx = (yi - y0)[None, None, :, None], (xi - x0)[None, None, None, :]
    g = coarse[:, :, y0][:, :, :, x0] * (1 - fy) * (1 - fx) + coarse[:, :, y0 + 1][:, :, :, x0] * fy * (1 - fx) \
        + coarse[:, :, y0][:, :, :, x0 + 1] * (1 - fy) * fx + coarse[:, :, y0 + 1][:, :, :, x0 + 1] * fy * fx
    content = np.clip(0.15 + 0.7 * g + 0.04 * rng.standard_normal(g.shape), 0, 1)
    gain = np.array([0.85, 1.0, 1.1])[None, :, None, None]
    shift = np.array([0.06, -0.03, 0.02])[None, :, None, None]
    style = np.clip(content * gain + shift + 0.08 * rng.standard_normal(g.shape), 0, 1)
    return bf16_round(content.astype(np.float32)), bf16_round(style.astype(np.float32))
