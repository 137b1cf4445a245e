"""numpy int64 restatement of csrc/yuv.hip: the normative definition of the RGB <-> YUV conversion.

Everything is integer fixed point with 16 fractional bits.  Coefficients are ``rint(c * 65536)`` of the float matrices below; a result
is rounded ONCE (``+ half`` before the final arithmetic shift, which floors) and clamped to 0..255.

Forward, per pixel with P = M_fwd @ (R, G, B) (no offset, un-rounded):
    Y = clamp((P0 + (off_y << 16) + 2^15) >> 16)
    444:  U = clamp((P1 + (128 << 16) + 2^15) >> 16)                                   (V from P2 alike)
    422:  S(i) = P1(2i-1) + 2 P1(2i) + P1(2i+1), x clamped to 0..W-1 ([1 2 1]/4, left co-sited)
    420:  S(i,j) = sum of P1 over luma rows 2j, 2j+1 and columns 2i, 2i+1, each clamped to the frame (centre-sited 2x2 mean)
          U = clamp((S + (128 << 18) + 2^17) >> 18)
A frame payload is the Y plane [H,W], then U, then V ([ceil(H/2) or H, ceil(W/2) or W]); mono is the Y plane alone.

Inverse: chroma is upsampled per axis with integer weights that sum to 4, neighbours clamped to the plane:
    centre-sited axis (420 vertical in every variant, 420jpeg horizontal): 3 C[i] + C[i -+ 1], i = x >> 1, the neighbour on the side of x
    left-sited axis (420mpeg2 / 420paldv / 422 horizontal):               4 C[i] at even x, 2 C[i] + 2 C[i+1] at odd x
so the upsampled chroma carries a scale 2^s (s = 4 for 420, 2 for 422, 0 for 444) into the matrix product:
    R = clamp((m00 ((Y - off_y) << s) + m01 (Us - (128 << s)) + m02 (Vs - (128 << s)) + 2^(15+s)) >> (16 + s))    (G, B alike)
mono: R = G = B = clamp((m00 (Y - off_y) + 2^15) >> 16).
420paldv's chroma rows are co-sited with alternating luma rows per plane in the DV standard; it is read here with the centred
vertical weights of the other 420 variants (an approximation of a quarter luma row)."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
CHROMAS = ("444", "422", "420", "mono")


def float_matrices(matrix: str, rng: str):
    """(forward 3x3, inverse 3x3, (off_y, 128, 128)) in float64."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc, oy = (219.0 / 255.0, 224.0 / 255.0, 16) if rng == "limited" else (1.0, 1.0, 0)
    fwd = np.array([[kr * sy, kg * sy, kb * sy],
                    [-0.5 * kr / (1 - kb) * sc, -0.5 * kg / (1 - kb) * sc, 0.5 * sc],
                    [0.5 * sc, -0.5 * kg / (1 - kr) * sc, -0.5 * kb / (1 - kr) * sc]], dtype=np.float64)
    inv = np.array([[1 / sy, 0.0, 2 * (1 - kr) / sc],
                    [1 / sy, -2 * kb * (1 - kb) / kg / sc, -2 * kr * (1 - kr) / kg / sc],
                    [1 / sy, 2 * (1 - kb) / sc, 0.0]], dtype=np.float64)
    return fwd, inv, (oy, 128, 128)


def int_matrices(matrix: str, rng: str):
    fwd, inv, off = float_matrices(matrix, rng)
    return np.rint(fwd * 65536).astype(np.int64), np.rint(inv * 65536).astype(np.int64), off


def chroma_shape(h: int, w: int, chroma: str):
    if chroma == "444":
        return h, w
    if chroma == "422":
        return h, (w + 1) // 2
    if chroma == "420":
        return (h + 1) // 2, (w + 1) // 2
    return 0, 0


def frame_bytes(h: int, w: int, chroma: str) -> int:
    ch, cw = chroma_shape(h, w, chroma)
    return h * w + 2 * ch * cw


def quantise(x: np.ndarray) -> np.ndarray:
    """float in [0,1] -> uint8 as dove_postprocess_u8: trunc(clamp(x * 255, 0, 255)) in fp32."""
    v = x.astype(np.float32) * np.float32(255.0)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, 0, 255).astype(np.uint8)


def _u8(v, shift):
    return np.clip(v >> shift, 0, 255).astype(np.uint8)


def rgb_to_yuv(rgb: np.ndarray, matrix: str = "bt601", rng: str = "limited", chroma: str = "444") -> np.ndarray:
    """[F,H,W,3] uint8 -> [F, frame_bytes] uint8 Y4M frame payloads."""
    assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3
    F, H, W, _ = rgb.shape
    M, _, off = int_matrices(matrix, rng)
    P = rgb.astype(np.int64) @ M.T                                              # [F,H,W,3], exact
    Y = _u8(P[..., 0] + (off[0] << 16) + (1 << 15), 16)
    if chroma == "mono":
        return Y.reshape(F, -1)
    C = P[..., 1:]
    if chroma == "444":
        UV = _u8(C + (128 << 16) + (1 << 15), 16)
    else:
        if chroma == "422":
            Cp = np.pad(C, ((0, 0), (0, 0), (1, 1), (0, 0)), mode="edge")
            xs = np.arange(0, W, 2)
            S = Cp[:, :, xs] + 2 * Cp[:, :, xs + 1] + Cp[:, :, xs + 2]
        else:
            Cp = np.pad(C, ((0, 0), (0, H % 2), (0, W % 2), (0, 0)), mode="edge")
            S = Cp[:, 0::2, 0::2] + Cp[:, 0::2, 1::2] + Cp[:, 1::2, 0::2] + Cp[:, 1::2, 1::2]
        UV = _u8(S + (128 << 18) + (1 << 17), 18)
    return np.concatenate([Y.reshape(F, -1), UV[..., 0].reshape(F, -1), UV[..., 1].reshape(F, -1)], axis=1)


def _up_axis(C: np.ndarray, axis: int, n_out: int, centre: bool) -> np.ndarray:
    """Upsample one axis by 2 to n_out samples; the result is scaled by 4."""
    x = np.arange(n_out)
    i = x >> 1
    odd = (x & 1).astype(bool)
    last = C.shape[axis] - 1
    shape = [1] * C.ndim
    shape[axis] = n_out
    if centre:
        other = np.clip(np.where(odd, i + 1, i - 1), 0, last)
        return 3 * np.take(C, i, axis) + np.take(C, other, axis)
    nxt = np.clip(i + 1, 0, last)
    return np.where(odd.reshape(shape), 2 * np.take(C, i, axis) + 2 * np.take(C, nxt, axis), 4 * np.take(C, i, axis))


def yuv_to_rgb(payload: np.ndarray, h: int, w: int, matrix: str = "bt601", rng: str = "limited", chroma: str = "444",
               siting_h: str = "centre") -> np.ndarray:
    """[F, frame_bytes] uint8 -> [F,H,W,3] uint8.  ``siting_h``: 'centre' (420jpeg) or 'left' (420mpeg2, 420paldv); 422 is always left."""
    assert payload.dtype == np.uint8 and payload.ndim == 2 and payload.shape[1] == frame_bytes(h, w, chroma)
    F = payload.shape[0]
    _, M, off = int_matrices(matrix, rng)
    Y = payload[:, :h * w].reshape(F, h, w).astype(np.int64) - off[0]
    if chroma == "mono":
        g = _u8(M[0, 0] * Y + (1 << 15), 16)
        return np.stack([g, g, g], axis=-1)
    ch, cw = chroma_shape(h, w, chroma)
    UV = payload[:, h * w:].reshape(F, 2, ch, cw).astype(np.int64)
    s = 0
    if chroma == "422":
        UV, s = _up_axis(UV, 3, w, False), 2
    elif chroma == "420":
        UV, s = _up_axis(_up_axis(UV, 2, h, True), 3, w, siting_h == "centre"), 4
    UV = UV - (128 << s)
    YUV = np.stack([Y << s, UV[:, 0], UV[:, 1]], axis=-1)                        # [F,H,W,3]
    return _u8(YUV @ M.T + (1 << (15 + s)), 16 + s)


# Y4M colourspace tag -> (chroma, horizontal siting)
TAGS = {"C420jpeg": ("420", "centre"), "C420": ("420", "centre"), "C420mpeg2": ("420", "left"), "C420paldv": ("420", "left"),
        "C422": ("422", "left"), "C444": ("444", "left"), "Cmono": ("mono", "left")}
