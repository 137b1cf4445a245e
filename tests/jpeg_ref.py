"""The byte-exact definition of the GPU JPEG encoder (csrc/jpeg.hip): baseline sequential JFIF, 8-bit, YCbCr 4:2:0 or
4:4:4, the Annex-K Huffman tables, one restart interval per ``restart_mcus`` MCUs.  The forward half (colour matrix, edge replication, chroma
mean, integer DCT, quantiser) is ``degrade_ref``'s; this file adds what follows the quantiser, a Huffman decoder that is independent of the
encoder's tables (it builds its own from the file's DHT segments), and the definition's own pixel decode."""
import numpy as np

import degrade_ref as D

RESTART_MCUS = 8                                      # dove_jpeg_restart_mcus()
# max |Pillow's decode - decode_pixels| over KINDS x SHAPES x QUALITIES below, both subsamplings, measured with Pillow 12.2 (libjpeg-turbo):
# 3 grey levels (libjpeg's IDCT, upsampling and colour conversion round differently).  Tests assert measured + 1, for another libjpeg build.
PILLOW_MEASURED = 3
PILLOW_BOUND = PILLOW_MEASURED + 1

# zigzag position k -> natural index 8 v + u
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63])

# ITU-T T.81 Annex K, tables K.3 - K.6: (number of codes of each length 1..16, symbols in code order)
def _rows(first_sizes):
    """The run/size symbols that end both AC tables: for each run r, sizes first_sizes[r]..10 in order."""
    return [0x10 * r + s for r in range(16) for s in range(first_sizes[r], 11)]


DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
            0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82]
           + [s for s in _rows([9, 6, 5, 4, 3, 3, 3, 3, 3, 2, 2, 2, 2, 2, 1, 1])])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
              0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
              0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A]
             + [s for s in _rows([11, 11, 11, 5, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2])])
TABLES = {"dc_luma": DC_LUMA, "dc_chroma": DC_CHROMA, "ac_luma": AC_LUMA, "ac_chroma": AC_CHROMA}


def huffman_codes(bits, vals):
    """T.81 Annex C: symbol -> (code, length) of the canonical code."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def geometry(H: int, W: int, subsampling: str):
    """(MCU size in pixels, blocks per MCU, MCU rows, MCU columns)."""
    if subsampling not in ("420", "444"):
        raise ValueError(f"subsampling {subsampling!r}: '420' or '444'")
    m = 16 if subsampling == "420" else 8
    return m, 6 if subsampling == "420" else 3, -(-H // m), -(-W // m)


def _planes(frame_u8: np.ndarray, subsampling: str):
    """Y, Cb, Cr int planes, edge-replicated to whole MCUs; chroma halved for 4:2:0 (degrade_ref.jpeg_frame's arithmetic)."""
    p = np.asarray(frame_u8, dtype=np.uint8).astype(np.int64)
    H, W, _ = p.shape
    m = geometry(H, W, subsampling)[0]
    p = np.pad(p, ((0, -H % m), (0, -W % m), (0, 0)), mode="edge")
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    if subsampling == "420":
        def down(c):
            s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
            return (s + np.where(np.arange(s.shape[1]) & 1, 2, 1)[None, :]) >> 2
        cb, cr = down(cb), down(cr)
    return Y, cb, cr


def _plane_levels(plane: np.ndarray, Q: np.ndarray) -> np.ndarray:
    """[by, bx, v, u] quantised levels of an int plane: the forward half of degrade_ref._codec, then the baseline clamp."""
    C = D.dct_matrix()
    h, w = plane.shape
    f = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128
    t = (np.einsum("abyx,ux->abyu", f, C) + 1024) >> 11
    F = np.einsum("abyu,vy->abvu", t, C)
    Qs = Q << 15
    lev = np.sign(F) * ((np.abs(F) + (Qs >> 1)) // Qs)
    lev = np.clip(lev, -1023, 1023)                                           # AC: size categories 1..10
    lev[..., 0, 0] = np.clip(np.sign(F[..., 0, 0]) * ((np.abs(F[..., 0, 0]) + (Qs[0, 0] >> 1)) // Qs[0, 0]), -1024, 1023)
    return lev


def levels(frame_u8: np.ndarray, quality: int, subsampling: str = "420") -> np.ndarray:
    """uint8 [H,W,3] -> int64 [MCU rows, MCU columns, blocks per MCU, 8, 8] quantised levels in natural [v][u] order; the blocks of an MCU
    are Y00 Y01 Y10 Y11 Cb Cr (4:2:0) or Y Cb Cr (4:4:4).

    The clamp sits directly after the quantiser, before DC prediction: AC levels to -1023..1023 (size category 10 at most) and DC levels to
    -1024..1023, so that every DC difference lies in -2047..2047 (category 11 at most).  With 8-bit samples neither clamp ever binds (the
    DC level of this DCT spans -1024..1016 and |AC| stays below 930); it is there so that the coder's tables cover every input."""
    H, W, _ = frame_u8.shape
    m, B, My, Mx = geometry(H, W, subsampling)
    Y, cb, cr = _planes(frame_u8, subsampling)
    ql, qc = D.quant_table(D.JPEG_LUMA, quality), D.quant_table(D.JPEG_CHROMA, quality)
    ly, lb, lr = _plane_levels(Y, ql), _plane_levels(cb, qc), _plane_levels(cr, qc)
    out = np.zeros((My, Mx, B, 8, 8), dtype=np.int64)
    if subsampling == "420":
        for k in range(4):
            out[:, :, k] = ly[k >> 1::2, k & 1::2]
        out[:, :, 4], out[:, :, 5] = lb, lr
    else:
        out[:, :, 0], out[:, :, 1], out[:, :, 2] = ly, lb, lr
    return out


def decode_pixels(lev: np.ndarray, H: int, W: int, quality: int, subsampling: str = "420") -> np.ndarray:
    """The definition's own decode of ``levels``: dequantise, degrade_ref's integer inverse DCT, fancy upsampling for 4:2:0 (none for
    4:4:4), JFIF YCbCr -> RGB.  For 4:2:0 this is the inverse half of degrade_ref.jpeg_frame."""
    C = D.dct_matrix()
    ql, qc = D.quant_table(D.JPEG_LUMA, quality), D.quant_table(D.JPEG_CHROMA, quality)
    My, Mx, B = lev.shape[:3]

    def inverse(blocks, Q):                                                   # [by, bx, v, u] -> plane
        t = (np.einsum("abvu,ux->abvx", blocks * Q, C) + 1024) >> 11
        out = np.clip(((np.einsum("abvx,vy->abyx", t, C) + 16384) >> 15) + 128, 0, 255)
        return out.transpose(0, 2, 1, 3).reshape(out.shape[0] * 8, out.shape[1] * 8)
    if subsampling == "420":
        ly = np.zeros((My * 2, Mx * 2, 8, 8), dtype=np.int64)
        for k in range(4):
            ly[k >> 1::2, k & 1::2] = lev[:, :, k]
        Y = inverse(ly, ql)[:H, :W]
        ch, cw = (H + 1) // 2, (W + 1) // 2
        cb = D._fancy_upsample(inverse(lev[:, :, 4], qc)[:ch, :cw], H, W) - 128
        cr = D._fancy_upsample(inverse(lev[:, :, 5], qc)[:ch, :cw], H, W) - 128
    else:
        Y = inverse(lev[:, :, 0], ql)[:H, :W]
        cb = inverse(lev[:, :, 1], qc)[:H, :W] - 128
        cr = inverse(lev[:, :, 2], qc)[:H, :W] - 128
    out = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(out, 0, 255).astype(np.uint8)


# ---- the stream -------------------------------------------------------------------------------------------------------------------------
def _seg(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(H: int, W: int, quality: int, subsampling: str, restart_mcus: int) -> bytes:
    """Everything before the entropy-coded data: SOI, APP0, two DQT, SOF0, four DHT, DRI, SOS."""
    geometry(H, W, subsampling)
    ql, qc = D.quant_table(D.JPEG_LUMA, quality), D.quant_table(D.JPEG_CHROMA, quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))       # 1.01, no units, density 1:1, no thumbnail
    for tq, q in ((0, ql), (1, qc)):
        out += _seg(0xDB, bytes([tq]) + bytes(int(v) for v in q.reshape(64)[ZIGZAG]))
    ys = 0x22 if subsampling == "420" else 0x11
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, ys, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, name in ((0x00, "dc_luma"), (0x10, "ac_luma"), (0x01, "dc_chroma"), (0x11, "ac_chroma")):
        bits, vals = TABLES[name]
        out += _seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _seg(0xDD, restart_mcus.to_bytes(2, "big"))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def _size(v: int) -> int:
    return int(abs(v)).bit_length()


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code: int, length: int):
        self.acc = (self.acc << length) | code
        self.n += length

    def finish(self) -> bytes:
        """Pad with 1-bits to a byte, then follow every 0xFF by 0x00."""
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        return self.acc.to_bytes(self.n // 8, "big").replace(b"\xff", b"\xff\x00")


def _code_block(bw: _Bits, zz, pred: int, dc, ac) -> int:
    diff = int(zz[0]) - pred
    s = _size(diff)
    bw.put(*dc[s])
    if s:
        bw.put(diff if diff > 0 else diff + (1 << s) - 1, s)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        s = _size(v)
        bw.put(*ac[(run << 4) | s])
        bw.put(v if v > 0 else v + (1 << s) - 1, s)
        run = 0
    if run:
        bw.put(*ac[0x00])
    return int(zz[0])


def encode_levels(lev: np.ndarray, H: int, W: int, quality: int, subsampling: str = "420", restart_mcus: int = RESTART_MCUS,
                  bit_counts: list = None) -> bytes:
    """``bit_counts``, if given, receives each interval's bits before padding."""
    My, Mx, B = lev.shape[:3]
    codes = {k: huffman_codes(*v) for k, v in TABLES.items()}
    zz = lev.reshape(My * Mx, B, 64)[:, :, ZIGZAG]
    comp = [0, 0, 0, 0, 1, 2] if B == 6 else [0, 1, 2]
    out = [header(H, W, quality, subsampling, restart_mcus)]
    n_int = -(-My * Mx // restart_mcus)
    for m in range(n_int):
        bw, pred = _Bits(), [0, 0, 0]
        for mcu in range(m * restart_mcus, min((m + 1) * restart_mcus, My * Mx)):
            for b in range(B):
                c = comp[b]
                pred[c] = _code_block(bw, zz[mcu, b], pred[c], codes["dc_luma" if c == 0 else "dc_chroma"],
                                      codes["ac_luma" if c == 0 else "ac_chroma"])
        if bit_counts is not None:
            bit_counts.append(bw.n)
        out.append(bw.finish())
        out.append(bytes([0xFF, 0xD0 + (m & 7)]) if m < n_int - 1 else b"\xff\xd9")
    return b"".join(out)


def encode(frame_u8: np.ndarray, quality: int, subsampling: str = "420", restart_mcus: int = RESTART_MCUS) -> bytes:
    """uint8 [H,W,3] -> the complete file."""
    H, W, _ = frame_u8.shape
    return encode_levels(levels(frame_u8, quality, subsampling), H, W, quality, subsampling, restart_mcus)


# ---- an independent Huffman decoder ---------------------------------------------------------------------------------------------------
def decode_levels(data: bytes) -> np.ndarray:
    """A baseline JFIF file as ``encode`` writes them -> the levels, [MCU rows, MCU columns, blocks per MCU, 8, 8].  The Huffman tables,
    sampling factors, restart interval and size are all read from the file."""
    assert data[:2] == b"\xff\xd8"
    pos, tables, ri, comps = 2, {}, 0, None
    while True:
        assert data[pos] == 0xFF, hex(data[pos])
        marker, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if marker == 0xC4:
            while body:
                bits = list(body[1:17])
                cnt = sum(bits)
                lut, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(bits[length - 1]):
                        lut[(length, code)] = body[17 + k]
                        code += 1
                        k += 1
                    code <<= 1
                tables[body[0]] = lut
                body = body[17 + cnt:]
        elif marker == 0xC0:
            assert body[0] == 8 and body[5] == 3
            H, W = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            comps = [(body[6 + 3 * i], body[7 + 3 * i]) for i in range(3)]
        elif marker == 0xDD:
            ri = int.from_bytes(body, "big")
        elif marker == 0xDA:
            sel = {body[1 + 2 * i]: body[2 + 2 * i] for i in range(3)}
            break
    hv = [(s >> 4, s & 15) for _, s in comps]
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    My, Mx = -(-H // (8 * vmax)), -(-W // (8 * hmax))
    order = [c for c, (h, v) in enumerate(hv) for _ in range(h * v)]
    out = np.zeros((My * Mx, len(order), 64), dtype=np.int64)

    # un-stuff and split at the restart markers
    intervals, cur, i = [], bytearray(), pos
    while True:
        b = data[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
        elif data[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif 0xD0 <= data[i + 1] <= 0xD7:
            assert data[i + 1] == 0xD0 + (len(intervals) & 7), "restart markers out of order"
            intervals.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            assert data[i + 1] == 0xD9 and i + 2 == len(data), "expected EOI at the end"
            intervals.append(bytes(cur))
            break
    assert ri > 0 and len(intervals) == -(-My * Mx // ri)

    for m, chunk in enumerate(intervals):
        acc, nbits, p = int.from_bytes(chunk, "big"), 8 * len(chunk), 0

        def take(n):
            nonlocal p
            assert p + n <= nbits, "ran past the interval"
            v = (acc >> (nbits - p - n)) & ((1 << n) - 1)
            p += n
            return v

        def symbol(lut):
            code = 0
            for length in range(1, 17):
                code = (code << 1) | take(1)
                if (length, code) in lut:
                    return lut[(length, code)]
            raise AssertionError("no Huffman code matches")

        def extend(s):
            if s == 0:
                return 0
            v = take(s)
            return v if v >> (s - 1) else v - (1 << s) + 1
        pred = [0, 0, 0]
        for mcu in range(m * ri, min((m + 1) * ri, My * Mx)):
            for b, c in enumerate(order):
                ts = sel[comps[c][0]]
                pred[c] += extend(symbol(tables[ts >> 4]))
                out[mcu, b, 0] = pred[c]
                k = 1
                while k < 64:
                    rs = symbol(tables[0x10 | (ts & 15)])
                    if rs == 0:
                        break
                    if rs == 0xF0:
                        k += 16
                        continue
                    k += rs >> 4
                    out[mcu, b, k] = extend(rs & 15)
                    k += 1
                assert k <= 64
        rest = nbits - p
        assert rest < 8 and take(rest) == (1 << rest) - 1, "padding is not 1-bits to the byte"
    nat = np.zeros_like(out)
    nat[:, :, ZIGZAG] = out
    return nat.reshape(My, Mx, len(order), 8, 8)


# ---- test inputs -------------------------------------------------------------------------------------------------------------------------
KINDS = ("noise", "ramp", "flat", "binary", "smooth")
SHAPES = ((1, 1), (8, 8), (16, 16), (17, 33), (40, 56), (31, 250))
QUALITIES = (1, 10, 50, 75, 95, 100)


def image(h: int, w: int, kind: str, seed: int = 0) -> np.ndarray:
    """uint8 [h,w,3]: uniform noise, a two-axis ramp, one flat colour, random 0/255 samples, or smooth sinusoids."""
    g = np.random.default_rng([seed, h, w, KINDS.index(kind)])
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(h + w - 2, 1)], -1).astype(np.uint8)
    if kind == "flat":
        return np.broadcast_to(g.integers(0, 256, size=3, dtype=np.uint8), (h, w, 3)).copy()
    if kind == "binary":
        return (g.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    if kind == "smooth":
        ph = g.random((3, 3)) * 6.283
        return np.stack([127.5 + 127.5 * np.sin(x / (3.0 + 2 * c) + ph[c, 0]) * np.cos(y / (4.0 + c) + ph[c, 1]) for c in range(3)],
                        -1).astype(np.uint8)
    raise ValueError(kind)


def basis_frame(h: int, w: int, v: int, u: int) -> np.ndarray:
    """0/255 samples following the sign of the 8x8 DCT basis function (v, u), tiled: the largest level that coefficient can take.  (0, 0)
    alternates whole blocks of 0 and 255 instead: the largest DC differences."""
    y, x = np.mgrid[0:h, 0:w]
    if (v, u) == (0, 0):
        s = ((y >> 3) + (x >> 3)) & 1
    else:
        s = np.cos((2 * (y & 7) + 1) * v * np.pi / 16) * np.cos((2 * (x & 7) + 1) * u * np.pi / 16) > 0
    return np.repeat((s * 255).astype(np.uint8)[..., None], 3, axis=2)
