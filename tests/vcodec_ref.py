"""numpy int64 definition of the video-compression step (csrc/vcodec.hip): the GPU reproduces every byte, every
chosen QP and every bit count of this file.

``vcodec_roundtrip(x, bitrate, gop)`` does to the pixels what a hybrid motion-compensated transform codec does, without writing a
bitstream:

  intake    u = trunc(clip(x, 0, 255)); edge replication to multiples of 16; BT.601 limited-range Y'CbCr 4:2:0 by yuv_ref.rgb_to_yuv
            (2x2 mean, centre-sited); at the end yuv_ref.yuv_to_rgb with siting SITING, cropped to the input size.
  structure closed groups of ``gop`` frames (the last may be shorter).  The first frame of a group is an I frame, predicted as PRED_I
            everywhere; the others are P frames predicted from the previous *reconstructed* frame; no intra macroblocks in P frames.
  motion    per 16x16 luma macroblock a full search over integer (dy, dx) in [-SEARCH, SEARCH]^2 on the edge-replicated reference:
            pred[y, x] = ref[y + dy, x + dx], cost = SAD + LAMBDA (se_len(dx) + se_len(dy)), the winner is the lexicographic minimum
            of (cost, |dy| + |dx|, dy, dx).  Chroma 8x8 blocks move by (dy / 2, dx / 2): the floor and ceil neighbours of each axis
            (the same sample when the coordinate is whole), (a + b + c + d + 2) >> 2.
  residual  the H.264 4x4 core transform and quantiser on every 4x4 block of the three planes at one QP in 0..51, no DC Hadamard
            stage: W = CF X CF^T; Z = sign(W) ((|W| MF[QP % 6][class] + f) >> (15 + QP // 6)), f = 2^qbits // 3 (I) or // 6 (P);
            W' = (Z V[QP % 6][class]) << (QP // 6); the inverse butterflies on rows, then on columns, then (t + 32) >> 6;
            reconstruction = clip(pred + residual', 0, 255).
  bits      an integer model: an all-zero 4x4 block costs 1 bit, another 1 + ue_len(nnz - 1) + sum over its non-zero levels in
            zigzag order of ue_len(run of zeros before it) + se_len(level); a P macroblock adds se_len(dx) + se_len(dy).
  rate      per group: budget = bitrate * frames; lo, hi = 0, 51; while lo < hi: mid = (lo + hi) // 2, code the group at mid,
            bits <= budget ? hi = mid : lo = mid + 1.  The group's output is its coding at lo - the procedure is the definition,
            whether bits(QP) is monotone or not.

Not modelled: sub-pel motion, B frames, intra macroblocks in P frames, the deblocking filter, entropy coding, and any difference between
codec names."""
import numpy as np

import yuv_ref

MB = 16
SEARCH = 7
LAMBDA = 4
PRED_I = 128
QP_MIN, QP_MAX = 0, 51
MATRIX, RANGE, SITING = "bt601", "limited", "centre"
CF = np.array([[1, 1, 1, 1], [2, 1, -1, -2], [1, -1, -1, 1], [1, -2, 2, -1]], dtype=np.int64)
MF = np.array([(13107, 5243, 8066), (11916, 4660, 7490), (10082, 4194, 6554), (9362, 3647, 5825), (8192, 3355, 5243), (7282, 2893, 4559)],
              dtype=np.int64)                                    # rows QP % 6, columns class a, b, c
V = np.array([(10, 16, 13), (11, 18, 14), (13, 20, 16), (14, 23, 18), (16, 25, 20), (18, 29, 23)], dtype=np.int64)
ZIGZAG = np.array([0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15])          # raster index (4 row + col) of the k-th coefficient
# class of coefficient (i, j): a = 0 at (even, even), b = 1 at (odd, odd), c = 2 elsewhere
CLASS = np.array([[0 if i % 2 == 0 and j % 2 == 0 else 1 if i % 2 == 1 and j % 2 == 1 else 2 for j in range(4)] for i in range(4)])


def ue_len(v):
    """2 floor(log2(v + 1)) + 1 for integers v >= 0."""
    t = np.asarray(v, dtype=np.int64) + 1
    n = np.zeros_like(t)
    for s in range(1, 40):
        n += (t >> s) > 0
    return 2 * n + 1


def se_len(v):
    v = np.asarray(v, dtype=np.int64)
    return ue_len(np.where(v > 0, 2 * v - 1, -2 * v))


def _blocks(plane):
    """[H,W] -> [H/4, W/4, 4, 4]."""
    h, w = plane.shape
    return plane.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3)


def _unblocks(b):
    bh, bw = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(bh * 4, bw * 4)


def forward(x):
    """[...,4,4] residuals -> W = CF X CF^T."""
    return CF @ x @ CF.T


def quantise(w, qp, intra):
    qbits = 15 + qp // 6
    f = (1 << qbits) // (3 if intra else 6)
    z = (np.abs(w) * MF[qp % 6][CLASS] + f) >> qbits
    return np.where(w < 0, -z, z)


def dequantise(z, qp):
    return (z * V[qp % 6][CLASS]) << (qp // 6)


def _butterfly(w, axis):
    w0, w1, w2, w3 = (np.take(w, i, axis) for i in range(4))
    e0, e1, e2, e3 = w0 + w2, w0 - w2, (w1 >> 1) - w3, w1 + (w3 >> 1)
    return np.stack([e0 + e3, e1 + e2, e1 - e2, e0 - e3], axis)


def inverse(w):
    """[...,4,4] dequantised coefficients -> residuals: each row, then each column, then (t + 32) >> 6."""
    return (_butterfly(_butterfly(w, -1), -2) + 32) >> 6


def block_bits(z):
    """[...,4,4] levels -> bits of each block."""
    zz = z.reshape(z.shape[:-2] + (16,))[..., ZIGZAG]
    nz = zz != 0
    nnz = nz.sum(-1)
    pos = np.arange(16)
    last = np.maximum.accumulate(np.where(nz, pos, -1), axis=-1)            # index of the latest non-zero at or before k
    prev = np.concatenate([np.full(last.shape[:-1] + (1,), -1), last[..., :-1]], -1)
    run = pos - prev - 1
    per = np.where(nz, ue_len(run) + se_len(zz), 0).sum(-1)
    return np.where(nnz == 0, 1, 1 + ue_len(np.maximum(nnz - 1, 0)) + per)


def code_plane(cur, pred, qp, intra):
    """One plane (multiples of 4): (reconstruction, bits, levels [H/4,W/4,4,4])."""
    z = quantise(forward(_blocks(cur.astype(np.int64) - pred)), qp, intra)
    rec = np.clip(pred + _unblocks(inverse(dequantise(z, qp))), 0, 255)
    return rec, int(block_bits(z).sum()), z


def motion_search(cur, ref, search=SEARCH, lam=LAMBDA):
    """cur, ref: [H,W] planes of any size (cur is edge-replicated to whole macroblocks, ref to wherever a vector points).
    -> (mv int64 [H/16 up, W/16 up, 2] as (dy, dx), sad int64 [.., ..]) of the winners."""
    cur, ref = np.asarray(cur, dtype=np.int64), np.asarray(ref, dtype=np.int64)
    h, w = cur.shape
    ph, pw = -(-h // MB) * MB, -(-w // MB) * MB
    cur = np.pad(cur, ((0, ph - h), (0, pw - w)), mode="edge")
    rp = np.pad(ref, ((search, ph - ref.shape[0] + search), (search, pw - ref.shape[1] + search)), mode="edge")     # clamped coordinates
    best = None
    for dy in range(-search, search + 1):
        for dx in range(-search, search + 1):
            shifted = rp[search + dy:search + dy + ph, search + dx:search + dx + pw]                  # ref[y + dy, x + dx]
            sad = np.abs(cur - shifted).reshape(ph // MB, MB, pw // MB, MB).sum((1, 3))
            cost = sad + lam * int(se_len(dx) + se_len(dy))
            key = ((cost * 64 + abs(dy) + abs(dx)) * 64 + dy + 32) * 64 + dx + 32     # lexicographic (cost, |dy|+|dx|, dy, dx)
            if best is None:
                best = (key, np.full(sad.shape, dy), np.full(sad.shape, dx), sad)
            else:
                better = key < best[0]
                best = tuple(np.where(better, n, o) for n, o in zip((key, dy, dx, sad), best))
    return np.stack([best[1], best[2]], -1), best[3]


def predict(ref_planes, mv):
    """Motion-compensated prediction of the three planes from the reconstructed (Y, Cb, Cr) and the macroblock vectors."""
    Y, Cb, Cr = ref_planes
    ph, pw = Y.shape
    my, mx = mv.shape[:2]
    dyl, dxl = np.repeat(mv[..., 0], MB, 0).repeat(MB, 1), np.repeat(mv[..., 1], MB, 0).repeat(MB, 1)
    yy, xx = np.mgrid[0:ph, 0:pw]
    py = Y[np.clip(yy + dyl, 0, ph - 1), np.clip(xx + dxl, 0, pw - 1)]
    ch, cw = ph // 2, pw // 2
    dyc, dxc = np.repeat(mv[..., 0], 8, 0).repeat(8, 1), np.repeat(mv[..., 1], 8, 0).repeat(8, 1)
    yy, xx = np.mgrid[0:ch, 0:cw]
    y0, y1 = np.clip(yy + (dyc >> 1), 0, ch - 1), np.clip(yy + (dyc >> 1) + (dyc & 1), 0, ch - 1)
    x0, x1 = np.clip(xx + (dxc >> 1), 0, cw - 1), np.clip(xx + (dxc >> 1) + (dxc & 1), 0, cw - 1)
    pc = [(C[y0, x0] + C[y0, x1] + C[y1, x0] + C[y1, x1] + 2) >> 2 for C in (Cb, Cr)]
    return py, pc[0], pc[1]


def code_frame(cur_planes, ref_planes, qp):
    """One frame at ``qp``: ref_planes None = I frame.  -> (reconstructed planes, bits, mv or None)."""
    intra = ref_planes is None
    bits, mv = 0, None
    if intra:
        pred = [np.full(p.shape, PRED_I, dtype=np.int64) for p in cur_planes]
    else:
        mv, _ = motion_search(cur_planes[0], ref_planes[0])
        pred = predict(ref_planes, mv)
        bits += int((se_len(mv[..., 0]) + se_len(mv[..., 1])).sum())
    rec = []
    for c, p in zip(cur_planes, pred):
        r, b, _ = code_plane(c, p, qp, intra)
        rec.append(r)
        bits += b
    return rec, bits, mv


def code_group(frames, qp):
    """frames: a list of (Y, Cb, Cr) int64 planes -> (list of reconstructed planes, bits of the group, list of mv)."""
    out, mvs, bits, ref = [], [], 0, None
    for f in frames:
        ref, b, mv = code_frame(f, ref, qp)
        out.append(ref)
        mvs.append(mv)
        bits += b
    return out, bits, mvs


def rate_control(frames, bitrate):
    """The QP search of one group -> (qp, reconstructed planes, bits at qp)."""
    budget = int(bitrate) * len(frames)
    lo, hi = QP_MIN, QP_MAX
    while lo < hi:
        mid = (lo + hi) // 2
        if code_group(frames, mid)[1] <= budget:
            hi = mid
        else:
            lo = mid + 1
    rec, bits, _ = code_group(frames, lo)
    return lo, rec, bits


def to_planes(x):
    """float [N,H,W,3] -> (list of (Y, Cb, Cr) int64 planes of the padded frames, padded height, padded width)."""
    x = np.asarray(x)
    u = np.clip(np.where(np.isnan(x), 0, x), 0, 255).astype(np.uint8)
    n, h, w, _ = u.shape
    ph, pw = -(-h // MB) * MB, -(-w // MB) * MB
    u = np.pad(u, ((0, 0), (0, ph - h), (0, pw - w), (0, 0)), mode="edge")
    pay = yuv_ref.rgb_to_yuv(u, MATRIX, RANGE, "420").astype(np.int64)
    L, Cn = ph * pw, ph * pw // 4
    return [(p[:L].reshape(ph, pw), p[L:L + Cn].reshape(ph // 2, pw // 2), p[L + Cn:].reshape(ph // 2, pw // 2)) for p in pay], ph, pw


def from_planes(planes, h, w):
    ph, pw = planes[0][0].shape
    pay = np.stack([np.concatenate([p.reshape(-1) for p in f]) for f in planes]).astype(np.uint8)
    return yuv_ref.yuv_to_rgb(pay, ph, pw, MATRIX, RANGE, "420", SITING)[:, :h, :w]


def vcodec_roundtrip(x, bitrate, gop=8, want_stats=False):
    """float32 [N,H,W,3] -> uint8 [N,H,W,3]; with want_stats also (QP of each group, bits of each group) as int64 arrays."""
    n, h, w, _ = np.asarray(x).shape
    planes, _, _ = to_planes(x)
    out, qps, bits = [], [], []
    for g0 in range(0, n, gop):
        qp, rec, b = rate_control(planes[g0:g0 + gop], bitrate)
        out += rec
        qps.append(qp)
        bits.append(b)
    y = from_planes(out, h, w)
    return (y, np.array(qps, dtype=np.int64), np.array(bits, dtype=np.int64)) if want_stats else y
