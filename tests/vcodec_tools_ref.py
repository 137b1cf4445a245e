"""numpy int64 definition of the codec round trip's H.264 tool set (csrc/vcodec_tools.hip): the GPU reproduces every
byte, every chosen QP and every bit count of this file.  ``tools`` is a bit mask; 0 is vcodec_ref.vcodec_roundtrip to the byte.

Frame t of a group at QP q:
  INTRA16  an I frame is predicted per 16 x 16 macroblock, in raster order, from the row above and the column to the left of the
           *unfiltered* reconstruction of the same frame.  Luma: V = 0, H = 1, DC = 2; chroma (Cb and Cr share the mode, 8 x 8 blocks):
           DC = 0, H = 1, V = 2.  DC is the rounded mean of the neighbours that exist, 128 with none.  The winner is the lexicographic
           minimum of (SAD + LAMBDA ue_len(index), index) over the available candidates; the macroblock pays ue_len of both indices.
           Without the bit the prediction is 128 everywhere, as in vcodec_ref.
  QPEL     a P macroblock's integer winner (vcodec_ref.motion_search) is refined in quarter luma samples: from (4 dy, 4 dx) the centre
           and its 8 neighbours at +-2, then the centre and its 8 neighbours at +-1, each step's winner the lexicographic minimum of
           (SAD + LAMBDA (se_len(mx) + se_len(my)), |my| + |mx|, my, mx).  Luma samples are the H.264 6-tap (1, -5, 20, 20, -5, 1) half
           samples and their averages (``luma_phases``); chroma reads the vector as eighths of a chroma sample, bilinear.  The vector
           costs se_len(mx) + se_len(my) in quarter units.  Without the bit prediction and bits are vcodec_ref's.
  residual exactly vcodec_ref's (code_plane), f = 2^qbits // 3 on I frames and // 6 on P frames.
  DEBLOCK  the H.264 edge filter with indexA = indexB = QP on the reconstructed frame: every vertical edge of a plane, each sample row
           left to right, then every horizontal edge on that result, each column top to bottom - frame-wide, not the standard's
           macroblock interleave.  The filtered frame is the output and the next frame's reference.

ALPHA, BETA and TC0 were typed from memory of H.264 Tables 8-16 and 8-17 and are unchecked against the standard: this file is the
definition.  Not modelled: B frames, intra macroblocks in P frames, Intra 4x4 and the plane mode, the Intra16x16 DC Hadamard,
per-macroblock QP, entropy coding."""
import numpy as np

import vcodec_ref as R

INTRA16, QPEL, DEBLOCK = 1, 2, 4
ALL_TOOLS = INTRA16 | QPEL | DEBLOCK
TOOL_NAMES = {"intra16": INTRA16, "qpel": QPEL, "deblock": DEBLOCK}
MB, LAMBDA = R.MB, R.LAMBDA
TAPS = (1, -5, 20, 20, -5, 1)
PADQ = R.SEARCH + 1                                   # how far a refined vector's base sample can lie from its own

ALPHA = np.array([0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127,
                             144, 162, 182, 203, 226, 255, 255], dtype=np.int64)
BETA = np.array([0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17,
                            18, 18], dtype=np.int64)
TC0 = np.array([(0, 0, 0)] * 17 + [(0, 0, 1), (0, 0, 1), (0, 0, 1), (0, 0, 1), (0, 1, 1), (0, 1, 1), (1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 1, 1),
                                   (1, 1, 2), (1, 1, 2), (1, 1, 2), (1, 1, 2), (1, 2, 3), (1, 2, 3), (2, 2, 3), (2, 2, 4), (2, 3, 4), (2, 3, 4),
                                   (3, 3, 5), (3, 4, 6), (3, 4, 6), (4, 5, 7), (4, 5, 8), (4, 6, 9), (5, 7, 10), (6, 8, 11), (6, 8, 13),
                                   (7, 10, 14), (8, 11, 16), (9, 12, 18), (10, 13, 20), (11, 15, 23), (13, 17, 25)], dtype=np.int64)


def new_stats():
    """Branch counters of the final coding of every group."""
    return {"luma_mode": [0, 0, 0], "chroma_mode": [0, 0, 0], "dc_case": {"both": 0, "one": 0, "none": 0},
            "phase": np.zeros((4, 4), dtype=np.int64), "bs": [0] * 5, "bs4_strong": 0, "bs4_weak": 0, "ap": [0, 0], "aq": [0, 0],
            "p1_update": 0}


def tools_mask(tools):
    """An int mask, or an iterable of names from TOOL_NAMES -> the mask."""
    if isinstance(tools, (int, np.integer)) and not isinstance(tools, bool):
        if tools < 0 or tools & ~ALL_TOOLS:
            raise ValueError(f"vcodec tools {tools!r}: unknown bits (known: {ALL_TOOLS})")
        return int(tools)
    mask = 0
    for name in tools:
        if name not in TOOL_NAMES:
            raise ValueError(f"vcodec tool {name!r}: one of {sorted(TOOL_NAMES)}")
        mask |= TOOL_NAMES[name]
    return mask


# ---- INTRA16 ----------------------------------------------------------------------------------------------------------------------
def _dc(top, left, shift):
    """Rounded mean of the neighbours that exist (each of 2^shift samples) -> (value, case)."""
    if top is not None and left is not None:
        return (int(top.sum() + left.sum()) + (1 << shift)) >> (shift + 1), "both"
    if top is not None or left is not None:
        return (int((top if top is not None else left).sum()) + (1 << (shift - 1))) >> shift, "one"
    return 128, "none"


def _candidates(rec, r, c, size, order):
    """Predictions of the size x size block (r, c) from the reconstructed plane: {index: (pred, DC case or None)}; order = (V, H, DC) indices."""
    y0, x0 = r * size, c * size
    top = rec[y0 - 1, x0:x0 + size] if r > 0 else None
    left = rec[y0:y0 + size, x0 - 1] if c > 0 else None
    out = {}
    if top is not None:
        out[order[0]] = (np.tile(top, (size, 1)), None)
    if left is not None:
        out[order[1]] = (np.repeat(left[:, None], size, 1), None)
    dc, case = _dc(top, left, 4 if size == 16 else 3)
    out[order[2]] = (np.full((size, size), dc, dtype=np.int64), case)
    return out


def intra_frame(cur, qp, stats=None):
    """An I frame with INTRA16 -> (unfiltered reconstructed planes, bits, luma modes [mby, mbx], chroma modes, non-zero levels per macroblock)."""
    ph, pw = cur[0].shape
    rec = [np.zeros(p.shape, dtype=np.int64) for p in cur]
    bits = 0
    lm, cm, nzl = (np.zeros((ph // MB, pw // MB), dtype=np.int64) for _ in range(3))
    for r in range(ph // MB):
        for c in range(pw // MB):
            blk = cur[0][r * 16:r * 16 + 16, c * 16:c * 16 + 16]
            cands = _candidates(rec[0], r, c, 16, (0, 1, 2))
            _, mode = min((int(np.abs(blk - p).sum()) + LAMBDA * int(R.ue_len(i)), i) for i, (p, _) in cands.items())
            rec[0][r * 16:r * 16 + 16, c * 16:c * 16 + 16], b, z = R.code_plane(blk, cands[mode][0], qp, True)
            bits += b + int(R.ue_len(mode))
            nzl[r, c] += int((z != 0).sum())
            lm[r, c] = mode
            cb, cr = (cur[k][r * 8:r * 8 + 8, c * 8:c * 8 + 8] for k in (1, 2))
            ca, cc = _candidates(rec[1], r, c, 8, (2, 1, 0)), _candidates(rec[2], r, c, 8, (2, 1, 0))
            _, cmode = min((int(np.abs(cb - ca[i][0]).sum() + np.abs(cr - cc[i][0]).sum()) + LAMBDA * int(R.ue_len(i)), i) for i in ca)
            for k, blkc, cd in ((1, cb, ca), (2, cr, cc)):
                rec[k][r * 8:r * 8 + 8, c * 8:c * 8 + 8], b, z = R.code_plane(blkc, cd[cmode][0], qp, True)
                bits += b
                nzl[r, c] += int((z != 0).sum())
            bits += int(R.ue_len(cmode))
            cm[r, c] = cmode
            if stats is not None:
                stats["luma_mode"][mode] += 1
                stats["chroma_mode"][cmode] += 1
                if mode == 2:
                    stats["dc_case"][cands[2][1]] += 1
    return rec, bits, lm, cm, nzl


# ---- QPEL -------------------------------------------------------------------------------------------------------------------------
def _tap6(a, axis):
    """The 6-tap over positions -2..+3 along ``axis``: the result is 5 shorter, its index 0 sits at input index 2."""
    n = a.shape[axis] - 5
    return sum(t * np.take(a, np.arange(k, k + n), axis) for k, t in enumerate(TAPS))


def luma_phases(ref, pad=0):
    """[4, 4, H + 2 pad, W + 2 pad]: the sample of phase (fy, fx) at every integer position -pad .. H + pad - 1 of the plane, every
    coordinate clamped to it."""
    ref = np.asarray(ref, dtype=np.int64)
    ny, nx = ref.shape[0] + 2 * pad, ref.shape[1] + 2 * pad
    A = np.pad(ref, (pad + 3, pad + 4), mode="edge")
    c = lambda v: np.clip(v, 0, 255)
    b1 = _tap6(A, 1)                                            # rows of A, columns 2 .. -4
    h1 = _tap6(A, 0)
    j1 = _tap6(b1, 0)
    core = lambda v, dy=0, dx=0: v[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]       # index 1 of these arrays is position -pad
    G, Gx, Gy = core(A[2:-3, 2:-3]), core(A[2:-3, 2:-3], 0, 1), core(A[2:-3, 2:-3], 1, 0)
    bf, hf = c((b1[2:-3] + 16) >> 5), c((h1[:, 2:-3] + 16) >> 5)
    b, s, h, m, j = core(bf), core(bf, 1, 0), core(hf), core(hf, 0, 1), core(c((j1 + 512) >> 10))
    avg = lambda u, v: (u + v + 1) >> 1
    return np.array([[G, avg(G, b), b, avg(b, Gx)],
                     [avg(G, h), avg(b, h), avg(b, j), avg(b, m)],
                     [h, avg(h, j), j, avg(j, m)],
                     [avg(h, Gy), avg(h, s), avg(j, s), avg(m, s)]])


def _gather_luma(PP, my, mx, ph, pw):
    """The prediction of every luma sample at per-sample quarter vectors (my, mx) from PP = luma_phases(ref, PADQ)."""
    yy, xx = np.mgrid[0:ph, 0:pw]
    return PP[my & 3, mx & 3, PADQ + yy + (my >> 2), PADQ + xx + (mx >> 2)]


def qpel_refine(cur, ref, mv):
    """Integer winners mv [mby, mbx, 2] -> (quarter vectors [mby, mbx, 2] as (my, mx), their SADs)."""
    cur = np.asarray(cur, dtype=np.int64)
    ph, pw = cur.shape
    PP = luma_phases(ref, PADQ)
    up = lambda v: np.repeat(np.repeat(v, MB, 0), MB, 1)
    cy, cx = 4 * mv[..., 0], 4 * mv[..., 1]
    sad = None
    for step in (2, 1):
        best = None
        for oy in (-step, 0, step):
            for ox in (-step, 0, step):
                my, mx = cy + oy, cx + ox
                s = np.abs(cur - _gather_luma(PP, up(my), up(mx), ph, pw)).reshape(ph // MB, MB, pw // MB, MB).sum((1, 3))
                cost = s + LAMBDA * (R.se_len(mx) + R.se_len(my))
                key = ((cost * 128 + np.abs(my) + np.abs(mx)) * 128 + my + 64) * 128 + mx + 64
                if best is None:
                    best = (key, my, mx, s)
                else:
                    better = key < best[0]
                    best = tuple(np.where(better, n, o) for n, o in zip((key, my, mx, s), best))
        _, cy, cx, sad = best
    return np.stack([cy, cx], -1), sad


def predict_qpel(ref_planes, mvq):
    """Prediction of the three planes at quarter vectors mvq [mby, mbx, 2]."""
    Y, Cb, Cr = ref_planes
    ph, pw = Y.shape
    up = lambda v, k: np.repeat(np.repeat(v, k, 0), k, 1)
    py = _gather_luma(luma_phases(Y, PADQ), up(mvq[..., 0], MB), up(mvq[..., 1], MB), ph, pw)
    ch, cw = ph // 2, pw // 2
    my, mx = up(mvq[..., 0], 8), up(mvq[..., 1], 8)
    yy, xx = np.mgrid[0:ch, 0:cw]
    y0, y1 = np.clip(yy + (my >> 3), 0, ch - 1), np.clip(yy + (my >> 3) + 1, 0, ch - 1)
    x0, x1 = np.clip(xx + (mx >> 3), 0, cw - 1), np.clip(xx + (mx >> 3) + 1, 0, cw - 1)
    xf, yf = mx & 7, my & 7
    pc = [((8 - xf) * (8 - yf) * C[y0, x0] + xf * (8 - yf) * C[y0, x1] + (8 - xf) * yf * C[y1, x0] + xf * yf * C[y1, x1] + 32) >> 6
          for C in (Cb, Cr)]
    return py, pc[0], pc[1]


# ---- DEBLOCK ----------------------------------------------------------------------------------------------------------------------
def boundary_strengths(intra, nz, mvq):
    """bS of every 4-sample luma edge segment: (vertical [bh, bw], horizontal [bh, bw]); entry (by, bx) is the edge between 4x4 block
    (by, bx) and the one to its left / above.  Column 0 / row 0 (picture borders) are 0: not filtered.  nz: [bh, bw] bool, a non-zero luma
    level in the block; mvq: [bh / 4, bw / 4, 2] quarter vectors (both unused on I frames)."""
    bh, bw = nz.shape
    out = []
    for axis in (1, 0):
        idx = np.arange(nz.shape[axis])
        mbedge = (idx % 4 == 0)
        mbedge = mbedge[None, :] if axis == 1 else mbedge[:, None]
        if intra:
            bs = np.where(mbedge, 4, 3) * np.ones((bh, bw), dtype=np.int64)
        else:
            v = np.repeat(np.repeat(mvq, 4, 0), 4, 1)
            far = (np.abs(v - np.roll(v, 1, axis)) >= 4).any(-1)
            bs = np.where(nz | np.roll(nz, 1, axis), 2, np.where(mbedge & far, 1, 0))
        bs = bs.copy()
        if axis == 1:
            bs[:, 0] = 0
        else:
            bs[0, :] = 0
        out.append(bs)
    return out[0], out[1]


def filter_edge(p, q, bs, qp, chroma, stats=None):
    """One edge of many lines at once: p, q [lines, 4] (p[:, 0] = p0 next to the edge ... p3; chroma uses p0, p1 only), bs [lines].
    -> new (p, q)."""
    alpha, beta = int(ALPHA[qp]), int(BETA[qp])
    p0, p1, p2, p3 = (p[:, i] for i in range(4))
    q0, q1, q2, q3 = (q[:, i] for i in range(4))
    on = (bs > 0) & (np.abs(p0 - q0) < alpha) & (np.abs(p1 - p0) < beta) & (np.abs(q1 - q0) < beta)
    ap, aq = np.abs(p2 - p0) < beta, np.abs(q2 - q0) < beta
    tc0 = TC0[qp][np.clip(bs, 1, 3) - 1]
    tc = tc0 + 1 if chroma else tc0 + ap + aq
    delta = np.clip((4 * (q0 - p0) + (p1 - q1) + 4) >> 3, -tc, tc)
    weak, strong = on & (bs < 4), on & (bs == 4)
    np_, nq = p.copy(), q.copy()
    np_[:, 0] = np.where(weak, np.clip(p0 + delta, 0, 255), p0)
    nq[:, 0] = np.where(weak, np.clip(q0 - delta, 0, 255), q0)
    small = np.abs(p0 - q0) < (alpha >> 2) + 2
    if chroma:
        np_[:, 0] = np.where(strong, (2 * p1 + p0 + q1 + 2) >> 2, np_[:, 0])
        nq[:, 0] = np.where(strong, (2 * q1 + q0 + p1 + 2) >> 2, nq[:, 0])
        return np_, nq
    mid = (p0 + q0 + 1) >> 1
    np_[:, 1] = np.where(weak & ap, p1 + np.clip((p2 + mid - 2 * p1) >> 1, -tc0, tc0), p1)
    nq[:, 1] = np.where(weak & aq, q1 + np.clip((q2 + mid - 2 * q1) >> 1, -tc0, tc0), q1)
    sp, sq = strong & ap & small, strong & aq & small
    np_[:, 0] = np.where(sp, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, np.where(strong, (2 * p1 + p0 + q1 + 2) >> 2, np_[:, 0]))
    np_[:, 1] = np.where(sp, (p2 + p1 + p0 + q0 + 2) >> 2, np_[:, 1])
    np_[:, 2] = np.where(sp, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, p2)
    nq[:, 0] = np.where(sq, (q2 + 2 * q1 + 2 * q0 + 2 * p0 + p1 + 4) >> 3, np.where(strong, (2 * q1 + q0 + p1 + 2) >> 2, nq[:, 0]))
    nq[:, 1] = np.where(sq, (q2 + q1 + q0 + p0 + 2) >> 2, nq[:, 1])
    nq[:, 2] = np.where(sq, (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3, q2)
    if stats is not None:
        stats["ap"][0] += int((on & ~ap).sum())
        stats["ap"][1] += int((on & ap).sum())
        stats["aq"][0] += int((on & ~aq).sum())
        stats["aq"][1] += int((on & aq).sum())
        stats["p1_update"] += int((weak & ap).sum())
        stats["bs4_strong"] += int(sp.sum() + sq.sum())
        stats["bs4_weak"] += int((strong & ~sp).sum() + (strong & ~sq).sum())
    return np_, nq


def _edge_pass(plane, bs, qp, chroma, stats):
    """Every vertical edge of ``plane``, left to right, rows independent.  bs: [rows, edges] the bS of the edge at 4 (k + 1) on each row."""
    out = plane.copy()
    for k in range(bs.shape[1]):
        x = 4 * (k + 1)
        p, q = filter_edge(out[:, x - 4:x][:, ::-1], out[:, x:x + 4], bs[:, k], qp, chroma, stats)
        out[:, x - 4:x], out[:, x:x + 4] = p[:, ::-1], q
    return out


def deblock_frame(planes, qp, intra, nz=None, mvq=None, stats=None):
    """The filtered (Y, Cb, Cr) of a reconstructed frame."""
    ph, pw = planes[0].shape
    if nz is None:
        nz = np.zeros((ph // 4, pw // 4), dtype=bool)
    bsv, bsh = boundary_strengths(intra, nz, mvq)
    if stats is not None:
        for bs in (bsv[:, 1:], bsh[1:, :]):
            for v in range(5):
                stats["bs"][v] += int((bs == v).sum())
    out = []
    for i, plane in enumerate(planes):
        if i == 0:
            v, h = np.repeat(bsv[:, 1:], 4, 0), np.repeat(bsh[1:, :], 4, 1).T
        else:                                                  # chroma edge 4k on row yc: the luma edge 8k on luma row 2 yc
            v, h = np.repeat(bsv[:, 2::2], 2, 0), np.repeat(bsh[2::2, :], 2, 1).T
        plane = _edge_pass(plane, v, qp, i > 0, stats if i == 0 else None)
        out.append(_edge_pass(plane.T, h, qp, i > 0, stats if i == 0 else None).T.copy())
    return out


# ---- frames, groups, rate ---------------------------------------------------------------------------------------------------------
def code_frame(cur, ref, qp, tools, stats=None):
    """One frame at ``qp``; ref None = I frame, else the previous output frame.  -> (output planes, bits, quarter vectors or None)."""
    intra = ref is None
    nz = mvq = None
    if intra and tools & INTRA16:
        rec, bits = intra_frame(cur, qp, stats)[:2]
    else:
        bits = 0
        if intra:
            pred = [np.full(p.shape, R.PRED_I, dtype=np.int64) for p in cur]
        else:
            mv, _ = R.motion_search(cur[0], ref[0])
            if tools & QPEL:
                mvq, _ = qpel_refine(cur[0], ref[0], mv)
                pred = predict_qpel(ref, mvq)
                bits += int((R.se_len(mvq[..., 0]) + R.se_len(mvq[..., 1])).sum())
                if stats is not None:
                    np.add.at(stats["phase"], (mvq[..., 0] & 3, mvq[..., 1] & 3), 1)
            else:
                mvq = 4 * mv
                pred = R.predict(ref, mv)
                bits += int((R.se_len(mv[..., 0]) + R.se_len(mv[..., 1])).sum())
        rec = []
        for i, (c, p) in enumerate(zip(cur, pred)):
            r, b, z = R.code_plane(c, p, qp, intra)
            rec.append(r)
            bits += b
            if i == 0:
                nz = (z != 0).any((-1, -2))
    if tools & DEBLOCK:
        rec = deblock_frame(rec, qp, intra, nz, mvq, stats)
    return rec, bits, mvq


def code_group(frames, qp, tools, stats=None):
    out, bits, ref = [], 0, None
    for f in frames:
        ref, b, _ = code_frame(f, ref, qp, tools, stats)
        out.append(ref)
        bits += b
    return out, bits


def rate_control(frames, bitrate, tools, stats=None):
    """vcodec_ref.rate_control's procedure with this file's frame coder -> (qp, output planes, bits at qp)."""
    budget = int(bitrate) * len(frames)
    lo, hi = R.QP_MIN, R.QP_MAX
    while lo < hi:
        mid = (lo + hi) // 2
        if code_group(frames, mid, tools)[1] <= budget:
            hi = mid
        else:
            lo = mid + 1
    rec, bits = code_group(frames, lo, tools, stats)
    return lo, rec, bits


def vcodec_roundtrip(x, bitrate, gop=8, tools=0, want_stats=False):
    """float32 [N,H,W,3] -> uint8 [N,H,W,3]; with want_stats also (QP of each group, bits of each group, branch counters)."""
    tools = tools_mask(tools)
    n, h, w, _ = np.asarray(x).shape
    planes, _, _ = R.to_planes(x)
    stats = new_stats()
    out, qps, bits = [], [], []
    for g0 in range(0, n, gop):
        qp, rec, b = rate_control(planes[g0:g0 + gop], bitrate, tools, stats)
        out += rec
        qps.append(qp)
        bits.append(b)
    y = R.from_planes(out, h, w)
    return (y, np.array(qps, dtype=np.int64), np.array(bits, dtype=np.int64), stats) if want_stats else y
