"""-m gpu: the T5 operators of csrc/t5.hip (rmsnorm, gated_gelu, attention_bias) and the token and tile glue kernels of csrc/elementwise.hip
that the norm / layout net did not reach (gemv, patchify / unpatchify, blend_edge, conv_out_gather[_cl], tile_gather) against the float64
definitions of tests/glue_ref.py, over the case table of tests/glue_cases.py.  Where the arithmetic is a copy or exact (patchify, tile_gather,
the `selection` family of the attention, the grid family of conv_out_gather, b outside the blended strip) the assertion is equality of bits.
Elsewhere, for EVERY output element,

    |got - ref64| <= 0.5 ulp_out(ref64) + k 2^-24 mag     (+ the half ulp of an inner bf16 rounding the kernel documents, see glue_ref.py)

k is not chosen here.  tests/test_glue_ref_cpu.py measures what the fp32 restatements of tests/emu_ops.py need on these same inputs; a kernel
is allowed max(4, 8 k_emu).  gated_gelu's `main` family is held to bits: outside a band of k 2^-24 |a| around a bf16 rounding boundary of
gelu64(a) the output is rne(rne(gelu64(a)) b), inside it either neighbour's product; k is the band a kernel needs.

    operator            k_emu   allowed   smallest k at which the kernel passed (MI355X)
    rmsnorm             2.94    23.52     2.653
    gated_gelu (band)   0.06    4.0       0.000   (no output of 2.6 million is the other neighbour's product)
    gated_gelu_tail     0.5     4.0       0.000
    attention_uniform   0.0     4.0       0.000
    attention_exact     1.67    13.36     2.570
    gemv                1.66    13.28     1.583
    gemv_silu           1.89    15.12     2.789
    blend_edge          0.01    4.0       1.121
    conv_out_gather     0.96    7.68      0.957
    ncthw_from_cl       0.72    5.76      0.000   (conv_out_gather's range map: norm_cases' constant)

Every test prints the k it needed (pytest -s).  Also here: the refusals."""
import pytest
import torch

import emu_ops as E
import glue_cases as GC
import glue_ref as G
import norm_cases as NC
import norm_ref as R
from dove_amd import lib as L
from dove_amd import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64


def _budget(op, got, ref, mag, what, dtype=None, slack=None, allowed=None):
    k = G.need_k(got, ref, mag, dtype, slack)
    allowed = GC.allowed_k(op) if allowed is None else allowed
    print(f"  {op} {what}: needs {k:.3f} (allowed {allowed:.2f})")
    assert k <= allowed, f"{op} {what}: the smallest passing k is {k:.3f}, allowed {allowed:.2f}"


def _bits(t):
    t = t.contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _refused(match, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=match):
        fn(*args, **kw)


# ---- rmsnorm -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", GC.RMS_D)
def test_rmsnorm(D):
    w = GC.rms_weight(D)
    wd = w.cuda()
    worst = 0.0
    for rows in GC.RMS_ROWS:
        for family in GC.RMS_FAMILIES:
            x = GC.rms_input(family, rows, D)
            xd = x.cuda()
            got = ops.rmsnorm(xd, wd, GC.RMS_EPS)
            torch.cuda.synchronize()
            ref, mag = G.rmsnorm(x, w, GC.RMS_EPS)
            k = R.need_k(got, ref, mag)
            worst = max(worst, k)
            assert k <= GC.allowed_k("rmsnorm"), f"rmsnorm {rows}x{D}/{family}: the smallest passing k is {k:.3f}"
            if rows == 226:                                      # a row does not depend on the block or the wave it lands in
                for r in GC.RMS_SINGLE_ROWS:
                    one = ops.rmsnorm(xd[r:r + 1].contiguous(), wd, GC.RMS_EPS)
                    assert _same_bits(one[0], got[r]), f"rmsnorm {D}/{family}: row {r} of 226 differs from its 1-row call"
    print(f"  rmsnorm D {D} (NIT {GC.rms_nit(D)}): needs {worst:.3f} (allowed {GC.allowed_k('rmsnorm'):.2f})")


def test_rmsnorm_refusals():
    w = torch.ones(4104, device="cuda")
    _refused("multiple of 8", ops.rmsnorm, torch.zeros(2, 12, dtype=BF, device="cuda"), w, 1e-6)
    _refused("<= 4096", ops.rmsnorm, torch.zeros(2, 4104, dtype=BF, device="cuda"), w, 1e-6)
    x, y = torch.zeros(1, 8, dtype=BF, device="cuda"), torch.full((1, 8), 7.0, dtype=BF, device="cuda")
    lib = L.load()
    assert lib.dove_rmsnorm_bf16(L.ptr(x), L.ptr(y), 0, 8, 1e-6, L.ptr(w), L.stream_ptr()) != 0 and b"empty" in lib.dove_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ---- gated_gelu ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Fh", GC.GG_F)
@pytest.mark.parametrize("M", GC.GG_M)
def test_gated_gelu(M, Fh):
    x = GC.gg_input("main", M, Fh)
    got = ops.gated_gelu(x.cuda())
    torch.cuda.synchronize()
    gg = G.GatedGelu(x)
    k = gg.need_k(got)
    print(f"  gated_gelu (band) {M}x{Fh}: needs {k:.3f} (allowed {GC.allowed_k('gated_gelu'):.2f}), "
          f"{int((got.double().cpu() != gg.out).sum())} of {got.numel()} outputs are the other neighbour's")
    assert k <= GC.allowed_k("gated_gelu"), f"gated_gelu {M}x{Fh}: an output is no neighbour's product, or needs a band of {k:.3f}"
    x = GC.gg_input("tail", M, Fh)
    got = ops.gated_gelu(x.cuda())
    torch.cuda.synchronize()
    ref, mag, slack = G.GatedGelu(x).tail()
    _budget("gated_gelu_tail", got, ref, mag, f"{M}x{Fh}", slack=slack)


def test_gated_gelu_refusals():
    lib = L.load()
    x, y = torch.zeros(2, 24, dtype=BF, device="cuda"), torch.zeros(2, 12, dtype=BF, device="cuda")
    assert lib.dove_gated_gelu_bf16(L.ptr(x), L.ptr(y), 2, 12, L.stream_ptr()) != 0 and b"multiple of 8" in lib.dove_last_error()
    assert lib.dove_gated_gelu_bf16(L.ptr(x), L.ptr(y), 0, 8, L.stream_ptr()) != 0


# ---- attention_bias ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,heads", GC.ATT_CASES)
def test_attention_bias(N, heads):
    # selection: q = 0 and bias = +40 at key pi_h(i): the row is v[pi_h(i)], bit for bit (key index, lane tails, row max, head strides)
    qkv, bias = GC.att_input("selection", N, heads)
    got = ops.attention_bias(qkv.cuda(), bias.cuda(), heads)
    torch.cuda.synchronize()
    want = G.selected_rows(qkv, GC.att_perm(N, heads))
    bad = (_bits(got) != _bits(want)).nonzero()
    assert bad.numel() == 0, f"attention_bias selection N {N} heads {heads}: {bad.shape[0]} elements differ, the first at (row, column) {bad[0].tolist()}"
    # uniform: q = 0, bias = 0: P = rne(1 / N) for every key
    qkv, bias = GC.att_input("uniform", N, heads)
    got = ops.attention_bias(qkv.cuda(), bias.cuda(), heads)
    torch.cuda.synchronize()
    A = G.AttentionBias(qkv, bias, heads)
    _budget("attention_uniform", got, A.ref, A.mag, f"N {N} heads {heads}")
    # exact scores: the two score roundings are identities, P's rounding is the only inner one
    qkv, bias = GC.att_input("exact", N, heads)
    got = ops.attention_bias(qkv.cuda(), bias.cuda(), heads)
    torch.cuda.synchronize()
    A = G.AttentionBias(qkv, bias, heads)
    assert A.scores_exact
    _budget("attention_exact", got, A.ref, A.mag, f"N {N} heads {heads}", slack=A.slack(GC.allowed_k("attention_exact")))


def test_attention_bias_refusals():
    lib = L.load()
    qkv = torch.zeros(8, 192 + 8, dtype=BF, device="cuda")
    bias = torch.zeros(8 * 8, device="cuda")
    out = torch.full((8, 64), 7.0, dtype=BF, device="cuda")
    base = qkv.data_ptr()

    def call(ld, N, head_dim):
        return lib.dove_attention_bias_bf16(L.ptr(qkv), L.C.c_void_p(base + 128), L.C.c_void_p(base + 256), ld, L.ptr(bias), L.ptr(out), 64, N, 1,
                                            head_dim, L.stream_ptr())
    assert call(192, 8, 128) != 0 and b"head_dim" in lib.dove_last_error()
    assert call(192, 0, 64) != 0 and b"1..1024" in lib.dove_last_error()
    assert call(192, 1025, 64) != 0 and b"1..1024" in lib.dove_last_error()
    assert call(196, 8, 64) != 0 and b"leading dimension" in lib.dove_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    assert call(200, 8, 64) == 0                                   # ld % 8 == 0 is all it takes
    torch.cuda.synchronize()


# ---- gemv ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_f", GC.GEMV_IN)
def test_gemv(in_f):
    worst = {0: 0.0, 1: 0.0}
    for out_f in GC.GEMV_OUT:
        Wm, b, x = GC.gemv_input(in_f, out_f)
        Wd, bd, xd = Wm.cuda(), b.cuda(), x.cuda()
        for act in (0, 1):
            op = "gemv_silu" if act else "gemv"
            for bias, bdev in ((b, bd), (None, None)):
                got = ops.gemv(Wd, bdev, xd, act)
                torch.cuda.synchronize()
                ref, mag = G.gemv(Wm, bias, x, act)
                k = R.need_k(got, ref, mag)
                worst[act] = max(worst[act], k)
                assert k <= GC.allowed_k(op), f"{op} {out_f}x{in_f} bias {bias is not None}: the smallest passing k is {k:.3f}"
    print(f"  gemv in {in_f}: needs {worst[0]:.3f} (allowed {GC.allowed_k('gemv'):.2f})")
    print(f"  gemv_silu in {in_f}: needs {worst[1]:.3f} (allowed {GC.allowed_k('gemv_silu'):.2f})")


def test_gemv_refusals():
    _refused("multiple of 8", ops.gemv, torch.zeros(4, 12, dtype=BF, device="cuda"), None, torch.zeros(12, device="cuda"))


# ---- patchify / unpatchify -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pt,p,Cc,T,H,W,extra", GC.PATCH_CASES)
def test_patchify(pt, p, Cc, T, H, W, extra):
    feat = Cc * pt * p * p
    ld = feat + extra
    x = GC.finite_bf16_patterns(T * Cc * H * W, pt, p, Cc).reshape(T, Cc, H, W)
    idx = G.patch_index(T, Cc, H, W, pt, p)
    want = x.reshape(-1)[idx]
    tok = ops.patchify(x.cuda(), pt, p, ld)
    torch.cuda.synchronize()
    assert tok.shape == (idx.shape[0], ld)
    assert _same_bits(tok[:, :feat], want), "patchify is not the reference permutation"
    assert bool((_bits(tok[:, feat:]) == 0).all()), "pad columns must be exactly +0"
    x32 = GC.widen_with_low_bits(x)                               # fp32 in: the RNE of the input, ties to even, overflow to inf
    tok32 = ops.patchify(x32.cuda(), pt, p, ld)
    torch.cuda.synchronize()
    assert torch.equal(_bits(tok32[:, :feat]), G.rne_bits_bf16(x32).reshape(-1)[idx]), "an fp32 input must be rounded to nearest even"
    tokp = tok.clone()
    tokp[:, feat:] = float("nan")                                 # the pad is never part of the result
    back = ops.unpatchify(tokp, T, Cc, H, W, pt, p, BF)
    back32 = ops.unpatchify(tokp, T, Cc, H, W, pt, p, torch.float32)
    torch.cuda.synchronize()
    assert _same_bits(back, x), "unpatchify(patchify(x)) != x"
    assert _same_bits(back32, x.float()), "the fp32 output must be the exact widening"
    fresh = GC.finite_bf16_patterns(idx.numel(), "tok", pt, p, Cc).reshape(idx.shape)      # unpatchify alone against the permutation
    wantx = torch.empty(T * Cc * H * W, dtype=BF)
    wantx[idx.reshape(-1)] = fresh.reshape(-1)
    assert _same_bits(ops.unpatchify(fresh.cuda(), T, Cc, H, W, pt, p, BF), wantx.reshape(T, Cc, H, W))


def test_patchify_refusals():
    x = torch.zeros(3, 2, 4, 6, dtype=BF, device="cuda")
    _refused("not divisible", ops.patchify, x, 2, 2, 16)                              # T % pt
    _refused("not divisible", ops.patchify, x[:2, :, :3].contiguous(), 2, 2, 16)      # H % p
    _refused("not divisible", ops.patchify, x[:2].contiguous(), 2, 2, 15)             # ld < 2 * 2 * 2 * 2
    tok = torch.zeros(6, 15, dtype=BF, device="cuda")
    _refused("not divisible", ops.unpatchify, tok, 2, 2, 4, 6, 2, 2, BF)
    _refused("not divisible", ops.unpatchify, torch.zeros(6, 16, dtype=BF, device="cuda"), 3, 2, 4, 6, 2, 2, BF)


# ---- blend_edge ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", GC.BLEND_CASES, ids=[f"axis{c[0]}-T{c[1]}-a{c[2][0]}x{c[2][1]}-b{c[3][0]}x{c[3][1]}-ld{c[4]}" for c in GC.BLEND_CASES])
def test_blend_edge(case):
    axis = case[0]
    a, b = GC.blend_input(case)
    for extent in GC.blend_extents(case):
        ad, bd = a.cuda(), b.cuda()
        out = ops.blend_edge(ad, bd, extent, axis)
        torch.cuda.synchronize()
        assert out.data_ptr() == bd.data_ptr()
        ref, mag, strip = G.blend_edge(a, b, extent, axis)
        _budget("blend_edge", bd, ref, mag, f"{case} extent {extent}")
        assert _same_bits(ad, a), "a must be untouched"
        assert torch.equal(_bits(bd)[~strip], _bits(b)[~strip]), "b outside the blended strip must be bit-identical"
        assert _same_bits(bd.narrow(axis + 1, 0, 1), a.narrow(axis + 1, a.shape[axis + 1] - extent, 1)), "e = 0 is a's row / column itself"


def test_blend_edge_refusals():
    a, b = torch.zeros(1, 3, 5, 4, dtype=BF, device="cuda"), torch.full((1, 6, 7, 4), 7.0, dtype=BF, device="cuda")
    _refused("equal widths", ops.blend_edge, a, b, 2, 0)                              # Wa != Wb
    _refused("equal widths", ops.blend_edge, a, b[:, :, :5].contiguous(), 4, 0)       # extent > Ha
    _refused("equal heights", ops.blend_edge, a, b, 2, 1)
    torch.cuda.synchronize()
    assert bool((b == 7.0).all()), "a refused call wrote b"


# ---- conv_out_gather / conv_out_gather_cl ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cc,ldp", GC.COG_CLDP)
def test_conv_out_gather(Cc, ldp):
    worst = {"conv_out_gather": 0.0, "ncthw_from_cl": 0.0}

    def note(op, got, ref, mag, what, dtype=None, allowed=None):
        k = R.need_k(got, ref, mag, dtype)
        worst[op] = max(worst[op], k)
        allowed = GC.allowed_k(op) if allowed is None else allowed
        assert k <= allowed, f"{op} C {Cc} ldp {ldp} {what}: the smallest passing k is {k:.3f}, allowed {allowed:.2f}"

    for H, W in GC.COG_HW:
        for T in GC.COG_T:
            p, bias = GC.cog_input("grid", Cc, ldp, T, H, W)
            pd, biasd = p.cuda(), bias.cuda()
            for bs, bsd in ((bias, biasd), (None, None)):
                what = f"{T}x{H}x{W} bias {bs is not None}"
                s, _ = G.conv_out_gather(p, Cc, bs)
                want = G.rne(s).to(BF)                             # the 9 taps + bias are exact in fp32: the bf16 rounding is determined
                for ldy in (l for l in GC.COG_LDY if l >= Cc):
                    y = ops.conv_out_gather_cl(pd, Cc, bsd, ldy)
                    torch.cuda.synchronize()
                    assert _same_bits(y[..., :Cc], want), f"conv_out_gather_cl {what} ldy {ldy}"
                    assert bool((_bits(y[..., Cc:]) == 0).all()), "pad channels must be exactly +0"
                for dt in (BF, torch.float32):
                    y = ops.conv_out_gather(pd, Cc, bsd, dt)
                    torch.cuda.synchronize()
                    assert _same_bits(y, want.permute(3, 0, 1, 2).to(dt)), f"conv_out_gather {what} {dt}"
                    for (sc, sh), (lo, hi) in ((NC.AFFINE[2], NC.CLAMP), (NC.AFFINE[3], (0.0, 255.0))):
                        ref, mag = R.ncthw_from_cl(want, Cc, sc, sh, lo, hi)
                        y = ops.conv_out_gather(pd, Cc, bsd, dt, sc, sh, lo, hi)
                        torch.cuda.synchronize()
                        note("ncthw_from_cl", y, ref, mag, f"{what} x{sc}+{sh} [{lo},{hi}]", allowed=NC.allowed_k("ncthw_from_cl"))
                        if H * W >= 441:
                            g = y.float().cpu()
                            assert float(g.min()) == R.f32(lo) and float(g.max()) == R.f32(hi), "the clamp must bite on both sides, exactly"
            p, bias = GC.cog_input("gaussian", Cc, ldp, T, H, W)
            pd, biasd = p.cuda(), bias.cuda()
            for bs, bsd in ((bias, biasd), (None, None)):
                what = f"gaussian {T}x{H}x{W} bias {bs is not None}"
                s, mag = G.conv_out_gather(p, Cc, bs)
                y = ops.conv_out_gather_cl(pd, Cc, bsd, 8)
                z = ops.conv_out_gather(pd, Cc, bsd, torch.float32)
                torch.cuda.synchronize()
                note("conv_out_gather", y[..., :Cc], s, mag, what)
                assert _same_bits(z, y[..., :Cc].permute(3, 0, 1, 2).float()), "the two forms round the same sum"
    for op, k in worst.items():
        allowed = NC.allowed_k(op) if op == "ncthw_from_cl" else GC.allowed_k(op)
        print(f"  {op} (conv_out_gather C {Cc} ldp {ldp}): needs {k:.3f} (allowed {allowed:.2f})")


def test_conv_out_gather_refusals():
    bias = torch.zeros(5, device="cuda")
    out = "conv_out_gather"
    _refused(out, ops.conv_out_gather_cl, torch.zeros(1, 2, 2, 48, device="cuda"), 5, bias, 8)        # C = 5
    _refused(out, ops.conv_out_gather_cl, torch.zeros(1, 2, 2, 40, device="cuda"), 3, bias, 8)        # ldp = 40
    _refused(out, ops.conv_out_gather_cl, torch.zeros(1, 2, 2, 30, device="cuda"), 3, bias, 8)        # ldp % 4
    _refused(out, ops.conv_out_gather_cl, torch.zeros(1, 2, 2, 24, device="cuda"), 3, bias, 8)        # ldp < 9 C
    _refused("ldy", ops.conv_out_gather_cl, torch.zeros(1, 2, 2, 36, device="cuda"), 4, bias, 0)      # ldy < C
    _refused("ldy", ops.conv_out_gather_cl, torch.zeros(1, 2, 2, 28, device="cuda"), 3, bias, 2)
    _refused(out, ops.conv_out_gather, torch.zeros(1, 2, 2, 48, device="cuda"), 5, bias, BF)
    _refused(out, ops.conv_out_gather, torch.zeros(1, 2, 2, 40, device="cuda"), 3, bias, BF)


# ---- tile_gather -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin", [0, 3], ids=["plain", "im2col3"])
def test_tile_gather_grid_stride(cin):
    """Just above 256 * 8192 sixteen-byte chunks: the last ~6 % of the output is written by a thread's SECOND trip."""
    c = GC.TG_BIG
    assert GC.tg_chunks(c) > GC.TG_GRID_CAP
    org = GC.tg_origins(c, c["nb"])
    src = GC.tg_source(c, 3)
    x = E.cl_im2col3x3_from_ncthw(src, c["C"]).cuda()             # [T, H, W, 32] bf16: 27 tap channels + 5 zero
    got = ops.tile_gather(x, c["t0"], c["nt"], c["th"], c["tw"], org, im2col_cin=cin)
    torch.cuda.synchronize()
    t0, nt, th, tw = c["t0"], c["nt"], c["th"], c["tw"]
    if cin == 0:
        want = torch.cat([x[t0:t0 + nt, oy:oy + th, ox:ox + tw] for oy, ox in org])
    else:                                                         # the im2col of the CROPPED tile: zero padding at the tile's own border
        want = torch.cat([E.cl_im2col3x3_from_ncthw(src[:, t0:t0 + nt, oy:oy + th, ox:ox + tw], c["C"]) for oy, ox in org]).cuda()
    assert got.shape == want.shape
    assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16))


def test_tile_gather_limits():
    c = GC.TG_SMALL
    src = GC.tg_source(c, 3)
    x = E.cl_im2col3x3_from_ncthw(src, c["C"]).cuda()
    org = GC.tg_origins(c, 65)
    for cin in (0, 3):
        got = ops.tile_gather(x, c["t0"], c["nt"], c["th"], c["tw"], org[:64], im2col_cin=cin)
        torch.cuda.synchronize()
        assert _same_bits(got, E.tile_gather(x.cpu(), c["t0"], c["nt"], c["th"], c["tw"], org[:64], im2col_cin=cin))
    _refused("nb <= 64", ops.tile_gather, x, c["t0"], c["nt"], c["th"], c["tw"], org)
    _refused("leaves", ops.tile_gather, x, c["t0"], c["nt"], c["th"], c["tw"], [(1, 0)])                  # th == H leaves oy = 0 only
    _refused("does not fit", ops.tile_gather, x, c["t0"], c["nt"], c["th"], c["tw"], org[:2], im2col_cin=4)
