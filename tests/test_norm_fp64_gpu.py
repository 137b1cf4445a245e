"""-m gpu: the normalisation family of csrc/norm.hip and the affine layout kernels of csrc/elementwise.hip against the float64 definitions
of tests/norm_ref.py, over the case table of tests/norm_cases.py, at rounding level: for EVERY output element

    |got - ref64| <= 0.5 ulp_out(ref64) + k 2^-24 mag          (statistics: c in place of k, mag = the output's absolute condition)

k and c are not chosen here.  tests/test_norm_ref_cpu.py measures what the fp32 restatements of tests/emu_ops.py (statistics: an fp32
emulation of the kernel's summation order) need on these same inputs; a kernel is allowed max(4, 8 k_emu), respectively 4 c_emu.  The entry
points that start from given fp32 rows or fp64 sums are held to one fp32 ulp (2^-23 relative for the fp64 sums).

    operator            k_emu / c_emu   allowed   smallest k / c at which the kernel passed (MI355X)
    gn_stats (c)        1.52            6.08      1.513
    gn_sums (c)         3.34            13.36     3.337
    gn_apply            1.5             12.0      1.497
    gn_apply_silu       0.95            7.6       0.858
    sn_apply            1.71            13.68     0.836
    sn_apply_silu       0.87            6.96      0.630
    ln_mod              2.02            16.16     1.878
    ln_constant_rows    0.0             4.0       0.000   (rows of equal elements, against B alone)
    cl_from_ncthw       0.96            7.68      0.952
    cl_im2col3x3        0.61            4.88      0.554
    ncthw_from_cl       0.72            5.76      0.573
    avgpool_time        0.0             4.0       0.000
    axpby               0.63            5.04      0.635
    posterior_sample    0.59            4.72      0.948

Every test prints the k it needed (pytest -s).  Also here: the bit-equalities the
kernels promise (nb instances == nb single calls, pieces of a frame-batch == the whole, in place == out of place) and the refusals."""
import pytest
import torch

import norm_cases as NC
import norm_ref as R
from dove_amd import lib as L
from dove_amd import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
EPS = 1e-6


def _budget(op, got, ref, mag, what, stat=False, dtype=None):
    """Assert the budget for every element; `got` must already be synchronised (the .cpu() inside need_k does it again)."""
    k = R.need_k(got, ref, mag, dtype)
    allowed = NC.allowed_c(op) if stat else NC.allowed_k(op)
    print(f"  {op} {what}: needs {k:.3f} (allowed {allowed:.2f})")
    assert k <= allowed, f"{op} {what}: the smallest passing {'c' if stat else 'k'} is {k:.3f}, allowed {allowed:.2f}"


def _bits(t):
    t = t.contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- GroupNorm statistics --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", NC.FAMILIES)
@pytest.mark.parametrize("case", NC.STATS_CASES, ids=[c[0] for c in NC.STATS_CASES])
def test_groupnorm_stats(case, family):
    name, Cc, shape, nb = case
    x = NC.stats_input(case, family)
    xd = x.cuda()
    ref, mag = R.gn_stats(x, EPS, nb)
    st = ops.groupnorm_stats(xd, EPS, nb)
    torch.cuda.synchronize()
    assert st.shape == ((nb, 32, 2) if nb > 1 else (32, 2)) and st.dtype == torch.float32
    _budget("gn_stats", st, ref, mag, f"{name}/{family}", stat=True)
    if nb > 1:                                                  # the batched form: bit-equal to nb single calls (gn_partial_kernel's promise)
        per = shape[0] // nb
        singles = torch.stack([ops.groupnorm_stats(xd[b * per:(b + 1) * per].contiguous(), EPS) for b in range(nb)])
        torch.cuda.synchronize()
        assert _same_bits(st, singles), f"{name}/{family}: nb form differs from {nb} single calls"
        return
    count = float(x.numel() // 32)
    sums = ops.groupnorm_sums(xd)
    torch.cuda.synchronize()
    sref, smag = R.gn_sums(x)
    _budget("gn_sums", sums, sref, smag, f"{name}/{family}", stat=True, dtype=F64)
    # statistics from the sums, with a count and as the 65-double pair message: one fp32 ulp of the float64 finalisation of those sums
    want, _ = R.gn_from_sums(sums.cpu(), count, EPS)
    a = ops.groupnorm_from_sums(sums, count, EPS)
    msg = torch.cat([sums.reshape(-1), torch.tensor([count], dtype=F64, device="cuda")])
    b = ops.groupnorm_from_sums(msg, None, EPS)
    torch.cuda.synchronize()
    assert R.ulps_off(a, want) <= 1.0, R.ulps_off(a, want)
    assert _same_bits(a, b), f"{name}/{family}: the 65-double message finalises differently"
    assert _same_bits(a, st), f"{name}/{family}: sums -> statistics differs from the one-call statistics"
    if x.dim() == 4 and shape[0] >= 2:                          # pieces of the frame-batch against the whole, bit for bit
        cut = shape[0] // 2 + 1 if shape[0] > 2 else 1
        sa, sb = ops.groupnorm_sums(xd[:cut].contiguous()), ops.groupnorm_sums(xd[cut:].contiguous())
        pieces = ops.groupnorm_from_sums(sa + sb, count, EPS)
        torch.cuda.synchronize()
        assert _same_bits(pieces, st), f"{name}/{family}: two pieces finalise differently from the whole batch"


@pytest.mark.parametrize("nb", NC.PARTIAL_NB)
@pytest.mark.parametrize("rows", NC.PARTIAL_ROWS)
def test_groupnorm_finalize_partials(rows, nb):
    """Synthetic fp32 partial rows through the entry points the conv epilogue's statistics use: 1024 / 1025 is the boundary between the
    one-level finalise and gn_reduce_rows_kernel + gn_finalize_kernel<double>."""
    lib = L.load()
    p, count = NC.partial_rows(rows, nb)
    pd = p.cuda()
    ref, _ = R.gn_from_partials(p, nb, count, EPS)
    ws = torch.zeros(nb * 256 * 64, dtype=F64, device="cuda")
    st = torch.full((nb, 32, 2), float("nan"), dtype=torch.float32, device="cuda")
    L.check(lib.dove_groupnorm_finalize_partials_nb(L.ptr(pd), rows, nb, count, EPS, L.ptr(ws), ws.numel() * 8, L.ptr(st), L.stream_ptr()),
            "dove_groupnorm_finalize_partials_nb")
    torch.cuda.synchronize()
    off = R.ulps_off(st.reshape(ref.shape), ref)
    print(f"  finalize_partials_nb rows {rows} nb {nb}: {off:.3f} fp32 ulp")
    assert off <= 1.0, off
    for b in range(nb):                                         # every instance alone, through the single-instance entry points
        one = pd[b * rows:(b + 1) * rows].contiguous()
        s1 = torch.full((32, 2), float("nan"), dtype=torch.float32, device="cuda")
        L.check(lib.dove_groupnorm_finalize_partials(L.ptr(one), rows, count, EPS, L.ptr(ws), L.ptr(s1), L.stream_ptr()),
                "dove_groupnorm_finalize_partials")
        sums = torch.full((32, 2), float("nan"), dtype=F64, device="cuda")
        L.check(lib.dove_groupnorm_sums_from_partials(L.ptr(one), rows, L.ptr(ws), L.ptr(sums), L.stream_ptr()), "dove_groupnorm_sums_from_partials")
        s2 = ops.groupnorm_from_sums(sums, count, EPS)
        torch.cuda.synchronize()
        assert _same_bits(s1, st[b]), f"rows {rows}: instance {b} of {nb} differs from its single call"
        sref, _ = R.sums_from_partials(p[b * rows:(b + 1) * rows])
        rel = float(((sums.cpu() - sref).abs() / sref.abs()).max())
        assert rel <= 2.0 ** -23, rel
        assert R.ulps_off(s2, ref.reshape(nb, 32, 2)[b]) <= 1.0


def test_groupnorm_finalize_partials_refuses_small_scratch():
    lib = L.load()
    nb, rows = 3, 1025
    p, count = NC.partial_rows(rows, nb)
    pd = p.cuda()
    ws = torch.zeros(nb * 256 * 64, dtype=F64, device="cuda")
    st = torch.full((nb, 32, 2), 7.0, dtype=torch.float32, device="cuda")
    rc = lib.dove_groupnorm_finalize_partials_nb(L.ptr(pd), rows, nb, count, EPS, L.ptr(ws), ws.numel() * 8 - 8, L.ptr(st), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"scratch" in lib.dove_last_error()
    assert bool((st == 7.0).all()) and bool((ws == 0).all()), "a refused call launched something"
    # no scratch at all is enough for 1024 rows (no first level)
    assert lib.dove_groupnorm_finalize_partials_nb(L.ptr(pd), 1024, nb, count, EPS, L.ptr(ws), 0, L.ptr(st), L.stream_ptr()) == 0
    torch.cuda.synchronize()


# ---- GroupNorm / SpatialNorm apply ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", NC.FAMILIES)
@pytest.mark.parametrize("case", NC.APPLY_CASES, ids=[c[0] for c in NC.APPLY_CASES])
def test_groupnorm_apply(case, family):
    name, Cc, nb, (T, H, W), ybs, sshift, tmap = case
    x, gamma, beta, yb = NC.apply_input(case, family)
    st = R.gn_stats(x, EPS, nb)[0].float()                       # the kernel's input: fp32 statistics, the same on both sides
    xd, gd, bd, sd = x.cuda(), gamma.cuda(), beta.cuda(), st.cuda()
    ybd = None if yb is None else yb.cuda()
    for with_yb in ((False, True) if ybs else (False,)):
        kw = dict(yb=yb, Tz=ybs[0], sshift=sshift, tmap=tmap) if with_yb else {}
        okw = dict(yb=ybd, sshift=sshift, tmap=tmap) if with_yb else {}
        p, pmag = R.gn_preact(x, st, gamma, beta, nb=nb, **kw)
        for silu in (False, True):
            ref, mag = R.silu_with_mag(p, pmag) if silu else (p, pmag)
            got = ops.groupnorm_apply(xd, sd, gd, bd, silu=silu, nb=nb, **okw)
            torch.cuda.synchronize()
            op = ("sn_apply" if with_yb else "gn_apply") + ("_silu" if silu else "")
            _budget(op, got, ref, mag, f"{name}/{family}")
            if nb > 1:                                          # bit-equal to nb single calls, each with its own statistics and yb block
                per, Tz = x.shape[0] // nb, ybs[0]
                singles = torch.cat([ops.groupnorm_apply(xd[b * per:(b + 1) * per].contiguous(), sd[b].contiguous(), gd, bd, silu=silu,
                                                         **(dict(yb=ybd[b * Tz:(b + 1) * Tz].contiguous(), sshift=sshift, tmap=tmap) if with_yb else {}))
                                     for b in range(nb)])
                torch.cuda.synchronize()
                assert _same_bits(got, singles), f"{name}/{family}: nb form differs from {nb} single calls"
            del ref, mag, got
        del p, pmag


def test_groupnorm_apply_refusals():
    Cc = 32
    gamma, beta = (t.cuda() for t in NC.channel_params(Cc, "refuse"))
    st = torch.zeros(32, 2, device="cuda")
    x33 = torch.zeros(33, 2, 2, Cc, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="T <= 32"):
        ops.groupnorm_apply(x33, st, gamma, beta)
    with pytest.raises(RuntimeError, match="T <= 32"):
        ops.groupnorm_apply(x33, st, gamma, beta, yb=torch.zeros(1, 2, 2, 2 * Cc, dtype=BF, device="cuda"), sshift=0, tmap=[0] * 33)
    x = torch.zeros(2, 5, 9, Cc, dtype=BF, device="cuda")
    out = torch.full_like(x, 7.0)
    for hz, wz in ((2, 5), (3, 4)):                             # (3, 5) << 1 covers 5 x 9; one less in either direction does not
        with pytest.raises(RuntimeError, match="latent grid too small"):
            ops.groupnorm_apply(x, st, gamma, beta, yb=torch.zeros(1, hz, wz, 2 * Cc, dtype=BF, device="cuda"), sshift=1, tmap=[0, 0], out=out)
    ops.groupnorm_apply(x, st, gamma, beta, yb=torch.zeros(1, 3, 5, 2 * Cc, dtype=BF, device="cuda"), sshift=1, tmap=[0, 0])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"


# ---- LayerNorm + modulation ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", NC.LN_FAMILIES)
@pytest.mark.parametrize("N,D", NC.LN_CASES)
def test_layernorm_modulate(N, D, family):
    x, gamma, beta, mod = NC.ln_input(N, D, family)
    xd, gd, bd, md = x.cuda(), gamma.cuda(), beta.cuda(), mod.cuda()
    for eps in NC.LN_EPS:
        for m, mdev in ((None, None), (mod, md)):
            for split in (NC.ln_splits(N) if m is not None else [0]):
                ref, mag = R.ln_mod(x, gamma, beta, eps, m, split)
                got = ops.layernorm_modulate(xd, gd, bd, eps, mdev, split)
                inplace = xd.clone()
                ops.layernorm_modulate(inplace, gd, bd, eps, mdev, split, out=inplace)
                torch.cuda.synchronize()
                _budget("ln_mod", got, ref, mag, f"{N}x{D}/{family} eps {eps} mod {m is not None} split {split}")
                assert _same_bits(got, inplace), f"{N}x{D}/{family}: in place differs from out of place"
                if family == "constant-rows":
                    # var = 0 and x - mean = 0 exactly (an fp32 sum of D <= 4096 equal bf16 values is exact, and so is its quotient by D),
                    # so rstd = eps^-1/2 multiplies a zero and the output is B: nothing but B's own two terms may round.  The general
                    # budget above cannot see an inexact mean here (its mag carries rstd); this one does, for every element.
                    _budget("ln_constant_rows", got, *R.ln_constant_rows(x, gamma, beta, m, split), f"{N}x{D} eps {eps} split {split}")


# ---- layout kernels --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc,cp,thw", NC.CL_CASES)
def test_cl_from_ncthw(Cc, cp, thw, dt):
    x = NC.layout_input((Cc,) + thw, dt, "cl", Cc, cp)
    for sc, sh in NC.AFFINE:
        ref, mag = R.cl_from_ncthw(x, cp, sc, sh)
        got = ops.cl_from_ncthw(x.cuda(), cp, sc, sh)
        torch.cuda.synchronize()
        _budget("cl_from_ncthw", got, ref, mag, f"C{Cc} Cp{cp} {thw} x{sc}+{sh}")
        assert bool((_bits(got[..., Cc:]) == 0).all()), "pad channels must be exactly +0"
        if (sc, sh) == (1.0, 0.0):
            assert _same_bits(got[..., :Cc], x.permute(1, 2, 3, 0).to(BF)), "scale 1, shift 0 is a correctly rounded copy"


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc,cp,thw", NC.IM2COL_CASES)
def test_cl_im2col3x3(Cc, cp, thw, dt):
    x = NC.layout_input((Cc,) + thw, dt, "im2col", Cc, cp)
    for sc, sh in NC.AFFINE:
        ref, mag = R.cl_im2col3x3_from_ncthw(x, cp, sc, sh)
        got = ops.cl_im2col3x3_from_ncthw(x.cuda(), cp, sc, sh)
        torch.cuda.synchronize()
        _budget("cl_im2col3x3", got, ref, mag, f"C{Cc} Cp{cp} {thw} x{sc}+{sh}")     # mag 0 outside the frame and beyond 9C: exact zeros
        assert bool((_bits(got[..., 9 * Cc:]) == 0).all())


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc,ld,thw", NC.NCTHW_CASES)
def test_ncthw_from_cl(Cc, ld, thw, dt):
    x = NC.layout_input(thw + (ld,), BF, "ncthw", Cc, ld)
    x[..., Cc:] = float("nan")                                  # pad channels of the source are never part of the result
    for sc, sh in NC.AFFINE:
        for lo, hi in ((-float("inf"), float("inf")), NC.CLAMP):
            ref, mag = R.ncthw_from_cl(x, Cc, sc, sh, lo, hi)
            got = ops.ncthw_from_cl(x.cuda(), Cc, dt, sc, sh, lo, hi)
            torch.cuda.synchronize()
            _budget("ncthw_from_cl", got, ref, mag, f"C{Cc} ld{ld} {thw} x{sc}+{sh} [{lo},{hi}]")
            if lo > -1e30 and ref.numel() > 100 and (sc, sh) == (1.7, -0.3):
                g = got.float().cpu()
                assert float(g.min()) == R.f32(lo) and float(g.max()) == R.f32(hi), "the clamp must bite on both sides, exactly"


@pytest.mark.parametrize("T,nb,fe", NC.POOL_CASES)
def test_avgpool_time(T, nb, fe):
    x = NC.layout_input((nb * T, 1, fe // 8, 8), BF, "pool", T, nb, fe)
    ref, mag = R.avgpool_time(x, nb)
    got = ops.avgpool_time(x.cuda(), nb)
    torch.cuda.synchronize()
    assert got.shape == ref.shape
    _budget("avgpool_time", got, ref, mag, f"T{T} nb{nb} frame {fe}")
    assert R.need_k(got, ref, mag) == 0.0, "0.5 (a + b) of two bf16 values is exact in fp32: the result is the correctly rounded mean"


@pytest.mark.parametrize("n,dt", NC.AXPBY_CASES, ids=[f"{n}-{'f32' if dt == torch.float32 else 'bf16'}" for n, dt in NC.AXPBY_CASES])
def test_axpby(n, dt):
    x, y = NC.layout_input((n,), dt, "ax", n), NC.layout_input((n,), dt, "ay", n)
    for a, b in NC.AXPBY_COEF:
        ref, mag = R.axpby(x, y, a, b)
        got = ops.axpby(x.cuda(), y.cuda(), a, b)
        torch.cuda.synchronize()
        _budget("axpby", got, ref, mag, f"n{n} {a} {b}")


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
def test_posterior_sample(dt):
    mom, noise = NC.posterior_input()
    lv = mom.float()[..., 16:32]
    assert float(lv.min()) < -30 and float(lv.max()) > 20
    ref, mag = R.posterior_sample(mom, 16, noise)
    got = ops.posterior_sample(mom.cuda(), 16, noise.cuda(), dt)
    torch.cuda.synchronize()
    _budget("posterior_sample", got, ref, mag, str(dt))
