"""No GPU needed: the float64 definitions of tests/norm_ref.py are checked against torch's own float64 operators; the budget constants
K_EMU / C_EMU of tests/norm_cases.py are re-measured on every case of the table (what the fp32 restatements of tests/emu_ops.py, and an
fp32 emulation of the statistics kernel's summation order, need against the definitions); and the deliberately wrong fp32
restatements must each MISS the budget the kernels are allowed on at least one case, so that the GPU test cannot pass a kernel that
makes one of those mistakes."""
import functools

import pytest
import torch
import torch.nn.functional as F

import emu_ops as E
import norm_cases as NC
import norm_ref as R

BF = torch.bfloat16
F64 = torch.float64


# ---- the definitions against torch's float64 operators ---------------------------------------------------------------------------

def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("family", NC.FAMILIES)
def test_ref_groupnorm_is_torch_group_norm(family):
    case = NC.STATS_CASES[2]
    x = NC.stats_input(case, family)
    gamma, beta = NC.channel_params(case[1], "t")
    st, _ = R.gn_stats(x, 1e-6)
    y, _ = R.gn_apply(x, st, gamma, beta, silu=False)
    assert _rel(y, R.torch_group_norm(x, 1e-6, gamma, beta)) < 1e-12
    ys, _ = R.gn_apply(x, st, gamma, beta, silu=True)
    assert _rel(ys, F.silu(R.torch_group_norm(x, 1e-6, gamma, beta))) < 1e-12
    # sums -> statistics is the same thing up to the one-pass variance's own conditioning in float64
    s, _ = R.gn_sums(x)
    st2, _ = R.gn_from_sums(s, x.numel() // 32, 1e-6)
    msg = torch.cat([s.reshape(-1), torch.tensor([x.numel() // 32], dtype=F64)])
    assert torch.equal(R.gn_from_sums(msg, None, 1e-6)[0], st2)
    assert _rel(st2, st) < 1e-9


@pytest.mark.parametrize("N,D", NC.LN_CASES)
def test_ref_layernorm_is_torch_layer_norm(N, D):
    x, gamma, beta, mod = NC.ln_input(N, D, "plain")
    y, _ = R.ln_mod(x, gamma, beta, 1e-5)
    assert _rel(y, F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), R.f32(1e-5))) < 1e-12
    split = N // 4
    ym, _ = R.ln_mod(x, gamma, beta, 1e-5, mod, split)
    cls = (torch.arange(N) >= split).long()
    want = y * (1 + mod.double()[cls, 1]) + mod.double()[cls, 0]
    assert _rel(ym, want) < 1e-12


@pytest.mark.parametrize("T,Tz,hz,wz,sshift", [(5, 3, 4, 6, 2), (3, 3, 5, 4, 0), (4, 2, 3, 5, 1), (9, 3, 2, 3, 3)])
def test_ref_gather_is_nearest_interpolate(T, Tz, hz, wz, sshift):
    Cc, H, W = 32, hz << sshift, wz << sshift
    x = NC.family_input("plain", (T, H, W, Cc), "g")
    yb = NC.yb_table((Tz, hz, wz, 2 * Cc), "g")
    gamma, beta = NC.channel_params(Cc, "g")
    st, _ = R.gn_stats(x, 1e-6)
    got, _ = R.gn_apply(x, st, gamma, beta, silu=False, yb=yb, Tz=Tz, sshift=sshift, tmap=NC.nearest_tmap(T, Tz))
    up = F.interpolate(yb.double().permute(3, 0, 1, 2)[None], size=(T, H, W), mode="nearest")[0].permute(1, 2, 3, 0)
    base, _ = R.gn_apply(x, st, gamma, beta, silu=False)
    assert _rel(got, base * up[..., :Cc] + up[..., Cc:]) < 1e-12


def test_ref_ulp_and_budget():
    v = torch.tensor([1.0, 1.5, 2.0, 3.0e-39, 0.0, -260.0], dtype=F64)
    assert R.ulp(v, BF).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0]
    assert R.ulp(v, torch.float32)[:3].tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22]
    ref = torch.tensor([1.0 + 2.0 ** -9], dtype=F64)
    assert R.need_k(torch.tensor([1.0], dtype=BF), ref, torch.ones(1, dtype=F64)) == 0.0
    assert R.need_k(torch.tensor([1.0 + 2.0 ** -7], dtype=BF), ref, torch.ones(1, dtype=F64)) == pytest.approx(2.0 ** -9 / R.U24)
    assert R.need_k(torch.tensor([1.0 + 2.0 ** -7], dtype=BF), ref, torch.zeros(1, dtype=F64)) == float("inf")


# ---- fp32 restatements with a switch for one deliberate mistake ---------------------------------------------------------------------

def kernel_order_partials(x, nb=1):
    """fp32 emulation of gn_partial_kernel's documented order -> partial rows [frames * blocks, 64] fp32 as the kernel writes them:
    per-thread running sums over that thread's pixels (stride blocks x lanes), then the lanes in turn, then the group's channels."""
    Cc = x.shape[-1]
    frames, fp = (x.shape[0], x.shape[1] * x.shape[2]) if x.dim() == 4 else (1, x.shape[0])
    nsub, bpf = NC.blocks_per_frame(fp, Cc)
    xf = x.float().reshape(frames, fp, Cc)
    stride = bpf * nsub
    trips = -(-fp // stride)
    xp = F.pad(xf, (0, 0, 0, trips * stride - fp)).reshape(frames, trips, bpf, nsub, Cc)
    s = torch.zeros(frames, bpf, nsub, Cc)
    ss = torch.zeros(frames, bpf, nsub, Cc)
    for t in range(trips):
        s = s + xp[:, t]
        ss = ss + xp[:, t] * xp[:, t]
    cs, css = torch.zeros(frames, bpf, Cc), torch.zeros(frames, bpf, Cc)
    for k in range(nsub):
        cs, css = cs + s[:, :, k], css + ss[:, :, k]
    cpg = Cc // 32
    cs, css = cs.reshape(frames, bpf, 32, cpg), css.reshape(frames, bpf, 32, cpg)
    gs, gss = torch.zeros(frames, bpf, 32), torch.zeros(frames, bpf, 32)
    for k in range(cpg):
        gs, gss = gs + cs[..., k], gss + css[..., k]
    return torch.stack([gs, gss], dim=-1).reshape(frames * bpf, 64)


def r32_gn_stats(x, eps, nb=1, mut=None):
    rows = kernel_order_partials(x)
    count = x.numel() // 32 // nb
    if mut == "eps10":
        eps = eps * 10
    st = r32_from_partials(rows, nb, count, eps)
    if mut == "inst0_stats" and nb > 1:
        st = st[:1].expand(nb, 32, 2).contiguous()
    return st


def r32_from_partials(rows, nb, count, eps, mut=None):
    r = rows.reshape(nb, -1, 32, 2)
    if mut == "fp32_combine":                                   # the rows summed in fp32, in order; the finalisation stays fp64
        s = torch.zeros(nb, 32, 2)
        for i in range(r.shape[1]):
            s = s + r[:, i]
        s = s.double()
    else:
        s = r.double().sum(dim=1)
    mean = s[..., 0] / count
    var = (s[..., 1] / count - mean * mean).clamp_min(0)
    st = torch.stack([mean, 1.0 / torch.sqrt(var + R.f32(eps))], dim=-1).float()
    return st[0] if nb == 1 else st


def r32_gn_apply(x, stats, gamma, beta, silu=True, yb=None, Tz=0, sshift=0, tmap=None, nb=1, mut=None):
    TT, H, W, Cc = x.shape
    T, cpg = TT // nb, Cc // 32
    st = stats.float().reshape(nb, 32, 2)
    if mut == "inst0_stats":
        st = st[:1].expand(nb, 32, 2)
    gidx = torch.arange(Cc) // (cpg + 1 if mut == "cpg+1" else cpg)
    gam = gamma.float().roll(-1) if mut == "gamma+1" else gamma.float()
    sc = st[:, gidx, 1] * gam
    sh = beta.float() - st[:, gidx, 0] * sc
    y = x.float().reshape(nb, T, H, W, Cc) * sc[:, None, None, None] + sh[:, None, None, None]
    if yb is not None:
        tm = list(tmap)
        if mut == "tmap+1":
            tm = tm[1:] + [0]
        tz = torch.arange(nb)[:, None] * (0 if mut == "yb_block0" else Tz) + torch.tensor(tm)[None]
        hi = (torch.arange(H) + ((1 << sshift) - 1 if mut == "h_ceil" else 0)) >> sshift
        g = yb.float()[tz.reshape(-1)][:, hi.clamp_max(yb.shape[1] - 1)][:, :, torch.arange(W) >> sshift].reshape(nb, T, H, W, 2 * Cc)
        y = y * g[..., :Cc] + g[..., Cc:]
    if silu:
        y = torch.sigmoid(y) if mut == "silu_no_mul" else F.silu(y)
    return y.reshape(TT, H, W, Cc).to(BF)


def r32_ln(x, gamma, beta, eps, mod=None, split=0, mut=None):
    xf = x.float()
    N, D = xf.shape
    mean = xf.mean(dim=1, keepdim=True)
    if mut == "one_pass":
        var = ((xf * xf).mean(dim=1, keepdim=True) - mean * mean).clamp_min(0)
    else:
        var = ((xf - mean) ** 2).sum(dim=1, keepdim=True) / (D - 1 if mut == "d-1" else D)
    if mut == "mean_ulp":                                       # what another summation order may do to the mean; var as before
        mean = mean * (1 + 2.0 ** -23)
    rstd = 1.0 / torch.sqrt(var + (eps * 10 if mut == "eps10" else eps))
    gam = gamma.float().roll(-1) if mut == "gamma+1" else gamma.float()
    y = (xf - mean) * rstd * gam + beta.float()
    if mod is not None:
        rows = torch.arange(N)
        m = mod.float()[((rows > split) if mut == "row<=split" else (rows >= split)).long()]
        shift, scale = (m[:, 1], m[:, 0]) if mut == "swap_shift_scale" else (m[:, 0], m[:, 1])
        y = y * (1 + scale) + shift
    return y.to(BF)


# ---- shared, cached case data ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _apply_case(ci, family):
    case = NC.APPLY_CASES[ci]
    name, Cc, nb, (T, H, W), ybs, sshift, tmap = case
    x, gamma, beta, yb = NC.apply_input(case, family)
    st = R.gn_stats(x, 1e-6, nb)[0].float()
    return x, gamma, beta, yb, st


def _apply_variants(ci):
    ybs = NC.APPLY_CASES[ci][4]
    return [(silu, with_yb) for silu in (False, True) for with_yb in ((False, True) if ybs else (False,))]


def _apply_op(silu, with_yb):
    return ("sn_apply" if with_yb else "gn_apply") + ("_silu" if silu else "")


def _apply_ref(ci, family, silu, with_yb):
    name, Cc, nb, (T, H, W), ybs, sshift, tmap = NC.APPLY_CASES[ci]
    x, gamma, beta, yb, st = _apply_case(ci, family)
    kw = dict(yb=yb, Tz=ybs[0], sshift=sshift, tmap=tmap) if with_yb else {}
    return R.gn_apply(x, st, gamma, beta, silu=silu, nb=nb, **kw), kw


# ---- K_EMU / C_EMU: what the fp32 restatements need, on exactly the GPU test's inputs ----------------------------------------------

def test_k_emu_ln_mod():
    worst = const = 0.0
    for N, D in NC.LN_CASES:
        for family in NC.LN_FAMILIES:
            x, gamma, beta, mod = NC.ln_input(N, D, family)
            for eps in NC.LN_EPS:
                for m in (None, mod):
                    for split in (NC.ln_splits(N) if m is not None else [0]):
                        ref, mag = R.ln_mod(x, gamma, beta, eps, m, split)
                        got = E.layernorm_modulate(x, gamma, beta, eps, m, split)
                        worst = max(worst, R.need_k(got, ref, mag))
                        if family == "constant-rows":           # x - mean is exactly 0: the output is B, and only B's two terms may round
                            const = max(const, R.need_k(got, *R.ln_constant_rows(x, gamma, beta, m, split)))
    print(f"k_emu ln_mod = {worst:.3f}, on constant rows against B alone = {const:.3f}")
    assert worst <= NC.K_EMU["ln_mod"]
    assert const <= NC.K_EMU["ln_constant_rows"]


@pytest.mark.parametrize("ci", range(len(NC.APPLY_CASES)), ids=[c[0] for c in NC.APPLY_CASES])
def test_k_emu_gn_apply(ci):
    name, Cc, nb, (T, H, W), ybs, sshift, tmap = NC.APPLY_CASES[ci]
    worst = {}
    for family in NC.FAMILIES:
        x, gamma, beta, yb, st = _apply_case(ci, family)
        for silu, with_yb in _apply_variants(ci):
            (ref, mag), kw = _apply_ref(ci, family, silu, with_yb)
            ekw = dict(yb=yb, sshift=sshift, tmap=tmap) if with_yb else {}
            got = E.groupnorm_apply(x, st, gamma, beta, silu=silu, nb=nb, **ekw)
            op = _apply_op(silu, with_yb)
            worst[op] = max(worst.get(op, 0.0), R.need_k(got, ref, mag))
            # the switchable restatement used for the mutants is the same arithmetic when nothing is switched
            if x.numel() < 1 << 20:
                assert torch.equal(r32_gn_apply(x, st, gamma, beta, silu=silu, nb=nb, **kw).view(torch.int16), got.view(torch.int16))
    _apply_case.cache_clear()
    print(f"k_emu {name}: " + ", ".join(f"{k} = {v:.3f}" for k, v in worst.items()))
    for op, v in worst.items():
        assert v <= NC.K_EMU[op], (op, v)


@pytest.mark.parametrize("case", NC.STATS_CASES, ids=[c[0] for c in NC.STATS_CASES])
def test_c_emu_gn_stats_in_kernel_order(case):
    name, Cc, shape, nb = case
    worst = 0.0
    for family in NC.FAMILIES:
        x = NC.stats_input(case, family)
        ref, mag = R.gn_stats(x, 1e-6, nb)
        worst = max(worst, R.need_k(r32_gn_stats(x, 1e-6, nb), ref, mag))
        if nb == 1:
            rows = kernel_order_partials(x)
            s, smag = R.gn_sums(x)
            cs = R.need_k(rows.double().reshape(-1, 32, 2).sum(dim=0), s, smag, dtype=F64)
            assert cs <= NC.C_EMU["gn_sums"], cs
            print(f"c_emu gn_sums {name}/{family} = {cs:.3f}")
            # emu_ops' float64 one-pass statistics are the definition's, to float64 conditioning
            assert R.need_k(E.groupnorm_stats(x, 1e-6), ref, mag) <= 1e-3
    print(f"c_emu gn_stats {name} = {worst:.3f}")
    assert worst <= NC.C_EMU["gn_stats"]


def test_from_partials_restatement_is_within_one_ulp():
    for rows in NC.PARTIAL_ROWS:
        for nb in NC.PARTIAL_NB:
            p, count = NC.partial_rows(rows, nb)
            ref, _ = R.gn_from_partials(p, nb, count, 1e-6)
            var = 1.0 / ref[..., 1] ** 2 - R.f32(1e-6)
            assert float((var / ref[..., 0] ** 2).min()) >= 1e-4                  # so that an fp64 reordering is invisible in fp32
            assert R.ulps_off(r32_from_partials(p, nb, count, 1e-6), ref) <= 1.0


def test_k_emu_layout():
    worst = {}

    def note(op, got, ref_mag):
        worst[op] = max(worst.get(op, 0.0), R.need_k(got, *ref_mag))

    for Cc, cp, thw in NC.CL_CASES:
        for dt in (torch.float32, BF):
            x = NC.layout_input((Cc,) + thw, dt, "cl", Cc, cp)
            for sc, sh in NC.AFFINE:
                note("cl_from_ncthw", E.cl_from_ncthw(x, cp, sc, sh), R.cl_from_ncthw(x, cp, sc, sh))
    for Cc, cp, thw in NC.IM2COL_CASES:
        for dt in (torch.float32, BF):
            x = NC.layout_input((Cc,) + thw, dt, "im2col", Cc, cp)
            for sc, sh in NC.AFFINE:
                note("cl_im2col3x3", E.cl_im2col3x3_from_ncthw(x, cp, sc, sh), R.cl_im2col3x3_from_ncthw(x, cp, sc, sh))
    for Cc, ld, thw in NC.NCTHW_CASES:
        x = NC.layout_input(thw + (ld,), BF, "ncthw", Cc, ld)
        for dt in (torch.float32, BF):
            for sc, sh in NC.AFFINE:
                for lo, hi in ((-float("inf"), float("inf")), NC.CLAMP):
                    note("ncthw_from_cl", E.ncthw_from_cl(x, Cc, dt, sc, sh, lo, hi), R.ncthw_from_cl(x, Cc, sc, sh, lo, hi))
    for T, nb, fe in NC.POOL_CASES:
        x = NC.layout_input((nb * T, 1, fe // 8, 8), BF, "pool", T, nb, fe)
        got = E.avgpool_time(x, nb)
        note("avgpool_time", got, R.avgpool_time(x, nb))
        assert R.need_k(got, *R.avgpool_time(x, nb)) == 0.0                     # exact arithmetic: correctly rounded
    for n, dt in NC.AXPBY_CASES:
        x, y = NC.layout_input((n,), dt, "ax", n), NC.layout_input((n,), dt, "ay", n)
        for a, b in NC.AXPBY_COEF:
            note("axpby", E.axpby(x, y, a, b), R.axpby(x, y, a, b))
    mom, noise = NC.posterior_input()
    for dt in (torch.float32, BF):
        note("posterior_sample", E.posterior_sample(mom, 16, noise, dt), R.posterior_sample(mom, 16, noise))
    print("k_emu layout: " + ", ".join(f"{k} = {v:.3f}" for k, v in worst.items()))
    for op, v in worst.items():
        assert v <= NC.K_EMU[op], (op, v)


# ---- discrimination: every wrong restatement misses the KERNEL's allowance on at least one case ------------------------------------

def _ln_killed(mut):
    for N, D in NC.LN_CASES:
        for family in NC.LN_FAMILIES:
            x, gamma, beta, mod = NC.ln_input(N, D, family)
            for eps in NC.LN_EPS:
                for split in NC.ln_splits(N):
                    ref, mag = R.ln_mod(x, gamma, beta, eps, mod, split)
                    if not R.within(r32_ln(x, gamma, beta, eps, mod, split, mut=mut), ref, mag, NC.allowed_k("ln_mod")):
                        return f"ln {N}x{D} {family} eps {eps} split {split}"
    return None


def _ln_constant_killed(mut):
    """Only the constant-row bound (against B alone) is consulted: the general budget's mag carries rstd = eps^-1/2 there."""
    for N, D in NC.LN_CASES:
        x, gamma, beta, mod = NC.ln_input(N, D, "constant-rows")
        for eps in NC.LN_EPS:
            B, magB = R.ln_constant_rows(x, gamma, beta, mod, N // 4)
            if not R.within(r32_ln(x, gamma, beta, eps, mod, N // 4, mut=mut), B, magB, NC.allowed_k("ln_constant_rows")):
                return f"ln constant rows {N}x{D} eps {eps}"
    return None


def _apply_killed(mut):
    for ci in (7, 6, 3, 4, 2, 1):                               # the small cases; any one is enough
        name, Cc, nb, (T, H, W), ybs, sshift, tmap = NC.APPLY_CASES[ci]
        for family in NC.FAMILIES:
            x, gamma, beta, yb, st = _apply_case(ci, family)
            for silu, with_yb in _apply_variants(ci):
                (ref, mag), kw = _apply_ref(ci, family, silu, with_yb)
                got = r32_gn_apply(x, st, gamma, beta, silu=silu, nb=nb, mut=mut, **kw)
                if not R.within(got, ref, mag, NC.allowed_k(_apply_op(silu, with_yb))):
                    return f"apply {name} {family} silu {silu} yb {with_yb}"
    return None


def _stats_killed(mut):
    for case in (NC.STATS_CASES[7], NC.STATS_CASES[0], NC.STATS_CASES[3]):
        for family in NC.FAMILIES:
            x = NC.stats_input(case, family)
            ref, mag = R.gn_stats(x, 1e-6, case[3])
            if not R.within(r32_gn_stats(x, 1e-6, case[3], mut=mut), ref, mag, NC.allowed_c("gn_stats")):
                return f"stats {case[0]} {family}"
    return None


def _partials_killed(mut):
    for rows in NC.PARTIAL_ROWS:
        for nb in NC.PARTIAL_NB:
            p, count = NC.partial_rows(rows, nb)
            ref, _ = R.gn_from_partials(p, nb, count, 1e-6)
            if R.ulps_off(r32_from_partials(p, nb, count, 1e-6, mut=mut), ref) > 1.0:
                return f"partials rows {rows} nb {nb}"
    return None


MUTANTS = [
    ("eps x 10 (LayerNorm)", _ln_killed, "eps10"),
    ("eps x 10 (GroupNorm statistics)", _stats_killed, "eps10"),
    ("variance over D - 1", _ln_killed, "d-1"),
    ("one-pass fp32 E[x^2] - mean^2", _ln_killed, "one_pass"),
    ("mean off by one fp32 ulp on constant rows", _ln_constant_killed, "mean_ulp"),
    ("fp32 combine of partial rows", _partials_killed, "fp32_combine"),
    ("gamma[ch + 1] (GroupNorm apply)", _apply_killed, "gamma+1"),
    ("gamma[c + 1] (LayerNorm)", _ln_killed, "gamma+1"),
    ("group index with cpg + 1", _apply_killed, "cpg+1"),
    ("shift and scale swapped", _ln_killed, "swap_shift_scale"),
    ("row <= split", _ln_killed, "row<=split"),
    ("tmap[t + 1]", _apply_killed, "tmap+1"),
    ("(h + (1 << sshift) - 1) >> sshift", _apply_killed, "h_ceil"),
    ("instance 0's yb block for every instance", _apply_killed, "yb_block0"),
    ("instance 0's statistics for every instance (apply)", _apply_killed, "inst0_stats"),
    ("instance 0's statistics for every instance (statistics)", _stats_killed, "inst0_stats"),
    ("SiLU without the multiply by x", _apply_killed, "silu_no_mul"),
]


@functools.lru_cache(maxsize=None)
def _clean(hunt):
    return hunt(None)


@pytest.mark.parametrize("what,hunt,mut", MUTANTS, ids=[m[2] + "-" + m[1].__name__[1:-7] for m in MUTANTS])
def test_wrong_restatement_misses_the_budget(what, hunt, mut):
    assert _clean(hunt) is None, "the unmutated restatement must pass everywhere the mutant is hunted"
    killed = hunt(mut)
    print(f"{what}: fails at {killed}")
    assert killed is not None, f"{what} survives every case of the table"
