"""No GPU needed: the float64 definitions of tests/glue_ref.py are checked against torch's own float64 operators; the budget constants
K_EMU of tests/glue_cases.py are re-measured on every case of the table (what the fp32 restatements of tests/emu_ops.py need against the
definitions); the table is proved to reach every branch of the kernels (each NIT of rmsnorm with a full and a ragged last iteration, each
tail class of gemv, gated_gelu and attention_bias, each (C, ldp) of conv_out_gather, the grid-stride loop of tile_gather); the two 1 % caps
(undecided gelu roundings, undecided P roundings) hold for the definitions alone; and deliberately wrong restatements miss the budget the
kernels are allowed."""
import functools

import pytest
import torch
import torch.nn.functional as F

import emu_ops as E
import glue_cases as GC
import glue_ref as G
import norm_cases as NC
import norm_ref as R

BF = torch.bfloat16
F64 = torch.float64


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---- the definitions against torch's float64 operators, and the rounding helpers ---------------------------------------------------

def test_ref_rounding_helpers():
    x32 = torch.cat([torch.randn(4096, generator=NC._gen("rne")) * 3, torch.tensor([0.0, 1.0, 1.00390625, 1.01171875, -2.0 ** -130, 3.0e38])])
    want = x32.to(BF).double()                                   # fp32 -> bf16 is one rounding; float64 -> fp32 of these values none
    assert torch.equal(G.rne(x32.double()), want)
    lo, hi, dist = G.neighbours(x32.double())
    assert bool((lo <= x32.double()).all()) and bool((x32.double() <= hi).all())
    assert bool(((hi - lo == R.ulp(x32.double(), BF)) | (hi == lo)).all())
    assert bool(((want == lo) | (want == hi)).all())
    one = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=F64)        # 2^-30 above the boundary between 1 and 1 + 2^-7
    assert G.neighbours(one)[2].item() == pytest.approx(2.0 ** -30) and G.rne(one).item() == 1.0 + 2.0 ** -7
    # a float64 value that the detour through fp32 would round the wrong way: just above a tie, by less than half an fp32 ulp
    assert G.rne(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=F64)).item() == 1.0 + 2.0 ** -7
    x = torch.tensor([3.0, 5.0], dtype=F64)
    assert G.need_k(torch.tensor([3.0, 5.03125], dtype=BF), x, torch.ones(2, dtype=F64), slack=torch.tensor([0.0, 2.0 ** -6], dtype=F64)) == 0.0
    patt = GC.finite_bf16_patterns(65280, "all")
    assert torch.unique(_bits(patt)).numel() == 65280 and bool(torch.isfinite(patt.float()).all())
    w = GC.widen_with_low_bits(patt)
    assert torch.equal(G.rne_bits_bf16(w), _bits(w.to(BF)))      # the integer rounding is torch's fp32 -> bf16, ties and overflow to inf included
    assert int((_bits(w.to(BF)) != _bits(patt)).sum()) > 20000   # and it does round up often


def test_ref_rmsnorm_gelu_gemv_attention_are_torch():
    x, w = GC.rms_input("gaussian3", 5, 520), GC.rms_weight(520)
    y, _ = G.rmsnorm(x, w, GC.RMS_EPS)
    xd = x.double()
    assert _rel(y, xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + R.f32(GC.RMS_EPS)) * w.double()) < 1e-14
    a = torch.linspace(-12, 12, 4001, dtype=F64)
    assert float((G.gelu_tanh(a) - F.gelu(a, approximate="tanh")).abs().max()) < 1e-15
    Wm, b, xv = GC.gemv_input(520, 5)
    assert _rel(G.gemv(Wm, b, xv, 0)[0], Wm.double() @ xv.double() + b.double()) < 1e-14
    assert _rel(G.gemv(Wm, None, xv, 1)[0], Wm.double() @ F.silu(xv.double())) < 1e-14
    qkv, bias = GC.att_input("exact", 65, 3)
    A = G.AttentionBias(qkv, bias, 3)
    assert A.scores_exact
    q, k, v = (qkv.double()[:, i * 192:(i + 1) * 192].reshape(65, 3, 64).transpose(0, 1) for i in range(3))
    full = F.scaled_dot_product_attention(q, k, v, attn_mask=bias.double(), scale=1.0).transpose(0, 1).reshape(65, 192)
    assert float((A.ref - full).abs().max()) < 2.0 ** -8 * float(A.mag.max())       # the definition differs by the bf16 rounding of P only
    assert _rel(torch.softmax(q @ k.transpose(1, 2) + bias.double(), -1), A.p) < 1e-14


def test_ref_patch_index_and_blend_and_gather():
    for pt, p, Cc, T, H, W, _ in GC.PATCH_CASES[:5]:
        assert torch.equal(G.patch_index(T, Cc, H, W, pt, p), G.patch_index_loops(T, Cc, H, W, pt, p))
    case = GC.BLEND_CASES[1]
    a, b = GC.blend_input(case)
    ref, mag, strip = G.blend_edge(a, b, 3, 0)
    for e in range(3):                                           # diffusers' blend_v, spelled out
        want = a.double()[:, a.shape[1] - 3 + e] * (1 - e / 3) + b.double()[:, e] * (e / 3)
        assert torch.equal(ref[:, e], want)
    assert torch.equal(ref[:, 3:], b.double()[:, 3:]) and bool(strip[:, :3].all()) and not bool(strip[:, 3:].any())
    p, bias = GC.cog_input("grid", 3, 28, 2, 9, 65)
    s, _ = G.conv_out_gather(p, 3, bias)
    # the same sum as a 3x3 convolution whose kernel picks plane (dy*3+dx)*C + c at tap (dy, dx)
    wsel = torch.zeros(3, 27, 3, 3, dtype=F64)
    for dy in range(3):
        for dx in range(3):
            for c in range(3):
                wsel[c, (dy * 3 + dx) * 3 + c, dy, dx] = 1
    conv = F.conv2d(p[..., :27].double().permute(0, 3, 1, 2), wsel, bias.double(), padding=1).permute(0, 2, 3, 1)
    assert torch.equal(s, conv)


# ---- the table reaches every branch -------------------------------------------------------------------------------------------------

def test_table_reaches_every_branch():
    # rmsnorm: every NIT 1..8 with a full (64 lanes) and a ragged last iteration; the D the operator's brief names are all there
    assert set(GC.RMS_D) >= {8, 504, 512, 520, 1024, 1528, 2048, 2560, 3072, 3576, 4088, 4096}
    seen = {(GC.rms_nit(D)[0], GC.rms_nit(D)[1] == 64) for D in GC.RMS_D}
    assert seen == {(n, full) for n in range(1, 9) for full in (False, True)}
    assert all(D % 8 == 0 and D <= 4096 for D in GC.RMS_D)
    assert set(GC.RMS_ROWS) == {1, 3, 4, 5, 226} and {r % 4 for r in GC.RMS_ROWS} == {0, 1, 2, 3}
    assert set(GC.RMS_FAMILIES) == {"gaussian3", "spike", "constant", "tiny"}
    x = GC.rms_input("spike", 5, 520).float()
    assert float(x[0, -1].abs()) == 1e3 and int((x.abs() > 1).sum()) == 5
    x = GC.rms_input("constant", 5, 520).float()
    assert bool((x == x[:, :1]).all()) and float(x.abs().min()) > 0
    x = GC.rms_input("tiny", 5, 520).double()
    assert float((x * x).mean(dim=1).max()) < 0.1 * GC.RMS_EPS
    # gated_gelu: a partial last block, many blocks, one thread
    assert set(GC.GG_F) == {8, 16, 1024, 10240} and set(GC.GG_M) == {1, 3, 226}
    threads = [M * F // 8 for M in GC.GG_M for F in GC.GG_F]
    assert any(t % 256 for t in threads) and any(t % 256 == 0 for t in threads) and min(threads) == 1
    a = GC.gg_input("main", 3, 1024).float()[:, :1024]
    assert float(a.min()) == -3.0 and float(a.max()) == 12.0 and bool((a == 0).any())
    assert bool((a == torch.tensor(GC.TINY).to(BF).float()).any()) and bool((a == -torch.tensor(GC.TINY).to(BF).float()).any())
    a = GC.gg_input("tail", 3, 1024).float()[:, :1024]
    assert float(a.min()) == -12.0 and float(a.max()) == -3.0
    # attention_bias: N % 64 in {1, 2, 63, 0}, below / at / above one and two key trips, N = 1024 (the limit), 4 queries a block
    assert {N for N, _ in GC.ATT_CASES} == {1, 2, 63, 64, 65, 128, 226, 1024}
    assert {h for N, h in GC.ATT_CASES if N != 226} == {1, 3} and {h for N, h in GC.ATT_CASES if N == 226} == {1, 3, 64}
    assert {N % 4 for N, _ in GC.ATT_CASES} == {0, 1, 2, 3}
    for N, h in GC.ATT_CASES:
        pi = GC.att_perm(N, h)
        assert torch.equal(pi.sort(dim=1).values, torch.arange(N).expand(h, N)), "every key is selected exactly once a head"
        if h > 1 and N > 2:
            assert not torch.equal(pi[0], pi[1])
    pi = GC.att_perm(226, 3)
    assert all(bool((pi[hh] == key).any()) for hh in range(3) for key in (0, 63, 64, 65, 225))
    # gemv: out % 4 classes with one and many blocks; one lane, 63 lanes, exactly one trip, one trip + one lane, six trips
    assert set(GC.GEMV_IN) == {8, 504, 512, 520, 3072} and set(GC.GEMV_OUT) == {1, 3, 4, 5, 701}
    assert any(o % 4 and o > 4 for o in GC.GEMV_OUT) and {i % 512 == 0 for i in GC.GEMV_IN} == {True, False}
    # patchify: every (pt, p), C = 1 and 16, H != W, totals that are and are not whole blocks, ld = features and more, 128 features
    assert {(c[0], c[1]) for c in GC.PATCH_CASES} == {(1, 1), (1, 2), (2, 2)} and {c[2] for c in GC.PATCH_CASES} == {1, 16}
    assert all(c[4] != c[5] for c in GC.PATCH_CASES)
    totals = [c[2] * c[3] * c[4] * c[5] for c in GC.PATCH_CASES]
    assert any(t % 256 for t in totals) and any(t % 256 == 0 for t in totals) and max(totals) <= 65280
    assert {c[6] > 0 for c in GC.PATCH_CASES} == {True, False}
    assert any(c[2] * c[0] * c[1] * c[1] == 128 for c in GC.PATCH_CASES)
    # blend_edge: the blended axis longer in a, and longer in b, for both axes; every ld and T; totals below and above one block
    for axis in (0, 1):
        diffs = {(c[2][axis] > c[3][axis]) for c in GC.BLEND_CASES if c[0] == axis}
        assert diffs == {True, False} and all(c[2][axis] != c[3][axis] and c[2][1 - axis] == c[3][1 - axis] for c in GC.BLEND_CASES if c[0] == axis)
    assert {c[4] for c in GC.BLEND_CASES} == {4, 8, 32} and {c[1] for c in GC.BLEND_CASES} == {1, 3}
    gran = [c[1] * e * (c[3][1] if c[0] == 0 else c[3][0]) * c[4] // 4 for c in GC.BLEND_CASES for e in GC.blend_extents(c)]
    assert min(gran) < 256 and max(gran) > 256 and any(g % 256 for g in gran)
    assert all({1, 2} <= set(GC.blend_extents(c)) and min(c[2][c[0]], c[3][c[0]]) in GC.blend_extents(c) for c in GC.BLEND_CASES)
    # conv_out_gather: every C, ldp = 9 C and more, the raised LDS limit, frames below / at / above one 8 x 64 block
    assert set(GC.COG_CLDP) == {(1, 12), (1, 36), (2, 20), (3, 28), (3, 32), (4, 36)}
    assert set(GC.COG_HW) == {(1, 1), (7, 63), (8, 64), (9, 65), (17, 130)} and set(GC.COG_T) == {1, 2} and set(GC.COG_LDY) == {4, 8, 32}
    assert max(10 * 66 * (ldp + 1) * 4 for _, ldp in GC.COG_CLDP) == 97680 > 65536
    # tile_gather: more 16-byte chunks than the capped grid has threads, by less than a tenth; a tile as tall as the frame
    assert GC.TG_GRID_CAP < GC.tg_chunks(GC.TG_BIG) < 1.1 * GC.TG_GRID_CAP
    assert GC.TG_BIG["th"] == GC.TG_BIG["H"] and 27 <= GC.TG_BIG["C"]
    org = GC.tg_origins(GC.TG_BIG, GC.TG_BIG["nb"])
    assert org[0][1] == 0 and org[-1][1] == GC.TG_BIG["W"] - GC.TG_BIG["tw"] and len(set(org)) > 8


# ---- K_EMU: what the fp32 restatements need, on exactly the GPU test's inputs --------------------------------------------------------

def _report(op, k):
    print(f"k_emu {op} = {k:.3f} (constant {GC.K_EMU[op]})")
    assert k <= GC.K_EMU[op], (op, k)


def test_k_emu_rmsnorm():
    worst = 0.0
    for D in GC.RMS_D:
        w = GC.rms_weight(D)
        for rows in GC.RMS_ROWS:
            for family in GC.RMS_FAMILIES:
                x = GC.rms_input(family, rows, D)
                ref, mag = G.rmsnorm(x, w, GC.RMS_EPS)
                worst = max(worst, R.need_k(E.rmsnorm(x, w, GC.RMS_EPS), ref, mag))
                if family == "constant":                        # w sign(x) up to eps
                    xd = x.double()
                    assert float((ref - w.double() * xd.sign()).abs().max()) <= GC.RMS_EPS / float((xd * xd).min()) * float(w.abs().max())
    _report("rmsnorm", worst)


def test_k_emu_gated_gelu_and_the_band_cap():
    worst = tail = 0.0
    for M in GC.GG_M:
        for Fh in GC.GG_F:
            x = GC.gg_input("main", M, Fh)
            gg = G.GatedGelu(x)
            worst = max(worst, gg.need_k(E.gated_gelu(x)))
            if M * Fh >= 1024:                                   # a share of fewer elements than 100 / cap says nothing
                share = gg.band_share(GC.allowed_k("gated_gelu"))
                print(f"gated_gelu main {M}x{Fh}: {share:.5f} of the elements undecided at k = {GC.allowed_k('gated_gelu')}")
                assert share <= GC.GG_BAND_CAP
            x = GC.gg_input("tail", M, Fh)
            ref, mag, slack = G.GatedGelu(x).tail()
            tail = max(tail, G.need_k(E.gated_gelu(x), ref, mag, slack=slack))
    _report("gated_gelu", worst)
    _report("gated_gelu_tail", tail)


@pytest.mark.parametrize("N,heads", GC.ATT_CASES)
def test_k_emu_attention_bias_and_the_b_cap(N, heads):
    # selection: the restatement returns v[pi(i)] bit for bit, as the kernel must
    qkv, bias = GC.att_input("selection", N, heads)
    want = G.selected_rows(qkv, GC.att_perm(N, heads))
    assert _same_bits(E.attention_bias(qkv, bias, heads), want)
    A = G.AttentionBias(qkv, bias, heads)                        # the definition agrees: the other keys weigh 4e-18 each
    assert float((A.ref - want.double()).abs().max()) <= 1e-14 * float(want.double().abs().max())
    # uniform: P = rne(1 / N) for every key, none of them near a boundary
    qkv, bias = GC.att_input("uniform", N, heads)
    A = G.AttentionBias(qkv, bias, heads)
    assert A.scores_exact and A.share(GC.allowed_k("attention_uniform")) == 0.0
    ku = R.need_k(E.attention_bias(qkv, bias, heads), A.ref, A.mag)
    # exact scores: the only inner rounding left is P to bf16
    qkv, bias = GC.att_input("exact", N, heads)
    A = G.AttentionBias(qkv, bias, heads)
    assert A.scores_exact
    share = A.share(GC.allowed_k("attention_exact"))
    got = E.attention_bias(qkv, bias, heads)
    k0 = R.need_k(got, A.ref, A.mag)
    ke = G.need_k(got, A.ref, A.mag, slack=A.slack(GC.K_EMU["attention_exact"]))
    print(f"attention_bias N {N} heads {heads}: k_emu uniform {ku:.3f}, exact {ke:.3f} ({k0:.3f} with no key undecided), "
          f"{share:.5f} of the keys undecided at k = {GC.allowed_k('attention_exact')}")
    if N * N * heads >= 1024:
        assert share <= GC.ATT_B_CAP
    assert ku <= GC.K_EMU["attention_uniform"] and ke <= GC.K_EMU["attention_exact"]


def test_k_emu_gemv():
    worst = {0: 0.0, 1: 0.0}
    for in_f in GC.GEMV_IN:
        for out_f in GC.GEMV_OUT:
            Wm, b, x = GC.gemv_input(in_f, out_f)
            for act in (0, 1):
                for bias in (b, None):
                    ref, mag = G.gemv(Wm, bias, x, act)
                    worst[act] = max(worst[act], R.need_k(E.gemv(Wm, bias, x, act), ref, mag))
    print(f"k_emu gemv = {worst[0]:.3f}, gemv_silu = {worst[1]:.3f}")
    _report("gemv", worst[0])
    _report("gemv_silu", worst[1])


def test_k_emu_blend_edge():
    worst = 0.0
    for case in GC.BLEND_CASES:
        a, b = GC.blend_input(case)
        for extent in GC.blend_extents(case):
            ref, mag, strip = G.blend_edge(a, b, extent, case[0])
            got = E.blend_edge(a.clone(), b.clone(), extent, case[0])
            worst = max(worst, R.need_k(got, ref, mag))
            assert _same_bits(got[~strip], b[~strip])
    _report("blend_edge", worst)


@pytest.mark.parametrize("Cc,ldp", GC.COG_CLDP)
def test_k_emu_conv_out_gather(Cc, ldp):
    worst = 0.0
    for H, W in GC.COG_HW:
        for T in GC.COG_T:
            p, bias = GC.cog_input("grid", Cc, ldp, T, H, W)
            for bs in (bias, None):
                s, mag = G.conv_out_gather(p, Cc, bs)
                assert bool((mag < 32).all()) and torch.equal(s.float().double(), s), "the grid family sums exactly in fp32"
                want = G.rne(s)
                assert torch.equal(E.conv_out_gather_cl(p, Cc, bs, 8)[..., :Cc].double(), want)
                assert torch.equal(E.conv_out_gather(p, Cc, bs, BF).double(), want.permute(3, 0, 1, 2))
            p, bias = GC.cog_input("gaussian", Cc, ldp, T, H, W)
            for bs in (bias, None):
                s, mag = G.conv_out_gather(p, Cc, bs)
                worst = max(worst, R.need_k(E.conv_out_gather_cl(p, Cc, bs, 8)[..., :Cc], s, mag))
    print(f"k_emu conv_out_gather C {Cc} ldp {ldp} = {worst:.3f}")
    assert worst <= GC.K_EMU["conv_out_gather"]


def test_patchify_restatement_is_the_permutation():
    for pt, p, Cc, T, H, W, extra in GC.PATCH_CASES:
        feat = Cc * pt * p * p
        x = GC.finite_bf16_patterns(T * Cc * H * W, pt, p, Cc).reshape(T, Cc, H, W)
        idx = G.patch_index(T, Cc, H, W, pt, p)
        tok = E.patchify(x, pt, p, feat + extra)
        assert _same_bits(tok[:, :feat], x.reshape(-1)[idx]) and bool((_bits(tok[:, feat:]) == 0).all())
        assert _same_bits(E.unpatchify(tok, T, Cc, H, W, pt, p, BF), x)


def test_tile_gather_restatement_is_the_im2col_of_the_cropped_tile():
    c = dict(GC.TG_SMALL, nb=5)
    src = GC.tg_source(c, 3)
    x = E.cl_im2col3x3_from_ncthw(src, c["C"])
    org = GC.tg_origins(c, 5)
    got = E.tile_gather(x, c["t0"], c["nt"], c["th"], c["tw"], org, im2col_cin=3)
    for n, (oy, ox) in enumerate(org):
        crop = src[:, c["t0"]:c["t0"] + c["nt"], oy:oy + c["th"], ox:ox + c["tw"]]
        assert _same_bits(got[n * c["nt"]:(n + 1) * c["nt"]], E.cl_im2col3x3_from_ncthw(crop, c["C"]))


# ---- discrimination: wrong restatements miss the KERNEL's allowance ---------------------------------------------------------------------

def _rms_wrong(x, w, eps, mut):
    xf = x.float()
    D = xf.shape[1]
    ss = (xf[:, :D - 8] if mut == "drop_tail" and D > 8 else xf).pow(2).sum(-1, keepdim=True)
    if mut == "mean_sub":
        ss = (xf - xf.mean(-1, keepdim=True)).pow(2).sum(-1, keepdim=True)
    wf = w.float().roll(-1) if mut == "w+1" else w.float()
    return (xf * torch.rsqrt(ss / D + (eps * 10 if mut == "eps10" else eps)) * wf).to(BF)


@pytest.mark.parametrize("mut", ["eps10", "drop_tail", "w+1", "mean_sub"])
def test_wrong_rmsnorm_misses_the_budget(mut):
    killed = None
    for D in (520, 4088):
        w = GC.rms_weight(D)
        for family in GC.RMS_FAMILIES:
            x = GC.rms_input(family, 5, D)
            ref, mag = G.rmsnorm(x, w, GC.RMS_EPS)
            assert R.within(_rms_wrong(x, w, GC.RMS_EPS, None), ref, mag, GC.allowed_k("rmsnorm"))
            if not R.within(_rms_wrong(x, w, GC.RMS_EPS, mut), ref, mag, GC.allowed_k("rmsnorm")):
                killed = f"{family} D {D}"
    print(f"rmsnorm {mut}: fails at {killed}")
    assert killed is not None


@pytest.mark.parametrize("mut", ["no_inner_rounding", "erf_gelu", "gate_is_a", "row_stride_F"])
def test_wrong_gated_gelu_misses_the_band(mut):
    M, Fh = 3, 1024
    x = GC.gg_input("main", M, Fh)
    a, b = x.float()[:, :Fh], x.float()[:, Fh:]
    if mut == "no_inner_rounding":                               # gelu kept in fp32 up to the product
        got = (F.gelu(a, approximate="tanh") * b).to(BF)
    elif mut == "erf_gelu":
        got = (F.gelu(a).to(BF).float() * b).to(BF)
    elif mut == "gate_is_a":
        got = (F.gelu(b, approximate="tanh").to(BF).float() * a).to(BF)
    else:                                                        # rows read at stride F instead of 2 F
        flat = x.float().reshape(-1)
        rows = torch.stack([flat[r * Fh:r * Fh + 2 * Fh] for r in range(M)])
        got = (F.gelu(rows[:, :Fh], approximate="tanh").to(BF).float() * rows[:, Fh:]).to(BF)
    gg = G.GatedGelu(x)
    assert gg.need_k(E.gated_gelu(x)) <= GC.allowed_k("gated_gelu")
    k = gg.need_k(got)
    print(f"gated_gelu {mut}: needs a band of {k}")
    assert k > GC.allowed_k("gated_gelu")


def _att_wrong(qkv, bias, heads, mut):
    N, D = qkv.shape[0], heads * 64
    q, k, v = (qkv.float()[:, i * D:(i + 1) * D].reshape(N, heads, 64).permute(1, 0, 2) for i in range(3))
    if mut == "head0_v":
        v = v[:1].expand(heads, N, 64)
    if mut == "key+1":
        bias = bias.roll(1, dims=2)
    s = (torch.einsum("hqd,hkd->hqk", q, k).to(BF).float() + bias.to(BF).float()).to(BF).float()
    if mut == "scaled":
        s = s / 8
    if mut == "drop_last_key" and N > 1:
        s[..., -1] = -1e30
    p = torch.softmax(s, dim=-1)
    if mut != "p_fp32":
        p = p.to(BF).float()
    return torch.einsum("hqk,hkd->hqd", p, v).permute(1, 0, 2).reshape(N, D).to(BF)


@functools.lru_cache(maxsize=None)
def _att_refs(N, heads):
    out = {}
    for family in GC.ATT_FAMILIES:
        qkv, bias = GC.att_input(family, N, heads)
        out[family] = (qkv, bias, G.AttentionBias(qkv, bias, heads))
    return out


def _att_passes(N, heads, mut):
    """The GPU test's three checks on a restatement; -> the family that fails, or None."""
    refs = _att_refs(N, heads)
    for family, (qkv, bias, A) in refs.items():
        got = _att_wrong(qkv, bias, heads, mut)
        if family == "selection":
            ok = _same_bits(got, G.selected_rows(qkv, GC.att_perm(N, heads)))
        else:
            k = GC.allowed_k("attention_" + family)
            ok = G.need_k(got, A.ref, A.mag, slack=A.slack(k) if family == "exact" else None) <= k
        if not ok:
            return family
    return None


@pytest.mark.parametrize("mut", ["head0_v", "key+1", "scaled", "drop_last_key", "p_fp32"])
def test_wrong_attention_bias_misses_the_budget(mut):
    assert _att_passes(65, 3, None) is None
    killed = _att_passes(65, 3, mut)
    print(f"attention_bias {mut}: fails in family {killed}")
    assert killed is not None


def test_wrong_gemv_blend_gather_miss_the_budget():
    Wm, b, x = GC.gemv_input(520, 5)
    ref, mag = G.gemv(Wm, b, x, 1)
    assert not R.within(Wm.float()[:, :512] @ F.silu(x[:512]) + b, ref, mag, GC.allowed_k("gemv_silu")), "a dropped K tail"
    assert not R.within(Wm.float() @ x + b, ref, mag, GC.allowed_k("gemv_silu")), "a dropped activation"
    assert not R.within(E.gemv(Wm, b.roll(1), x, 1), ref, mag, GC.allowed_k("gemv_silu")), "a neighbour's bias"
    case = GC.BLEND_CASES[0]                                      # Ha = 5, Hb = 3
    a, bb = GC.blend_input(case)
    ref, mag, _ = G.blend_edge(a, bb, 2, 0)
    wrong = bb.clone().float()
    for e in range(2):                                           # a's row taken from b's height
        wrong[:, e] = a.float()[:, bb.shape[1] - 2 + e] * (1 - e / 2) + bb.float()[:, e] * (e / 2)
    assert not R.within(wrong.to(BF), ref, mag, GC.allowed_k("blend_edge"))
    assert R.within(E.blend_edge(a.clone(), bb.clone(), 2, 0), ref, mag, GC.allowed_k("blend_edge"))
    p, bias = GC.cog_input("gaussian", 3, 32, 1, 9, 65)
    s, mag = G.conv_out_gather(p, 3, bias)
    pt = p.clone()
    pt[..., :27] = p[..., :27].reshape(1, 9, 65, 3, 3, 3).transpose(3, 4).reshape(1, 9, 65, 27)      # taps transposed (dy <-> dx)
    assert not R.within(E.conv_out_gather_cl(pt, 3, bias, 8)[..., :3], s, mag, GC.allowed_k("conv_out_gather"))
