"""CPU: the case table of tests/mx_cases.py - its class keys and their completeness at 256 compute units, the budget's k against the fp32 chain
restatement of the MXFP8 GEMM's K order, and the proof that the budget discriminates: each wrong restatement below, evaluated in float64 and
rounded once like the kernel's output, must leave the budget on every case of the class it belongs to.  Then the exact quantiser rule against
emu_ops.mx_quant_ref and torch's own e4m3 cast, and the Q8 / K8 budget of dove_qkv_post_mxfp8 against emu_ops' fp32 restatement and seven
wrong ones."""
import math

import pytest
import torch

import emu_ops as E
import mx_cases as MC

BF = torch.bfloat16
_memo = {}


def ref_of(c, family):
    """(operands, rows, ref, mag, gterm), computed once per case and family and never modified."""
    if (c.name, family) not in _memo:
        inp = MC.quantise_cpu(MC.operands(c, family))
        rows = MC.sample_rows(c)
        _memo[(c.name, family)] = (inp, rows) + MC.reference64(c, inp, rows=rows)
    return _memo[(c.name, family)]


def test_names_are_unique_and_every_row_has_its_literals():
    assert len({c.name for c in MC.CASES}) == len(MC.CASES) == len(MC.EXPECT)
    assert sum(c.sampled for c in MC.CASES) <= 4
    assert all(c.kk >= 1.0 and c.key for c in MC.CASES)
    assert len({c.key for c in MC.CASES}) == len(MC.CASES)          # one case per class


@pytest.mark.parametrize("c", MC.CASES, ids=[c.name for c in MC.CASES])
def test_class_key_is_the_rows_literal(c):
    assert "/".join(MC.class_key(c, 256)) == c.key


def test_every_class_has_a_case():
    assert MC.missing_classes(MC.CASES, 256) == []


def test_decode_visits_every_tile_once_and_the_hand_over_classes_are_what_the_keys_say():
    for c in MC.CASES:
        g = MC.geometry(c)
        seen = [MC.decode(t, g["ntiles"], g["tiles_n"]) for t in range(g["ntiles"])]
        assert sorted(seen) == [(m, n) for m in range(g["tiles_m"]) for n in range(g["tiles_n"])], c.name
        live = sum(b + g["G"] < g["ntiles"] for b in range(g["G"]))     # workgroups whose first successor is on-stream
        want = {"off": live == 0, "mixed": 0 < live < g["G"], "live": live == g["G"]}
        assert want[dict(f.split("=") for f in MC.class_key(c) if "=" in f and not f.startswith("ld"))["succ"]], c.name
    c = MC.by_name("gm8_ragged")
    g = MC.geometry(c)
    wrong = {MC.decode(t, g["ntiles"], g["tiles_n"], gm8_always=True) for t in range(g["ntiles"])}
    assert len(wrong) < g["ntiles"] or max(m for m, _ in wrong) >= g["tiles_m"]


def test_sampled_rows_cover_what_they_must():
    for c in MC.CASES:
        rows = MC.sample_rows(c)
        if rows is None:
            continue
        have = set(rows.tolist())
        tiles_m = (c.M + 255) // 256
        assert {0, c.M - 1} <= have and {r // 256 for r in have} == set(range(tiles_m))
        for t0 in (0, (tiles_m - 1) * 256):
            for b in range(t0, min(t0 + 257, c.M + 1), 32):
                assert {r for r in (b - 1, b) if 0 <= r < c.M} <= have, (c.name, b)
        if c.gate:
            assert {c.gate_split - 1, c.gate_split} <= have


@pytest.mark.parametrize("c", MC.CASES, ids=[c.name for c in MC.CASES])
def test_chain_meets_the_budget_and_k_is_pinned(c):
    """k_chain over both families (at MC.chain_rows of the case's rows); the row's literal k lies in [16, 16.2] k_chain (or is 1 at the
    floor); the chain, rounded once to bf16, meets the budget."""
    kc = 0.0
    for fam in MC.FAMILIES:
        inp, rows, ref, mag, gterm = ref_of(c, fam)
        sel = MC.chain_rows(c, torch.arange(c.M) if rows is None else rows)
        chain = MC.chain32(c, inp, sel if rows is None else rows[sel])
        ref, mag, gterm = ref[sel], mag[sel], gterm[sel]
        kc = max(kc, MC.k_of((chain.double() - ref).abs(), mag, gterm))
        assert not bool(MC.over_budget(chain.to(BF), ref, MC.budget(c, ref, mag, gterm)).any()), (c.name, fam)
    print(f"{c.name}: k_chain {kc:.4f}, k {c.kk}")
    assert (c.kk == 1.0 and 16 * kc <= 1.0) or 16 * kc <= c.kk <= 16.2 * kc, (c.name, kc, c.kk)


# wrong restatement -> the cases of its class (None: every case); EVERY listed case must catch it
_ALL = [c.name for c in MC.CASES if not c.x_zero]                   # the K walk's mutants need products
_GATE = [c.name for c in MC.CASES if c.gate]
MUTANTS = {
    "drop_step": _ALL,
    "next_tile_chunk": _ALL,
    "u_plus": _ALL,
    "u_minus": _ALL,
    "h_swap": _ALL,
    "row_next": _ALL,
    "chunk_next": _ALL,
    "gm8_always": [c.name for c in MC.CASES if "gm=8ragged" in c.key],
    "gate_off1": [n for n in _GATE if MC.by_name(n).gate_split < MC.by_name(n).M],
    "gate_swap": _GATE,
    "resid_after_round": [c.name for c in MC.CASES if c.resid],
    "bias_neighbour": [c.name for c in MC.CASES if c.bias],
    # erf-GELU differs from the tanh form by at most 4.7e-4 (near |v| = 2.2): below 16 x the instruction's own truncation wherever 64 Gaussian
    # products are summed (k 2^-24 1.13 mag with k in the thousands and mag >= |v|), so its class is the case that sums none
    "gelu_erf": [c.name for c in MC.CASES if c.act and c.x_zero],
    "ldr_as_ldo": [c.name for c in MC.CASES if c.resid and c.ldr_x != c.ldo_x],
}
MUTANT_PAIRS = [(m, n) for m, names in MUTANTS.items() for n in names]


def test_every_mutant_has_its_class():
    assert all(MUTANTS.values())


@pytest.mark.parametrize("mut,name", MUTANT_PAIRS, ids=[f"{m}-{n}" for m, n in MUTANT_PAIRS])
def test_budget_rejects_wrong_restatement(mut, name):
    c = MC.by_name(name)
    caught = 0
    for fam in MC.FAMILIES:
        inp, rows, ref, mag, gterm = ref_of(c, fam)
        wrong = MC.reference64(c, inp, rows=rows, mut=mut)[0].to(BF)
        caught += int(MC.over_budget(wrong, ref, MC.budget(c, ref, mag, gterm)).sum())
    assert caught > 0, f"{mut} passes the budget on {name}: the case table is too weak"


@pytest.mark.parametrize("c", [c for c in MC.CASES if c.M % 256], ids=[c.name for c in MC.CASES if c.M % 256])
def test_rows_past_m_land_on_the_guards(c):
    """Rows past M that are neither zeroed nor dropped: with finite poison behind the operand they are finite values stored behind row M - the
    guard rows catch them on every case with a ragged last row tile."""
    inp, rows, ref, mag, gterm = ref_of(c, "blocks")
    buf, out = MC.guarded_out(c)
    assert MC.guards_intact(c, buf) and bool(torch.isnan(out[:, :c.N]).all()) and out.shape == (c.M, c.ldo)
    MC.rows_past_m_store(c, inp, buf)
    assert not MC.guards_intact(c, buf)


# ---- the quantiser ----------------------------------------------------------------------------------------------------------------------------
def test_power_of_two_helper_is_exact():
    k = torch.arange(-400, 401)
    assert MC._p2(k).tolist() == [2.0 ** int(i) for i in k]


def test_exact_e4m3_rounding_agrees_with_torch_on_every_tie_and_neighbour():
    """Every e4m3 value, every midpoint between neighbours and the fp32 values on either side of each, both signs: torch's cast from fp32 is
    round-to-nearest-even too."""
    vals = torch.arange(0, 0x7F, dtype=torch.uint8).view(MC.F8).float()
    mid = (vals[:-1] + vals[1:]) / 2
    pts = torch.cat([vals, mid, torch.nextafter(mid, torch.tensor(math.inf)), torch.nextafter(mid, torch.tensor(-math.inf))])
    pts = torch.cat([pts, -pts])
    assert torch.equal(MC.e4m3_rne_bytes(pts), pts.to(MC.F8).view(torch.uint8))


@pytest.mark.parametrize("K", [256, 512, 3072])
def test_exact_rule_agrees_with_mx_quant_ref_where_amax_over_448_is_a_normal_fp32(K):
    x = MC.quant_sweep(K)
    rows = x.shape[0]
    assert (rows * K // 8) % 256 != 0                                 # a thread count that is no multiple of the 256-thread block
    q, e = MC.quant_exact(x)
    qr, er = E.mx_quant_ref(x)
    amax = x.double().reshape(rows, K // 32, 32).abs().amax(dim=2)
    normal = (amax == 0) | (amax / 448.0 >= 2.0 ** -126)
    assert int((~normal).sum()) > 400                                 # the band below 448 2^-126 is in the sweep
    assert torch.equal(e[normal], er[normal])
    nb = normal[..., None].expand(rows, K // 32, 32).reshape(rows, K)
    assert torch.equal(q[nb], qr.view(torch.uint8)[nb])
    # every block's scale is the smallest admissible one, and nothing above 448 is converted (asserted inside e4m3_rne_bytes too)
    s = MC._p2(e.to(torch.int64) - 127)
    assert bool((amax / s <= 448).all()) and bool(((amax / (s / 2) > 448) | (e == 0)).all())
    assert torch.equal(MC.scale_bytes(MC.scale_words(e)), e) and torch.equal(MC.scale_words(e), E.mx_scale_words(e))


def test_sweep_holds_every_block_maximum_and_the_edges():
    x = MC.quant_sweep(256).double().reshape(-1, 32)
    amax = x.abs().amax(dim=1)
    assert len(torch.unique(amax[amax > 0])) == 0x7F7F                # every finite positive bf16 value
    arg = x.abs().argmax(dim=1)
    assert len(torch.unique(arg)) == 32
    first = x[torch.arange(x.shape[0]), arg]
    assert bool((first > 0).any()) and bool((first < 0).any())
    assert bool(((x == 0) & torch.signbit(x)).any())                  # -0
    assert bool(((x != 0) & (x.abs() < 2.0 ** -126)).any())           # bf16 subnormals
    q, e = MC.quant_exact(MC.quant_sweep(256))
    qb = q.reshape(-1, 32)
    xs = x / MC._p2(e.reshape(-1).to(torch.int64) - 127)[:, None]
    frac = xs.abs() * 512                                             # in units of the subnormal step
    assert bool(((xs != 0) & ((qb & 0x7F) == 0)).any())               # rounds to zero
    assert bool((((qb & 0x78) == 0) & ((qb & 0x7F) != 0)).any())      # rounds into the subnormals
    assert bool((frac == 0.5).any())                                  # the underflow tie
    ulp = MC.ulp_e4m3(xs)
    on_tie = ((xs.abs() / ulp) % 1.0) == 0.5
    assert int(on_tie.sum()) > 100000                                 # ties of the normal binades and of the subnormals


# ---- dove_qkv_post_mxfp8 ------------------------------------------------------------------------------------------------------------------------
QSCALE = 0.125 * math.log2(math.e)
QKV_CPU = [(70, 2, 0, True), (70, 2, 30, True), (129, 1, 129, True), (200, 3, 26, False)]


def _qkv_case(N, heads, tl, rope):
    qkv, aff, cos, sin = MC.qkv_operands(N, heads, tl, rope)
    return qkv, aff, cos, sin, MC.qkv_ref64(qkv, N, heads, tl, aff, cos, sin, QSCALE, 1e-6)


@pytest.mark.parametrize("N,heads,tl,rope", QKV_CPU)
def test_qkv_emulation_meets_the_budget_and_k_emu_is_an_upper_bound(N, heads, tl, rope):
    qkv, aff, cos, sin, (Q, mQ, K, mK) = _qkv_case(N, heads, tl, rope)
    Qf, Kf, Vf = E.qkv_post_mx_f32(qkv, N, N, heads, tl, *aff, cos, sin, QSCALE, 1e-6)
    for got, ref, mag in ((Qf, Q, mQ), (Kf, K, mK)):
        k_emu = float(((got.double() - ref).abs() / (MC.EPS24 * mag)).max())
        print(f"qkv_post_mx emulation N={N}: k_emu {k_emu:.3f}")
        assert k_emu <= MC.K_EMU_QKV
        got8 = got.to(MC.F8).double()
        assert bool(((got8 - ref).abs() <= MC.qkv_budget(ref, mag)).all())
    npad = (N + 127) // 128 * 128
    V8, Vs = MC.v_exact(qkv, N, npad, heads)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    Q8, K8, V8e, Vse = u8(heads, npad, 64), u8(heads, npad, 64), u8(heads, 64, npad), u8(heads, npad // 64, 64, 2)
    E.qkv_post_mx(qkv, N, npad, heads, tl, *aff, cos, sin, QSCALE, 1e-6, Q8, K8, V8e, Vse)
    assert torch.equal(V8, V8e) and torch.equal(Vs, Vse)              # bf16 V of ordinary magnitude: the fp32-log2 rule and the exact one agree


QKV_MUTANTS = ["eps10", "var_d1", "gk_for_gq", "rope_on_text", "table_row_off1", "pair_swapped", "q_not_x8"]


@pytest.mark.parametrize("mut", QKV_MUTANTS)
def test_qkv_budget_rejects_wrong_restatement(mut):
    N, heads, tl = 70, 2, 30
    qkv, aff, cos, sin, (Q, mQ, K, mK) = _qkv_case(N, heads, tl, True)
    if mut == "eps10":                                                # eps matters where the variance is small: rows of a tiny spread
        qkv = (qkv.float() * 2e-3).to(BF)
        Q, mQ, K, mK = MC.qkv_ref64(qkv, N, heads, tl, aff, cos, sin, QSCALE, 1e-6)
    wQ, _, wK, _ = MC.qkv_ref64(qkv, N, heads, tl, aff, cos, sin, QSCALE, 1e-6, mut=mut)
    caught = int(((wQ.float().to(MC.F8).double() - Q).abs() > MC.qkv_budget(Q, mQ)).sum())
    if mut != "q_not_x8":
        caught = min(caught, int(((wK.float().to(MC.F8).double() - K).abs() > MC.qkv_budget(K, mK)).sum())) if mut != "gk_for_gq" else caught
    assert caught > 0, f"{mut} passes the budget"
