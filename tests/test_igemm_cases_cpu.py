"""CPU: the case table of tests/igemm_cases.py against the library's own dispatch (no launch: the reporting entry points only), the budget's
k against the fp32 chain restatement of every kernel's K order, and the proof that the budget discriminates: each wrong restatement below,
evaluated in float64 and rounded once like a kernel's output, must leave the budget on the cases of the class it belongs to."""
import ctypes as C
import os

import pytest
import torch

import emu_ops as E
import igemm_cases as IC
from dove_amd import lib as L

BF = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


_memo = {}


def ref_of(c, family):
    """(operands, rows, ref, mag, gterm, chain32), computed once per case and family and never modified."""
    if (c.name, family) not in _memo:
        inp = IC.operands(c, family)
        rows = IC.sample_rows(c)
        _memo[(c.name, family)] = (inp, rows) + IC.reference64(c, inp, rows=rows, chain=True)
    return _memo[(c.name, family)]


def test_names_are_unique_and_every_row_has_its_literals():
    assert len({c.name for c in IC.CASES}) == len(IC.CASES) == len(IC.EXPECT)
    assert sum(c.sampled for c in IC.CASES) <= 4                 # the largest cases only
    assert all(c.kk >= 1.0 and c.key for c in IC.CASES)


@pytest.mark.parametrize("c", IC.CASES, ids=[c.name for c in IC.CASES])
def test_class_key_agrees_with_the_library(lib, c):
    """At 256 compute units: what cu_count() reports without a device and what an MI355X has."""
    key = IC.class_key(c, 256)
    assert "/".join(key) == c.key
    q = IC.lib_desc(c, L)
    assert lib.dove_conv_kernel_name(C.byref(q)).decode() == IC.KERNEL_NAME[key[0]]
    assert int(lib.dove_conv_partial_launches(C.byref(q))) == IC.partial_launches(c, 256)
    assert int(lib.dove_conv_gn_partial_rows(C.byref(q))) == IC.gn_partial_rows(IC.desc(c))
    if c.name in IC.NEAR_MISSES:
        assert key[0] == IC.NEAR_MISSES[c.name]


def test_every_class_has_a_case():
    assert IC.missing_classes(IC.CASES, 256) == []
    assert set(IC.NEAR_MISSES) <= {c.name for c in IC.CASES}


def test_kpart_case_takes_the_partial_launch_and_near_misses_do_not():
    assert IC.partial_launches(IC.by_name("h_kpart_cut")) == 1 and IC.partial_launches(IC.by_name("h_kpart_uncut")) == 1
    assert sum(IC.partial_launches(c) for c in IC.CASES) == 2


@pytest.mark.parametrize("c", IC.CASES, ids=[c.name for c in IC.CASES])
def test_chain_meets_the_budget_and_k_is_pinned(c):
    """k_chain over both families; the row's literal k lies in [16, 64] k_chain (or is 1 at the floor); the chain, rounded once to the
    output format, meets the budget."""
    kc = 0.0
    for fam in IC.FAMILIES:
        inp, rows, ref, mag, gterm, chain = ref_of(c, fam)
        kc = max(kc, IC.k_of((chain.double() - ref).abs(), mag, gterm))
        got = chain if c.out_f32 else chain.to(BF)
        assert bool(((got.double() - ref).abs() <= IC.budget(c, ref, mag, gterm)).all()), (c.name, fam)
    print(f"{c.name}: k_chain {kc:.3f}, k {c.kk}")
    assert (c.kk == 1.0 and 16 * kc <= 1.0) or 16 * kc <= c.kk <= 64 * kc, (c.name, kc, c.kk)
    assert c.kk == 1.0 or c.kk <= 16 * kc * 1.01, (c.name, kc, c.kk)        # the literal IS 16 k_chain (rounded up to three digits)


def _emu_applies(c):
    """The emulation computes the per-tap conv: the same function as the launch wherever no pack-time weight sum is in use."""
    d = IC.desc(c)
    kern = IC.select_kernel(d)
    return not c.sampled and kern != "halo4x_sub" and not (kern == "halo4x" and d["kt"] == 3 and (d["w_first"] or d["tdup"]))


EMU_CASES = [c for c in IC.CASES if _emu_applies(c)]


EMU_PARAMS = [(c, f) for c in EMU_CASES for f in IC.FAMILIES]


@pytest.mark.parametrize("c,family", EMU_PARAMS, ids=[f"{c.name}-{f}" for c, f in EMU_PARAMS])
def test_emulation_meets_the_budget(c, family):
    """emu_ops.linear for the token-major rows, emu_ops.conv for the rest."""
    inp, rows, ref, mag, gterm, _ = ref_of(c, family)
    d = IC.desc(c)
    cache = inp["cache"]
    if cache is not None and c.nb == 1:
        cache = cache[0]
    if c.k == (1, 1, 1) and c.T == 1 and c.H == 1 and c.nb == 1:
        out = E.linear(inp["x"].view(c.W, -1), inp["pc"], resid=None if inp["resid"] is None else inp["resid"].view(c.W, -1), gate=inp["gate"],
                       gate_split=c.gate_split, act=c.act)
    else:
        out = E.conv(inp["x"], inp["pc"], cache=cache, stride=c.stride, pad=(d["pad_h"], d["pad_w"]), up=c.up, tmode=c.tmode,
                     t_out=d["t_out"], resid=inp["resid"], gate=inp["gate"], gate_split=c.gate_split, act=c.act, out_f32=c.out_f32, nb=c.nb)
    got = out.reshape(-1, out.shape[-1])[:, :d["cout_store"]].double()
    assert bool(((got - ref).abs() <= IC.budget(c, ref, mag, gterm)).all())


GN_CASES = [c for c in IC.CASES if c.gn]
GN_RAGGED = ["h_gn128", "h_gn256_resid", "u_t0_lowres_small", "s_t0_ragged", "s_t0_gn256"]


@pytest.mark.parametrize("c", GN_CASES, ids=[c.name for c in GN_CASES])
def test_gn_partials_budget_and_rows_past_the_edge(c):
    """The fused GroupNorm partial sums: an fp32 restatement meets K_GN; on every case with a ragged tile, rows / columns past the image
    entering the sums (the 'rows >= M of the last tile contribute' mutant) leave it."""
    d = IC.desc(c)
    inp, rows, ref, mag, gterm, chain = ref_of(c, "plain")
    stored = chain.to(BF).view(c.nb * d["t_out"], d["h_out"], d["w_out"], d["cout_store"])
    want, pm = IC.gn_partials64(c, stored)
    assert want.shape == (IC.gn_partial_rows(d), 64)
    tol = IC.K_GN * IC.EPS24 * pm
    got, _ = IC.gn_partials64(c, stored, dtype=torch.float32)     # fp32 sums over the same pixels, in another order
    assert got.dtype == torch.float32 and bool(((got.double() - want).abs() <= tol).all())
    wrong, _ = IC.gn_partials64(c, stored, mut="rows_past_edge")
    caught = int(((wrong - want).abs() > tol).sum())
    assert (caught > 0) == (c.name in GN_RAGGED), (c.name, caught)
    assert set(GN_RAGGED) <= {g.name for g in GN_CASES}


# wrong restatement -> the cases of the class it belongs to; EVERY listed case must catch it
MUTANTS = {
    "drop_chunk": ["h_cache_2ct", "s_t0_ragged", "u_t2_2ct", "f_kt3_frame0", "g_plain_1row", "sk_lt32", "l_up_t0"],
    "border_kept": ["h_wfirst", "h_min16", "u_t0_lowres_small", "l_up_t0", "h_miss_h15"],
    "border_zeroed": ["h_wfirst", "h_min16", "u_t0_lowres_small", "l_up_t0", "h_miss_h15"],
    "front_frame0": ["h_cache_2ct", "h_nb2_strided", "f_kt3_cache_nb2", "f_32x32_f32_cache"],
    "front_other": ["h_nocache_plain", "f_kt3_frame0", "h_miss_cin32"],
    "wfirst_swap": ["h_wfirst"],
    "wpair_parity": ["h_tdup1_cache", "h_tdup1_nocache", "h_tdup2"],
    "tdup2_as_1": ["h_tdup2"],
    "tmode_swap": ["u_t1_no_wsub", "u_t2_2ct", "s_t1_exact", "s_t2_2ct", "l_up_t1", "l_up_t2"],
    "sub_phase": ["s_t0_ragged", "s_t1_exact", "s_t2_2ct"],
    "resid_after_round": ["g_resid_full", "g_gate_129", "h_resid_ldr", "h_gn256_resid", "f_64x64_even_resid"],
    "gate_off1": ["g_gate_129", "g_gate_inplace", "f_128x64_nk2_gate"],
    "gate_unshifted": ["g_split_gate_main", "g_split_gate_edge", "g_split_gate_tail"],
    "bias_quad": ["g_plain_1row", "h_min16", "sk_lt32", "f_128x64_nk1", "s_t0_ragged"],
    "gelu_on_gate": ["g_gate_129", "f_128x64_nk2_gate"],
    "gelu_missing": ["g_gelu_le128", "g_split_gelu", "f_128x32_odd_gelu"],
    "gelu_erf": ["g_gelu_le128", "g_split_gelu", "f_128x32_odd_gelu"],
    "stride_origin": ["f_s2_even", "f_s2_odd"],
}
MUTANT_PAIRS = [(m, n) for m, names in MUTANTS.items() for n in names]


@pytest.mark.parametrize("mut,name", MUTANT_PAIRS, ids=[f"{m}-{n}" for m, n in MUTANT_PAIRS])
def test_budget_rejects_wrong_restatement(mut, name):
    c = IC.by_name(name)
    caught = 0
    for fam in IC.FAMILIES:
        inp, rows, ref, mag, gterm, _ = ref_of(c, fam)
        wrong = IC.reference64(c, inp, rows=rows, mut=mut)[0]
        wrong = wrong.float() if c.out_f32 else wrong.to(BF)
        caught += int(((wrong.double() - ref).abs() > IC.budget(c, ref, mag, gterm)).sum())
    assert caught > 0, f"{mut} passes the budget on {name}: the case table is too weak"
