"""CPU: the case list of tests/test_attention_lengths_gpu.py is justified by enumeration, its float64 reference sits well inside the
tolerance the kernels are held to, and that tolerance sees the faults the list is meant to catch (a dropped key, a quad-order slip)."""
import pytest
import torch

import attention_cases as A

RTOL, AFRAC = 3e-2, 8e-3              # the attention tolerance of tests/test_ops_gpu.py against the exact softmax
HEADS = 2
SAMPLE_N = (65, 384, 832)


def test_lengths_are_the_stated_list():
    assert len(A.LENGTHS) == 43 == len(set(A.LENGTHS)) and max(A.LENGTHS) == 832 and min(A.LENGTHS) == 1
    for t in range(1, 14):
        assert {64 * (t - 1) + 1, 64 * (t - 1) + 33, 64 * t} <= set(A.LENGTHS)
    assert {96, 127, 352, 383} <= set(A.LENGTHS)


@pytest.mark.parametrize("cls", [A.pipe_class, A.fwd_class], ids=["pipe", "fwd"])
def test_lengths_reach_every_loop_class(cls):
    every = {cls(N) for N in range(1, 64 * A.MAX_TILES + 1)}
    hit = {cls(N) for N in A.LENGTHS}
    assert hit == every, sorted(every - hit)


def test_loop_classes_are_what_the_kernels_do():
    # attn_pipe_kernel: one tile runs no main trip and one tail trip; 5 ragged tiles: last_full = 3, no main trip, two tail trips;
    # 8 full tiles: last_full = 7 -> one main trip, one tail trip; 13 ragged: last_full = 11 -> two main trips, tiles 8 .. 12 = two tail trips
    assert A.pipe_class(1) == (1, True, 0, 1) and A.pipe_class(64) == (1, False, 0, 1)
    assert A.pipe_class(4 * 64 + 1) == (1, True, 0, 2)
    assert A.pipe_class(8 * 64) == (0, False, 1, 1)
    assert A.pipe_class(12 * 64 + 33) == (1, True, 2, 2)
    assert A.pipe_class(6 * 64) == (2, False, 1, 1)
    assert len({A.pipe_class(N) for N in A.LENGTHS}) >= 21
    # attn_fwd_kernel: 1 or 2 tiles leave through the break of the first trip, 3 or 4 run both phases
    assert A.fwd_class(64) == ("break", 1, False, 0) and A.fwd_class(65) == ("break", 2, True, 0)
    assert A.fwd_class(3 * 64) == ("end", 1, False, 0) and A.fwd_class(4 * 64 - 1) == ("end", 2, True, 0)
    assert A.fwd_class(6 * 64) == ("break", 2, False, 1) and A.fwd_class(13 * 64) == ("break", 1, False, 2)


def test_pipe_form_restates_the_launch_rule():
    # 48 heads x 72 query blocks on 256 CUs: 13 whole rounds on <2>, the half round of 128 items on <1>
    assert A.pipe_form(18226, 48, 256) == (3328, 128)
    assert A.pipe_form(300, 2, 256) == (0, 4)
    assert A.pipe_form(300, 65, 256) == (130, 0)               # 130 items: more than half a round stays on <2>
    for N in A.LENGTHS:
        for cus in (256, 304, 64):
            assert A.pipe_form(N, 2, cus) == (0, 2 * A.qblocks(N))
            h = A.pipe2_heads(N, cus)
            assert A.pipe_form(N, h, cus) == (h * A.qblocks(N), 0)


@pytest.mark.parametrize("family", A.FAMILIES)
def test_operand_families(family):
    N = 384
    q, k, v = A.natural(family, N, HEADS)
    Qh, Kh, Vt = A.kernel_layout(q, k, v)
    assert Qh.shape == (HEADS, 384, 64) and Vt.shape == (HEADS, 64, 384)
    Qh, Kh, Vt = A.kernel_layout(*A.natural(family, 300, HEADS))
    assert not Qh[:, 300:].any() and not Kh[:, 300:].any() and Vt.shape[-1] == 384
    assert int((Vt != 0).any(0).any(0).sum()) == 300           # pads zero wherever the swap put them
    s = torch.matmul(q.double(), k.double().transpose(1, 2))
    if family == "selector":
        p = torch.softmax(s * 0.6931471805599453, dim=-1)
        top = p.argmax(-1)
        assert torch.equal(top, torch.arange(N - 1, -1, -1).expand(HEADS, N))   # query i selects key N - 1 - i: every key exactly once
        assert float(p.amax(-1).min()) >= 0.999
        b = 1.01 * (A.norm2(Qh, Kh, 300)[:, 0] * A.norm2(Qh, Kh, 300)[:, 1]).sqrt()
        assert 23.0 < float(b.min()) and float(b.max()) < 26.0
    else:
        assert 3.5 < float(s.std()) < 4.5


@pytest.mark.parametrize("N", SAMPLE_N)
@pytest.mark.parametrize("family", A.FAMILIES)
def test_reference_alone_is_inside_half_the_tolerance(family, N):
    q, k, v = A.natural(family, N, HEADS)
    ratio = A.tolerance_ratio(A.flash_emulation(q, k, v), A.reference(q, k, v), RTOL, AFRAC)
    print(f"flash emulation vs float64 reference, {family} N={N}: worst error / tolerance {float(ratio.max()):.3f}")
    assert float(ratio.max()) < 0.5


def _drop(t, dim, j):
    keep = [i for i in range(t.shape[dim]) if i != j]
    return t.index_select(dim, torch.tensor(keep))


def _mutations(q, k, v):
    N = k.shape[1]
    yield "last key dropped", A.reference(q, k[:, :N - 1], v[:, :, :N - 1])
    yield "key 5 dropped", A.reference(q, _drop(k, 1, 5), _drop(v, 2, 5))
    vs = v.clone()
    vs[:, :, 4:8], vs[:, :, 8:12] = v[:, :, 8:12], v[:, :, 4:8]
    yield "V keys 4-7 <-> 8-11", A.reference(q, k, vs)


@pytest.mark.parametrize("N", SAMPLE_N)
@pytest.mark.parametrize("family", A.FAMILIES)
def test_tolerance_sees_a_dropped_key_and_a_quad_slip(family, N):
    q, k, v = A.natural(family, N, HEADS)
    ref = A.reference(q, k, v)
    for name, wrong in _mutations(q, k, v):
        ratio = A.tolerance_ratio(wrong, ref, RTOL, AFRAC)
        off = int((ratio > 1).sum())
        print(f"{family} N={N} {name}: {off} elements off, worst error / tolerance {float(ratio.max()):.1f}")
        assert off >= 100, (name, off)
