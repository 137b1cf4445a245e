"""-m gpu: dove_linear_mxfp8 at every walk class of tests/mx_cases.py against the float64 reference at the rounding-level budget of that
module, and dove_mx_quant_bf16 over every block maximum against the exact rule, bit for bit.  A GEMM launch reads its operands from views
inside 0xFF-filled (the e4m3 NaN byte, the largest E8M0 scale) or NaN-filled slabs - a descriptor that is a row or a K-chunk too long reads
NaN, not allocator slack - and writes into a guarded, NaN-prefilled buffer: a store past column N, past row M or before row 0 lands on a guard,
an element nobody writes stays NaN.  (dove_qkv_post_mxfp8 is held to the same module's budget in tests/test_attention_lengths_gpu.py.)"""
import pytest
import torch

import mx_cases as MC
from dove_amd import lib as L
from dove_amd import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")


def slab(t, fill):
    """CUDA copy of `t` as a view into a larger allocation whose other elements are `fill`; the view starts four rows (last-dim pitch) in."""
    pre = 4 * t.shape[-1]
    buf = torch.full((t.numel() + 2 * pre,), fill, dtype=t.dtype, device="cuda")
    v = buf[pre:pre + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def packed_in_slabs(pm, bias=None):
    return ops.PackedMx(slab(pm.q, 0xFF), slab(pm.s, -1), pm.rows, pm.K, None if bias is None else slab(bias, NAN))


def bits(t):
    return t.contiguous().view(torch.int16)


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_class_set_is_complete_at_the_device_cu_count():
    """The keys depend on the compute-unit count (grid, tiles per workgroup, live successors): recomputed for this device, every class must
    still have its case and every row its key."""
    cus = cu_count()
    assert MC.missing_classes(MC.CASES, cus) == []
    assert ["/".join(MC.class_key(c, cus)) for c in MC.CASES] == [c.key for c in MC.CASES]


PARAMS = [(c, f) for c in MC.CASES for f in MC.FAMILIES]


@pytest.mark.parametrize("c,family", PARAMS, ids=[f"{c.name}-{f}" for c, f in PARAMS])
def test_linear_mx_case(c, family):
    """One launch per walk class and operand family against the float64 reference at the case's budget.  On an MI355X the largest k any
    element needs is 465 of 8870 (m300_k1024_ld, blocks); with exactly summed K-64 blocks (literals 1.4 - 54) the kernel needed 40 - 190:
    the instruction's own truncation, which tests/mx_cases.py mfma_sum restates."""
    inp = MC.operands(c, family)
    px, pw = ops.mx_quant(inp["x"].cuda()), ops.mx_quant(inp["w"].cuda())
    torch.cuda.synchronize()
    # the reference multiplies the bytes the GPU quantiser produced (test_mx_quant_sweep holds them to the exact rule)
    inp.update(xq=px.q.cpu(), xe=MC.scale_bytes(px.s.cpu()), wq=pw.q.cpu(), we=MC.scale_bytes(pw.s.cpu()))
    rows = MC.sample_rows(c)
    ref, mag, gterm = MC.reference64(c, inp, rows=rows, cus=cu_count())
    dx, dw = packed_in_slabs(px), packed_in_slabs(pw, inp["bias"])
    resid = None if inp["resid"] is None else slab(inp["resid"], NAN)
    gate = None if inp["gate"] is None else slab(inp["gate"], NAN)
    del px, pw

    def launch(out, r):
        ops.linear_mx(dx, dw, resid=r, gate=gate, gate_split=c.gate_split, act=c.act, out=out)
        torch.cuda.synchronize()

    buf, out = MC.guarded_out(c, "cuda")
    launch(out, resid)
    assert MC.guards_intact(c, buf), f"{c.name}: a store outside [0, M) x [0, N)"
    stored = out[:, :c.N]
    assert not bool(torch.isnan(stored).any()), f"{c.name}: {int(torch.isnan(stored).sum())} elements were never written"
    assert bool(torch.isfinite(stored).all())
    got = (stored if rows is None else stored[rows.cuda()]).double().cpu()
    err = (got - ref).abs()
    tol = MC.budget(c, ref, mag, gterm)
    print(f"{c.name}-{family}: k used {MC.k_of((err - 0.5 * MC.ulp_out(ref)).clamp_min(0), mag, gterm):.3f} of {c.kk}")
    bad = MC.over_budget(got, ref, tol)
    if bool(bad.any()):
        i, j = bad.nonzero()[0].tolist()
        raise AssertionError(f"{c.name}-{family}: {int(bad.sum())}/{bad.numel()} elements over the budget; worst {float((err / tol).max()):.3g}x; "
                             f"first at row {i if rows is None else int(rows[i])} col {j}: got {float(got[i, j])!r} ref {float(ref[i, j])!r} "
                             f"mag {float(mag[i, j]):.4g}")
    want = bits(stored)

    buf2, out2 = MC.guarded_out(c, "cuda")                            # two launches agree bit for bit
    launch(out2, resid)
    assert MC.guards_intact(c, buf2) and torch.equal(bits(out2[:, :c.N]), want), "two launches differ"
    if c.resid and c.ldr_x == c.ldo_x:                                # out is resid
        buf3, out3 = MC.guarded_out(c, "cuda", prefill=resid)
        launch(out3, out3)
        assert MC.guards_intact(c, buf3) and torch.equal(bits(out3[:, :c.N]), want), "in place differs from out of place"
    if buf.numel() > (16 << 20):
        del buf, out, stored, buf2, out2, dx, dw, resid
        torch.cuda.empty_cache()


# ---- the quantiser ----------------------------------------------------------------------------------------------------------------------------
def _guarded_u8(n, pad=256):
    """n bytes of 0x55 inside a flat buffer with `pad` guard bytes (0xA7) on either side."""
    flat = torch.full((n + 2 * pad,), 0xA7, dtype=torch.uint8, device="cuda")
    flat[pad:pad + n] = 0x55
    return flat, flat[pad:pad + n]


def _u8_guards_intact(flat, n, pad=256):
    return bool((flat[:pad] == 0xA7).all()) and bool((flat[pad + n:] == 0xA7).all())


@pytest.mark.parametrize("K,one_row", [(256, False), (512, False), (3072, False), (256, True), (3072, True)])
def test_mx_quant_sweep(K, one_row):
    """Every finite positive bf16 value as a block's maximum (tests/mx_cases.py quant_sweep), K / 256 = 1 / 2 / 12 scale chunks, row counts
    whose thread count rows K / 8 is no multiple of the 256-thread block (one row among them): bytes and scale words bit-identical to the
    exact rule, the scale array fully written, nothing outside q and s touched."""
    x = MC.quant_sweep(K)
    if one_row:
        x = x[x.shape[0] // 2:x.shape[0] // 2 + 1].contiguous()
    rows = x.shape[0]
    assert (rows * K // 8) % 256 != 0
    q_ref, e_ref = MC.quant_exact(x)
    fq, q = _guarded_u8(rows * K)
    fs, s = _guarded_u8(rows * (K // 32))
    xd = slab(x, NAN)
    L.check(L.load().dove_mx_quant_bf16(L.ptr(xd), rows, K, L.ptr(q), L.ptr(s), L.stream_ptr()), "dove_mx_quant_bf16")
    torch.cuda.synchronize()
    assert _u8_guards_intact(fq, rows * K) and _u8_guards_intact(fs, rows * (K // 32)), "wrote outside q or s"
    words = s.cpu().view(torch.int32).reshape(K // 256, rows, 2)
    e_got, q_got = MC.scale_bytes(words), q.cpu().reshape(rows, K)
    if not torch.equal(e_got, e_ref):
        i, j = (e_got != e_ref).nonzero()[0].tolist()
        amax = float(x[i, 32 * j:32 * j + 32].double().abs().max())
        raise AssertionError(f"{int((e_got != e_ref).sum())} scale bytes differ; first at row {i} block {j}: amax {amax!r} = 448 x 2^"
                             f"{torch.log2(torch.tensor(amax / 448.0, dtype=torch.float64)).item():.3f}, got {int(e_got[i, j])} want {int(e_ref[i, j])}")
    assert torch.equal(words, MC.scale_words(e_ref))
    if not torch.equal(q_got, q_ref):
        i, j = (q_got != q_ref).nonzero()[0].tolist()
        raise AssertionError(f"{int((q_got != q_ref).sum())} e4m3 bytes differ; first at row {i} col {j}: x {float(x[i, j])!r} scale byte "
                             f"{int(e_ref[i, j // 32])}, got {int(q_got[i, j]):#x} want {int(q_ref[i, j]):#x}")
    assert torch.equal(MC.dequant64(q_got, e_got), MC.dequant64(q_ref, e_ref))
