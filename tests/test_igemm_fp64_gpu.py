"""-m gpu: every kernel behind dove_conv_igemm_bf16 at every walk class of tests/igemm_cases.py, against the float64 reference at the
rounding-level budget of that module.  Each launch reads its operands from views inside NaN-filled slabs (a descriptor that is a row, a
chunk or a tap too long reads NaN, not allocator slack) and writes into a guarded, NaN-prefilled buffer (a store past cout_store, past
row M or past the last frame lands on a guard; an element nobody writes stays NaN)."""
import ctypes as C
import dataclasses

import pytest
import torch

import igemm_cases as IC
from dove_amd import lib as L
from dove_amd import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
GUARD = -1232.0                                     # exact in bf16 and fp32, nothing a case computes
GUARD_FRAMES = 2
PAD_POISON = 7.0
_OWN = object()


def slab(t):
    """CUDA copy of `t` as a view into a larger allocation whose other elements are NaN; the view starts four rows (last-dim pitch) in."""
    pre = 4 * t.shape[-1]
    buf = torch.full((t.numel() + 2 * pre,), NAN, dtype=t.dtype, device="cuda")
    v = buf[pre:pre + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def strided_cache(cache):
    """[nb, kt-1, H, W, C] as the VAE hands it over: the last frames of each instance of a longer, NaN-filled batch (stride(0) > size)."""
    nb, k = cache.shape[:2]
    full = slab(torch.full((nb, k + 1) + tuple(cache.shape[2:]), NAN, dtype=cache.dtype))
    v = full[:, 1:]
    v.copy_(cache)
    return v


def device_operands(c, inp, pad_poison=False):
    x, cache = inp["x"], inp["cache"]
    if pad_poison:
        x = x.clone()
        x[..., c.cin:] = PAD_POISON
        if cache is not None:
            cache = cache.clone()
            cache[..., c.cin:] = PAD_POISON
    pc = inp["pc"]
    pc = dataclasses.replace(pc, w=slab(pc.w), bias=None if pc.bias is None else slab(pc.bias),
                             w_first=None if pc.w_first is None else slab(pc.w_first), w_sub=None if pc.w_sub is None else slab(pc.w_sub),
                             w_pair=None if pc.w_pair is None else slab(pc.w_pair))
    if cache is not None:
        cache = strided_cache(cache) if c.cache == "s" else slab(cache)
        if c.nb == 1:
            cache = cache[0]
    return dict(x=slab(x), cache=cache, pc=pc, resid=None if inp["resid"] is None else slab(inp["resid"]),
                gate=None if inp["gate"] is None else slab(inp["gate"]))


def guarded_out(c, d, prefill=None):
    """([frames + 4, Ho, Wo, ldo] buffer, its interior view): guard value in the two frames (rows of a GEMM) before and after and in the columns
    [cout_store, ldo); the stored columns NaN, or `prefill` (the residual of an in-place launch)."""
    F = c.nb * d["t_out"]
    dt = torch.float32 if c.out_f32 else BF
    buf = torch.full((F + 2 * GUARD_FRAMES, d["h_out"], d["w_out"], d["ldo"]), GUARD, dtype=dt, device="cuda")
    out = buf[GUARD_FRAMES:GUARD_FRAMES + F]
    out[..., :d["cout_store"]] = NAN
    if prefill is not None:
        out.copy_(prefill)
    return buf, out


def guards_intact(buf, d):
    g = GUARD_FRAMES
    return bool((buf[:g] == GUARD).all()) and bool((buf[-g:] == GUARD).all()) and bool((buf[g:-g, ..., d["cout_store"]:] == GUARD).all())


def launch(c, d, dev, out, *, resid=_OWN, gn=None, nb=None, sl=None):
    """One dove_conv_igemm_bf16 call of the case on the device operands (sl: one instance of an nb > 1 case, as a call of its own)."""
    x, cache, r = dev["x"], dev["cache"], dev["resid"] if resid is _OWN else resid
    nb = c.nb if nb is None else nb
    if sl is not None:
        x = x[sl * c.T:(sl + 1) * c.T]
        cache = None if cache is None else cache[sl]
        r = None if r is None else r[sl * d["t_out"]:(sl + 1) * d["t_out"]]
    gn = c.gn if gn is None else gn
    return ops.conv(x, dev["pc"], cache=cache, stride=c.stride, pad=(d["pad_h"], d["pad_w"]), up=c.up, tmode=c.tmode, t_out=d["t_out"],
                    resid=r, gate=dev["gate"], gate_split=c.gate_split, act=c.act, ldo=d["ldo"], out=out, gn_eps=1e-6 if gn else None,
                    out_f32=c.out_f32, nb=nb, tdup=c.tdup, weight_sums=c.wsums)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_class_set_is_complete_at_the_device_cu_count():
    """The keys depend on the compute-unit count (tiles per workgroup, tail split, partial-tile launch): recomputed for this device, every
    class must still have its case and every row its key."""
    cus = cu_count()
    assert IC.missing_classes(IC.CASES, cus) == []
    assert ["/".join(IC.class_key(c, cus)) for c in IC.CASES] == [c.key for c in IC.CASES]


PARAMS = [(c, f) for c in IC.CASES for f in IC.FAMILIES]


@pytest.mark.parametrize("c,family", PARAMS, ids=[f"{c.name}-{f}" for c, f in PARAMS])
def test_igemm_case(c, family):
    d = IC.desc(c)
    cs = d["cout_store"]
    key = IC.class_key(c, cu_count())
    # the launch is the one the key names
    lib = L.load()
    q = IC.lib_desc(c, L)
    assert lib.dove_conv_kernel_name(C.byref(q)).decode() == IC.KERNEL_NAME[key[0]]
    assert int(lib.dove_conv_partial_launches(C.byref(q))) == IC.partial_launches(c, cu_count())
    gn_rows = int(lib.dove_conv_gn_partial_rows(C.byref(q)))
    assert gn_rows == IC.gn_partial_rows(d) and (not c.gn or gn_rows > 0)

    inp = IC.operands(c, family)
    rows = IC.sample_rows(c, cu_count())
    ref, mag, gterm = IC.reference64(c, inp, rows=rows, cus=cu_count())
    dev = device_operands(c, inp)
    buf, out = guarded_out(c, d)
    y = launch(c, d, dev, out)
    torch.cuda.synchronize()
    assert guards_intact(buf, d), f"{c.name}: a store outside [frames] x [0, cout_store)"
    stored = out[..., :cs]
    assert not bool(torch.isnan(stored).any()), f"{c.name}: {int(torch.isnan(stored).sum())} elements were never written"
    assert bool(torch.isfinite(stored).all())
    if c.gn:                                                        # the fused partial sums: the stored values, the image's pixels only
        assert y.gn_rows.shape == (gn_rows, 64) and bool(torch.isfinite(y.gn_rows).all())
        want_gn, mag_gn = IC.gn_partials64(c, stored.cpu())
        err_gn = (y.gn_rows.double().cpu() - want_gn).abs()
        print(f"{c.name}-{family}: gn partials use {float((err_gn / (IC.EPS24 * mag_gn).clamp_min(1e-300)).max()):.3f} of {IC.K_GN}")
        assert bool((err_gn <= IC.K_GN * IC.EPS24 * mag_gn).all()), f"{c.name}: gn_partial off by up to {float(err_gn.max()):.4g}"
    flat = stored.reshape(-1, cs)
    got = (flat if rows is None else flat[rows.cuda()]).double().cpu()
    err = (got - ref).abs()
    tol = IC.budget(c, ref, mag, gterm)
    print(f"{c.name}-{family}: k used {IC.k_of((err - 0.5 * IC.ulp_out(ref, c.out_f32)).clamp_min(0), mag, gterm):.3f} of {c.kk}")
    bad = err > tol
    if bool(bad.any()):
        i, j = bad.nonzero()[0].tolist()
        raise AssertionError(f"{c.name}-{family}: {int(bad.sum())}/{bad.numel()} elements over the budget; worst {float((err / tol).max()):.3g}x; "
                             f"first at row {i if rows is None else int(rows[i])} col {j}: got {float(got[i, j])!r} ref {float(ref[i, j])!r} "
                             f"mag {float(mag[i, j]):.4g}")
    want = bits(stored)

    if c.cin < d["cin"]:                                            # finite poison in the activation pad channels: the weight pad is zero
        dev2 = device_operands(c, inp, pad_poison=True)
        buf2, out2 = guarded_out(c, d)
        launch(c, d, dev2, out2)
        torch.cuda.synchronize()
        assert guards_intact(buf2, d) and torch.equal(bits(out2[..., :cs]), want), "the activation pad channels reach the output"
        del dev2, buf2, out2
    if c.gn:                                                        # the fused statistics do not change what is stored
        buf2, out2 = guarded_out(c, d)
        launch(c, d, dev, out2, gn=False)
        torch.cuda.synchronize()
        assert guards_intact(buf2, d) and torch.equal(bits(out2[..., :cs]), want), "gn_partial changes the output"
        del buf2, out2
    if c.inplace:                                                   # out is resid
        buf2, out2 = guarded_out(c, d, prefill=dev["resid"])
        launch(c, d, dev, out2, resid=out2)
        torch.cuda.synchronize()
        assert guards_intact(buf2, d) and torch.equal(bits(out2[..., :cs]), want), "in place differs from out of place"
        del buf2, out2
    if c.nb > 1:                                                    # nb instances in one launch = nb calls
        buf2, out2 = guarded_out(c, d)
        for b in range(c.nb):
            launch(c, d, dev, out2[b * d["t_out"]:(b + 1) * d["t_out"]], nb=1, sl=b)
        torch.cuda.synchronize()
        assert guards_intact(buf2, d) and torch.equal(bits(out2[..., :cs]), want), "nb instances differ from nb calls"
        del buf2, out2
    big = buf.numel() * buf.element_size() > (64 << 20)
    del dev, buf, out, y, stored, flat, want
    if big:
        torch.cuda.empty_cache()
