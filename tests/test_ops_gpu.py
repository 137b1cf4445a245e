"""-m gpu: every HIP operator, called through the C-ABI (dove_amd.ops -> ctypes -> libdove_hip.so), against
the torch restatement of the same operator (tests/emu_ops.py) on identical seeded inputs.
Tolerance (written here, floating point): both sides accumulate in fp32 from the same bf16 operands and round
the result to bf16 once, so they may differ by accumulation order + 1 bf16 ulp:
    |hip - ref| <= 1.6e-2*|ref| + 4e-3*max|ref|."""
import math

import pytest
import torch

import emu_ops as E
from dove_amd import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def close(name, got, ref, rtol=1.6e-2, afrac=4e-3, max_bad=0):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - ref).abs()
    tol = rtol * ref.abs() + afrac * ref.abs().max() + 1e-6
    bad = err > tol
    if int(bad.sum()) > max_bad:
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements off; max err {float(err.max()):.4g} "
                             f"(ref max {float(ref.abs().max()):.4g}); first bad idx {idx} got {float(got[tuple(idx)]):.5g} "
                             f"ref {float(ref[tuple(idx)]):.5g}")


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def pack(cout, cin, k, seed=1, bias=True):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, *k, generator=g) * (cin * math.prod(k)) ** -0.5
    b = torch.randn(cout, generator=g) * 0.1 if bias else None
    return E.pack_conv(w, b, "cpu"), ops.pack_conv(w, b, "cuda")


CONV_CASES = [
    # name, cin, cout, k, T, H, W, kwargs
    ("c3d_128_128", 128, 128, (3, 3, 3), 3, 20, 24, {}),
    ("c3d_128_128_cache", 128, 128, (3, 3, 3), 2, 9, 17, {"cache": True}),
    ("c3d_3_128", 3, 128, (3, 3, 3), 2, 16, 16, {}),
    ("c3d_128_256", 128, 256, (3, 3, 3), 2, 10, 12, {"cache": True}),
    ("c3d_512_32", 512, 32, (3, 3, 3), 3, 6, 10, {}),
    ("c3d_128_3", 128, 3, (3, 3, 3), 2, 16, 24, {"cache": True}),
    ("c3d_16_512", 16, 512, (3, 3, 3), 3, 5, 7, {}),
    ("c3d_64_64_T1", 64, 64, (3, 3, 3), 1, 8, 8, {}),
    ("c3d_96_64", 96, 64, (3, 3, 3), 2, 8, 8, {}),
    ("c111_128_256", 128, 256, (1, 1, 1), 3, 9, 11, {}),
    ("c111_16_1024", 16, 1024, (1, 1, 1), 3, 4, 6, {}),
    ("c111_M6144", 128, 256, (1, 1, 1), 2, 48, 64, {}),            # a plain GEMM that misses gemm8p's shape rules: igemm_fast
    # smallk_kernel: CogVideoXSpatialNorm3D's conv_y || conv_b on the 16-channel latent (Cin_pad 32), ragged last row block
    ("c111_smallk_spatialnorm", 16, 512, (1, 1, 1), 2, 45, 81, {}),
    ("c2d_down_even", 128, 128, (3, 3), 3, 16, 20, {"stride": 2, "pad": (0, 0)}),
    ("c2d_down_odd", 64, 64, (3, 3), 2, 15, 9, {"stride": 2, "pad": (0, 0)}),
    ("c2d_up", 128, 128, (3, 3), 3, 6, 9, {"up": 1, "pad": (1, 1)}),
    ("c2d_up_t1", 128, 128, (3, 3), 2, 6, 8, {"up": 1, "pad": (1, 1), "tmode": 1, "t_out": 4}),
    ("c2d_up_t2", 256, 256, (3, 3), 3, 5, 8, {"up": 1, "pad": (1, 1), "tmode": 2, "t_out": 5}),
    ("c3d_resid", 128, 128, (3, 3, 3), 2, 12, 16, {"resid": True}),
    # LDS-halo kernel: several 8x32 tiles, ragged borders, 2 channel chunks x 3 frame taps, 2 cout tiles
    ("c3d_halo_multi", 64, 256, (3, 3, 3), 3, 20, 70, {"cache": True}),
    ("c2d_halo_kt1", 128, 128, (3, 3), 2, 9, 40, {}),
    ("c3d_halo_resid", 128, 128, (3, 3, 3), 2, 17, 33, {"resid": True, "cache": True}),
    ("c3d_halo_cin3", 3, 128, (3, 3, 3), 4, 12, 48, {}),
    ("c3d_halo_512", 512, 512, (3, 3, 3), 2, 8, 32, {}),
    # 3 x 3 tiles of 16x32 with ragged edges, 2 cout tiles (the shapes that used to pin the 8-wave ping-pong kernel)
    ("c3d_tiles_ragged", 64, 256, (3, 3, 3), 2, 40, 70, {"cache": True, "resid": True}),
    ("c3d_512_128_T1", 512, 128, (3, 3, 3), 1, 16, 32, {}),
    # upsample-fused conv on the ping-pong halo kernel (UP variant): ragged tiles, both temporal maps
    ("c2d_up8", 128, 128, (3, 3), 2, 20, 40, {"up": 1, "pad": (1, 1)}),
    ("c2d_up8_t2", 64, 256, (3, 3), 3, 9, 17, {"up": 1, "pad": (1, 1), "tmode": 2, "t_out": 5}),
    ("c2d_up8_t1", 256, 128, (3, 3), 2, 16, 16, {"up": 1, "pad": (1, 1), "tmode": 1, "t_out": 4}),
    # persistent one-wave-per-SIMD kernel (conv3x3_halo4x): the shortest K walk it accepts (2 groups = 18 steps per tile,
    # so the staging streams cross a tile boundary every 18 steps) with more tiles than workgroups, and a kt = 1 conv
    ("c2d_halo4x_k64_many", 64, 128, (3, 3), 20, 64, 128, {}),
    ("c2d_halo4x_kt1_resid", 128, 256, (3, 3), 2, 24, 40, {"resid": True}),
    # Cin_pad == 32 convs with H, W >= 16 (direct encoder.conv_in 3 -> 128 of the tiled VAE, decoder.conv_in 16 -> 512): igemm_fast
    # SUB-PIXEL form of the upsample-fused conv (dove_conv_desc.w_sub; low-res grid >= 16 x 32): ragged low-res edges in both directions,
    # several tiles, two cout tiles per phase, Upsample3D's two time-doubling maps
    ("c2d_up_sub", 128, 128, (3, 3), 2, 17, 37, {"up": 1, "pad": (1, 1)}),
    ("c2d_up_sub_256", 256, 256, (3, 3), 2, 20, 70, {"up": 1, "pad": (1, 1)}),
    ("c2d_up_sub_t1", 128, 128, (3, 3), 2, 16, 32, {"up": 1, "pad": (1, 1), "tmode": 1, "t_out": 4}),
    ("c2d_up_sub_t2", 64, 256, (3, 3), 3, 18, 40, {"up": 1, "pad": (1, 1), "tmode": 2, "t_out": 5}),
    ("c3d_conv_in_enc", 3, 128, (3, 3, 3), 3, 40, 48, {"cache": True}),
    ("c3d_conv_in_dec", 16, 512, (3, 3, 3), 2, 18, 34, {}),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv(case):
    name, cin, cout, k, T, H, W, kw = case
    pc_c, pc_g = pack(cout, cin, k)
    x = torch.zeros(T, H, W, pc_c.cin_pad, dtype=BF)
    x[..., :cin] = rnd(T, H, W, cin, seed=2)
    kw = dict(kw)
    use_cache, use_resid = kw.pop("cache", False), kw.pop("resid", False)
    cache = resid = None
    if use_cache:
        cache = torch.zeros(k[0] - 1, H, W, pc_c.cin_pad, dtype=BF)
        cache[..., :cin] = rnd(cache.shape[0], H, W, cin, seed=3)
    if use_resid:
        resid = rnd(*E.conv(x, pc_c, cache=cache, **kw).shape, seed=4)
    ref = E.conv(x, pc_c, cache=cache, resid=resid, **kw)
    got = ops.conv(x.cuda(), pc_g, cache=None if cache is None else cache.cuda(),
                   resid=None if resid is None else resid.cuda(), **kw)
    torch.cuda.synchronize()
    close(name, got, ref)


LIN_CASES = [
    ("lin_3072_9216", 300, 3072, 9216, {}),
    ("lin_128_3072", 260, 128, 3072, {}),
    ("lin_4096_3072", 226, 4096, 3072, {}),
    ("lin_gelu", 200, 256, 1024, {"act": 1}),
    ("lin_3072_128", 333, 3072, 128, {}),
    ("lin_gate", 300, 1024, 256, {"gate": True}),
    ("lin_12288_3072_gate_inplace", 270, 12288, 3072, {"gate": True, "inplace": True}),
    ("lin_M1", 1, 256, 256, {}),
    ("lin_M129", 129, 256, 64, {}),
    # plain GEMMs with M >= 4096 that miss gemm8p's shape rules (were gemm8, now igemm_fast): ragged M tail, every K-loop tail length (nk = 1, 2, 3, 4, 96), epilogues
    ("lin8_basic", 4700, 3072, 256, {}),
    ("lin8_gelu", 4096, 256, 1024, {"act": 1}),
    ("lin8_gate_inplace", 5000, 1024, 128, {"gate": True, "inplace": True}),
    ("lin8_k32", 4100, 32, 128, {}),
    ("lin8_k64", 4100, 64, 256, {}),
    ("lin8_k96", 4200, 96, 128, {}),
    ("lin8_k128", 4608, 128, 3072, {}),
    # gemm8p persistent 256x256 kernel (M >= 4096, cout % 256 == 0, cin % 128 == 0): ragged M tail, one and many K chunks, GELU / gated
    # in-place residual epilogues.  Since gemm_tail_split, lin4x_many_tiles is 316 tiles = a 256-tile main launch (exactly ONE tile per
    # workgroup on 256 CUs) + an igemm_fast tail, and lin4x_many_tiles_gate is 237 tiles on 237 workgroups: neither switches tiles inside a
    # workgroup.  Of this list only lin4x_tail_dit_out does (864 tiles -> 768 in three rounds + tail); the walk classes (tiles per workgroup,
    # off-stream successors, supertile groups) are enumerated and pinned by tests/igemm_cases.py / tests/test_igemm_fp64_gpu.py
    ("lin4x_ragged", 4099, 256, 256, {}),
    ("lin4x_many_tiles", 20011, 256, 1024, {}),
    ("lin4x_many_tiles_gate", 20011, 384, 768, {"gate": True, "inplace": True}),
    # gemm8p + igemm_fast tail split (rows behind the last full round of 256 tiles): 316 tiles -> 16384 rows + 3627 rows; the
    # gate's row-class boundary before / inside the tail; GELU; the DiT's own N = 3072 shape (864 tiles -> 16384 + 1842 rows)
    ("lin4x_tail_gate", 20011, 256, 1024, {"gate": True, "inplace": True}),
    ("lin4x_tail_gate_late", 20011, 256, 1024, {"gate": True, "gate_split": 18000}),
    ("lin4x_tail_gelu", 20011, 128, 1024, {"act": 1}),
    ("lin4x_tail_dit_out", 18226, 256, 3072, {"gate": True, "gate_split": 226, "inplace": True}),
    ("lin4x_gelu_deep", 4500, 1536, 512, {"act": 1}),
    ("lin4x_resid", 4300, 512, 256, {"resid_only": True}),
]


@pytest.mark.parametrize("T,H,W,use_cache", [(3, 20, 37, True), (9, 18, 70, False)])
def test_conv_in_im2col(T, H, W, use_cache):
    """encoder.conv_in as a (3,1,1) conv on the im2col'ed input (dove_cl_im2col3x3_from_ncthw) against the direct 3x3x3 conv on the
    3-channel input: same products, fp32 sums in another order."""
    cin, co = 3, 128
    g = torch.Generator().manual_seed(41)
    w = torch.randn(co, cin, 3, 3, 3, generator=g) * (cin * 27) ** -0.5
    b = torch.randn(co, generator=g) * 0.1
    x = torch.randn(cin, T + 2, H, W, generator=g)                       # [C, frames, H, W]; the first two frames act as the cache
    xs = x[:, 2:] if use_cache else x[:, :T]
    xc = x[:, :2] if use_cache else None
    im = ops.cl_im2col3x3_from_ncthw(xs.cuda(), 32)
    assert torch.equal(im.cpu(), E.cl_im2col3x3_from_ncthw(xs, 32))
    w27 = w.permute(0, 3, 4, 1, 2).reshape(co, 27, 3, 1, 1)
    pt_g = ops.pack_conv(w27, b, "cuda")
    got = ops.conv(im, pt_g, cache=None if xc is None else ops.cl_im2col3x3_from_ncthw(xc.cuda(), 32))
    pc_c, pc_g = E.pack_conv(w, b, "cpu"), ops.pack_conv(w, b, "cuda")
    direct = ops.conv(ops.cl_from_ncthw(xs.cuda(), 32), pc_g, cache=None if xc is None else ops.cl_from_ncthw(xc.cuda(), 32))
    want = E.conv(E.cl_from_ncthw(xs, 32), pc_c, cache=None if xc is None else E.cl_from_ncthw(xc, 32))
    torch.cuda.synchronize()
    close("conv_in_im2col.vs_direct_hip", got, direct, rtol=8e-3, afrac=4e-3)
    close("conv_in_im2col.vs_emu", got, want)


@pytest.mark.parametrize("T,H,W,use_cache", [(3, 20, 37, True), (2, 9, 70, False), (1, 16, 16, False)])
def test_conv_out_tap_split(T, H, W, use_cache):
    """decoder.conv_out as a (3,1,1) conv with the 9 spatial taps as 27 fp32 output channels + dove_conv_out_gather: same result as
    the direct 3x3x3 conv followed by the layout kernel (fp32 sums in another order, one bf16 rounding each), incl. the frame border."""
    cin, co = 128, 3
    g = torch.Generator().manual_seed(31)
    w = torch.randn(co, cin, 3, 3, 3, generator=g) * (cin * 27) ** -0.5
    b = torch.randn(co, generator=g) * 0.1
    x = rnd(T, H, W, cin, seed=32)
    cache = rnd(2, H, W, cin, seed=33) if use_cache else None
    post = dict(scale=0.5, shift=0.5, lo=0.0, hi=1.0)
    pc_c, pc_g = E.pack_conv(w, b, "cpu"), ops.pack_conv(w, b, "cuda")
    want = E.ncthw_from_cl(E.conv(x, pc_c, cache=cache), co, torch.float32, **post)
    direct = ops.ncthw_from_cl(ops.conv(x.cuda(), pc_g, cache=None if cache is None else cache.cuda()), co, torch.float32, **post)
    w27 = w.permute(3, 4, 0, 1, 2).reshape(27, cin, 3, 1, 1)
    pt_c, pt_g = E.pack_conv(w27, None, "cpu"), ops.pack_conv(w27, None, "cuda")
    p = ops.conv(x.cuda(), pt_g, cache=None if cache is None else cache.cuda(), out_f32=True)
    assert p.dtype == torch.float32 and p.shape == (T, H, W, 28)
    got = ops.conv_out_gather(p, co, b.cuda(), torch.float32, **post)
    emu = E.conv_out_gather(E.conv(x, pt_c, cache=cache, out_f32=True), co, b, torch.float32, **post)
    torch.cuda.synchronize()
    close("conv_out_split.vs_direct_hip", got, direct, rtol=8e-3, afrac=4e-3)
    close("conv_out_split.vs_emu", got, emu, rtol=8e-3, afrac=4e-3)
    close("conv_out_split.vs_direct_emu", got, want, rtol=8e-3, afrac=4e-3)
    got_bf = ops.conv_out_gather(p, co, b.cuda(), BF)
    assert got_bf.dtype == BF and got_bf.shape == (co, T, H, W)


@pytest.mark.parametrize("case", LIN_CASES, ids=[c[0] for c in LIN_CASES])
def test_linear(case):
    name, N, cin, cout, kw = case
    pc_c, pc_g = pack(cout, cin, ())
    x = rnd(N, cin, seed=5)
    kw = dict(kw)
    gate = resid = None
    inplace = kw.pop("inplace", False)
    if kw.pop("resid_only", False):
        resid = rnd(N, cout, seed=7)
    if kw.pop("gate", False):
        g = torch.Generator().manual_seed(6)
        gate = torch.randn(2, pc_c.cout_pad, generator=g)
        resid = rnd(N, cout, seed=7)
        kw.setdefault("gate_split", N // 3)
    ref = E.linear(x, pc_c, resid=resid, gate=gate, **kw)
    rg = None if resid is None else resid.cuda()
    got = ops.linear(x.cuda(), pc_g, resid=rg, gate=None if gate is None else gate.cuda(), out=rg if inplace else None, **kw)
    torch.cuda.synchronize()
    close(name, got, ref)


@pytest.mark.parametrize("C,T,H,W", [(128, 3, 20, 24), (256, 2, 9, 13), (512, 3, 6, 5), (32, 2, 8, 8), (64, 1, 40, 40)])
def test_groupnorm_stats_apply(C, T, H, W):
    x = (rnd(T, H, W, C, seed=8).float() * 1.7 + 0.9).to(BF)
    g = torch.Generator().manual_seed(9)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    st_ref = E.groupnorm_stats(x, 1e-6)
    st = ops.groupnorm_stats(x.cuda(), 1e-6)
    torch.cuda.synchronize()
    assert torch.allclose(st.cpu(), st_ref, rtol=2e-4, atol=2e-5), (st.cpu() - st_ref).abs().max()
    ref = E.groupnorm_apply(x, st_ref, gamma, beta, silu=True)
    got = ops.groupnorm_apply(x.cuda(), st, gamma.cuda(), beta.cuda(), silu=True)
    torch.cuda.synchronize()
    close(f"gn_apply_{C}", got, ref)


@pytest.mark.parametrize("C,T,H,W", [(128, 5, 20, 24), (512, 3, 6, 5)])
def test_groupnorm_sums_pieces(C, T, H, W):
    """Distributed form: raw fp64 (sum, sumsq) of two pieces of a frame-batch, added, finalised == statistics of the batch."""
    x = (rnd(T, H, W, C, seed=8).float() * 1.3 - 0.4).to(BF).cuda()
    cut = T // 2 + 1
    sa, sb = ops.groupnorm_sums(x[:cut].contiguous()), ops.groupnorm_sums(x[cut:].contiguous())
    got = ops.groupnorm_from_sums(sa + sb, float(x.numel() // 32), 1e-6)
    ref = ops.groupnorm_stats(x, 1e-6)
    emu = E.groupnorm_from_sums(E.groupnorm_sums(x.cpu()), float(x.numel() // 32), 1e-6)
    torch.cuda.synchronize()
    assert torch.allclose(got.cpu(), ref.cpu(), rtol=2e-4, atol=2e-5)
    assert torch.allclose(got.cpu(), emu, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("C,Tf,Tz,hz,wz,sshift", [(128, 5, 3, 4, 6, 2), (512, 3, 3, 5, 4, 0), (256, 4, 2, 3, 5, 1), (128, 9, 3, 2, 3, 3)])
def test_spatial_norm_apply(C, Tf, Tz, hz, wz, sshift):
    from dove_amd.vae import spatial_norm_tmap
    H, W = hz << sshift, wz << sshift
    x = rnd(Tf, H, W, C, seed=10)
    yb = rnd(Tz, hz, wz, 2 * C, seed=11)
    g = torch.Generator().manual_seed(12)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    st = E.groupnorm_stats(x, 1e-6)
    tmap = spatial_norm_tmap(Tf, Tz)
    ref = E.groupnorm_apply(x, st, gamma, beta, silu=True, yb=yb, sshift=sshift, tmap=tmap)
    got = ops.groupnorm_apply(x.cuda(), st.cuda(), gamma.cuda(), beta.cuda(), silu=True, yb=yb.cuda(), sshift=sshift, tmap=tmap)
    torch.cuda.synchronize()
    close(f"sn_apply_{C}", got, ref)


@pytest.mark.parametrize("N,D,mod", [(300, 3072, True), (129, 256, True), (77, 3072, False), (5, 4096, True), (64, 512, False)])
def test_layernorm_modulate(N, D, mod):
    x = (rnd(N, D, seed=13).float() * 2 + 0.3).to(BF)
    g = torch.Generator().manual_seed(14)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    m = 0.3 * torch.randn(2, 2, D, generator=g) if mod else None
    ref = E.layernorm_modulate(x, gamma, beta, 1e-5, m, N // 4)
    got = ops.layernorm_modulate(x.cuda(), gamma.cuda(), beta.cuda(), 1e-5, None if m is None else m.cuda(), N // 4)
    torch.cuda.synchronize()
    close(f"ln_{N}_{D}", got, ref)


@pytest.mark.parametrize("N,heads,text_len", [(738, 48, 226), (300, 4, 226), (130, 2, 0), (64, 1, 10), (1000, 3, 226)])
def test_qkv_post_and_attention(N, heads, text_len):
    D = heads * 64
    npad = (N + 127) // 128 * 128
    qkv = rnd(N, 3 * D, seed=15)
    g = torch.Generator().manual_seed(16)
    gq, bq, gk, bk = (1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g),
                      1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g))
    ang = torch.rand(N - text_len, 32, generator=g) * 6.28
    cos, sin = ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous()
    qscale = 0.125 * math.log2(math.e)
    z = lambda *s: torch.zeros(*s, dtype=BF)   # noqa: E731
    Qr, Kr, Vr = z(heads, npad, 64), z(heads, npad, 64), z(heads, 64, npad)
    E.qkv_post(qkv, N, npad, heads, text_len, gq, bq, gk, bk, cos, sin, qscale, 1e-6, Qr, Kr, Vr)
    Qg, Kg, Vg = z(heads, npad, 64).cuda(), z(heads, npad, 64).cuda(), z(heads, 64, npad).cuda()
    n2 = torch.full((heads, 2), -1.0, device="cuda")             # stale contents: the call clears the array itself
    ops.qkv_post(qkv.cuda(), N, npad, heads, text_len, gq.cuda(), bq.cuda(), gk.cuda(), bk.cuda(), cos.cuda(), sin.cuda(),
                 qscale, 1e-6, Qg, Kg, Vg, norm2=n2)
    torch.cuda.synchronize()
    close("qkv_post.Q", Qg, Qr)
    close("qkv_post.K", Kg, Kr)
    close("qkv_post.Vt", Vg, Vr)
    # the score bound: max squared norms of the rows the kernel STORED (fp32 sums of bf16 squares; only the summation order differs)
    want = torch.stack([(Qg[:, :N].float() ** 2).sum(-1).amax(-1), (Kg[:, :N].float() ** 2).sum(-1).amax(-1)], dim=1)
    assert torch.allclose(n2, want, rtol=1e-5, atol=0), (n2, want)
    ref = E.attention(Qr, Kr, Vr, N, npad, heads, torch.zeros(N, D, dtype=BF))
    got = ops.attention(Qr.cuda(), Kr.cuda(), Vr.cuda(), N, npad, heads, torch.zeros(N, D, dtype=BF, device="cuda"))
    torch.cuda.synchronize()
    # P is rounded to bf16 before PV in the kernel (flash attention): allow 2 ulp
    close(f"attention_{N}_{heads}", got, ref, rtol=3e-2, afrac=8e-3)
    # the same product with the constant shift from the bound instead of the running maximum (what the DiT runs)
    nr = torch.stack([(Qr[:, :N].float() ** 2).sum(-1).amax(-1), (Kr[:, :N].float() ** 2).sum(-1).amax(-1)], dim=1).cuda().contiguous()
    assert float(1.01 * (nr[:, 0] * nr[:, 1]).sqrt().max()) < 80.0
    assert ops.attention_head_paths(None, heads) == ["attn_fwd_kernel"] * heads
    got2 = ops.attention(Qr.cuda(), Kr.cuda(), Vr.cuda(), N, npad, heads, torch.zeros(N, D, dtype=BF, device="cuda"), norm2=nr)
    torch.cuda.synchronize()
    assert ops.attention_head_paths(nr) == ["attn_pipe_kernel"] * heads      # what the DiT runs: the no-shift pipelined kernel
    close(f"attention_bound_{N}_{heads}", got2, ref, rtol=3e-2, afrac=8e-3)


@pytest.mark.parametrize("counts,hloc", [([37, 36, 40], 2), ([300], 3), ([1, 0, 130, 61], 1), ([2279, 2278, 2278, 2278, 2278, 2278, 2279, 2278], 6)])
def test_ulysses_place(counts, hloc):
    """dove_ulysses_place_bf16 (receive side of the sequence/head-parallel DiT's all-to-all): per-source-rank blocks -> the attention
    kernel's operands in one launch; bit-exact (a copy), V^T quad-swapped, pad columns zero whatever the buffers held before."""
    N = sum(counts)
    npad = (N + 127) // 128 * 128
    g = torch.Generator().manual_seed(31)
    rq, rk, rv = (torch.randn(N * hloc * 64, generator=g).to(BF) for _ in range(3))
    ref = [torch.zeros(hloc, npad, 64, dtype=BF), torch.zeros(hloc, npad, 64, dtype=BF), torch.zeros(hloc, 64, npad, dtype=BF)]
    E.ulysses_place(rq, rk, rv, counts, hloc, N, npad, *ref)
    got = [torch.zeros(hloc, npad, 64, dtype=BF, device="cuda"), torch.zeros(hloc, npad, 64, dtype=BF, device="cuda"),
           torch.full((hloc, 64, npad), 7.0, dtype=BF, device="cuda")]               # stale V^T contents must not survive in the pad
    ops.ulysses_place(rq.cuda(), rk.cuda(), rv.cuda(), counts, hloc, N, npad, *got)
    torch.cuda.synchronize()
    for name, a, b in zip(("Qh", "Kh", "Vt"), got, ref):
        assert torch.equal(a.cpu(), b), f"{name} differs"


def _mx_operands(N, heads, text_len, seed=15, spread=1.0):
    D = heads * 64
    npad = (N + 127) // 128 * 128
    qkv = (rnd(N, 3 * D, seed=seed).float() * spread).to(BF)
    g = torch.Generator().manual_seed(seed + 1)
    gq, bq, gk, bk = (1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g),
                      1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g))
    ang = torch.rand(N - text_len, 32, generator=g) * 6.28
    cos, sin = ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous()
    return npad, qkv, (gq, bq, gk, bk), cos, sin


def _mx_bufs(heads, npad, device="cpu"):
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=device)   # noqa: E731
    return z(heads, npad, 64), z(heads, npad, 64), z(heads, 64, npad), z(heads, npad // 64, 64, 2)


def _fp8(u8):
    return u8.cpu().view(torch.float8_e4m3fn).float()


@pytest.mark.parametrize("N,heads,text_len", [(738, 48, 226), (300, 4, 226), (130, 2, 0), (64, 1, 10), (1000, 3, 226)])
def test_qkv_post_mx_and_attention_mx(N, heads, text_len):
    """fp8 attention operands + kernel against the tile-by-tile restatement (tests/emu_ops.py), and the whole thing against the
    exact fp32 softmax attention of the bf16 operands (accuracy of the variant, stated)."""
    D = heads * 64
    npad, qkv, (gq, bq, gk, bk), cos, sin = _mx_operands(N, heads, text_len)
    qscale = 0.125 * math.log2(math.e)
    Qr, Kr, Vr, Sr = _mx_bufs(heads, npad)
    E.qkv_post_mx(qkv, N, npad, heads, text_len, gq, bq, gk, bk, cos, sin, qscale, 1e-6, Qr, Kr, Vr, Sr)
    Qg, Kg, Vg, Sg = _mx_bufs(heads, npad, "cuda")
    Qg.fill_(0x55), Kg.fill_(0x55), Vg.fill_(0x55), Sg.fill_(0x55)            # every padded row must be rewritten
    ops.qkv_post_mx(qkv.cuda(), N, npad, heads, text_len, gq.cuda(), bq.cuda(), gk.cuda(), bk.cuda(), cos.cuda(), sin.cuda(),
                    qscale, 1e-6, Qg, Kg, Vg, Sg)
    torch.cuda.synchronize()
    # V: bf16 inputs, power-of-two scales -> bit-exact
    assert torch.equal(Sg.cpu(), Sr), "V scales differ"
    assert torch.equal(Vg.cpu(), Vr), "V e4m3 bytes differ"
    # Q, K: fp32 LayerNorm sums in a different order -> a value on a rounding boundary may land one e4m3 step away
    for name, a, b in (("Q8", Qg, Qr), ("K8", Kg, Kr)):
        fa, fb = _fp8(a), _fp8(b)
        assert (a.cpu() != b).float().mean() < 2e-3, f"{name}: too many differing bytes"
        assert ((fa - fb).abs() <= 0.126 * fb.abs() + 2.0 ** -9).all(), f"{name}: off by more than one e4m3 step"
    ref = E.attention_mx(Qr, Kr, Vr, Sr, N, npad, heads, torch.zeros(N, D, dtype=BF))
    got = ops.attention_mx(Qr.cuda(), Kr.cuda(), Vr.cuda(), Sr.cuda(), N, npad, heads, torch.zeros(N, D, dtype=BF, device="cuda"))
    torch.cuda.synchronize()
    # a probability on an e4m3 rounding boundary (v_exp_f32 vs torch.exp2), or a tile max next to an integer (the MFMA adds
    # -m inside its fp32 accumulation, the restatement after it: ceil() flips and the tile is quantised one binade coarser),
    # moves outputs by an e4m3 step of the keys involved - the elementwise tolerance is an e4m3 step on small elements
    close(f"attention_mx_{N}_{heads}", got, ref, rtol=4e-2, afrac=2e-2, max_bad=max(2, got.numel() // 200000))
    # accuracy against the unquantised attention
    z = lambda *s: torch.zeros(*s, dtype=BF)   # noqa: E731
    Qb, Kb, Vb = z(heads, npad, 64), z(heads, npad, 64), z(heads, 64, npad)
    E.qkv_post(qkv, N, npad, heads, text_len, gq, bq, gk, bk, cos, sin, qscale, 1e-6, Qb, Kb, Vb)
    exact = E.attention(Qb, Kb, Vb, N, npad, heads, torch.zeros(N, D, dtype=BF)).float()
    rel = float((got.float().cpu() - exact).pow(2).mean().sqrt() / exact.pow(2).mean().sqrt())
    print(f"attention_mx N={N} heads={heads}: rel RMS error vs exact {rel:.4f}")
    assert rel < 6e-2, rel


def test_attention_mx_spike_and_flat_tail():
    """(1) late / early dominant keys exercise the rescale path; (2) one dominant key followed by 4000 keys at 2^-11 of it: the
    tail carries ~2x the mass of the spike and must survive the fp8 probabilities (per-tile block scale, not one scale against
    the running max)."""
    N, heads = 4160, 2
    npad = 4224
    g = torch.Generator().manual_seed(17)
    q = torch.randn(heads, N, 64, generator=g) * 0.3
    k = torch.randn(heads, N, 64, generator=g) * 0.3
    v = torch.randn(heads, 64, N, generator=g)
    k[:, 400] = q[:, 7] * 40
    k[:, 3] = q[:, 300] * 30
    # query 1000: key 0 scores +11 (log2) above a flat tail
    q[:, 1000] = 0
    q[:, 1000, 0] = 4.0
    k[:, :, 0] = 0
    k[:, 0, 0] = 11.0 / 4.0
    Q8, K8, V8, Vs = _mx_bufs(heads, npad)
    Q8[:, :N] = (q * 8).to(torch.float8_e4m3fn).view(torch.uint8)
    K8[:, :N] = k.to(torch.float8_e4m3fn).view(torch.uint8)
    vp = torch.zeros(heads * 64, npad)
    vp[:, :N] = v.reshape(heads * 64, N)
    vq, ve = E.mx_quant_ref(vp)
    V8.copy_(E.v8_store_order(vq.view(torch.uint8).reshape(heads, 64, npad)))    # the kernel's key order inside a 32-key block
    Vs.copy_(ve.reshape(heads, 64, npad // 64, 2).permute(0, 2, 1, 3))
    ref = E.attention_mx(Q8, K8, V8, Vs, N, npad, heads, torch.zeros(N, heads * 64, dtype=BF))
    got = ops.attention_mx(Q8.cuda(), K8.cuda(), V8.cuda(), Vs.cuda(), N, npad, heads, torch.zeros(N, heads * 64, dtype=BF, device="cuda"))
    torch.cuda.synchronize()
    close("attention_mx_spike", got, ref, rtol=4e-2, afrac=2e-2, max_bad=4)
    # exact softmax over the dequantised operands: the only difference left is the quantisation of P
    qd, kd = _fp8(Q8)[:, :N] * 0.125, _fp8(K8)[:, :N]
    vd = E.mx_dequant(vq, ve).reshape(heads, 64, npad)[:, :, :N]
    p = torch.softmax(torch.einsum("hqd,hkd->hqk", qd, kd) * math.log(2.0), dim=-1)
    exact = torch.einsum("hqk,hdk->hqd", p, vd).permute(1, 0, 2).reshape(N, heads * 64)
    assert float(p[0, 1000, 1:].sum()) > 0.5                                    # the tail really dominates query 1000
    close("attention_mx_spike_exactP", got, exact.to(BF), rtol=4e-2, afrac=1.5e-2)
    row = (got.float().cpu()[1000] - exact[1000]).abs().max() / exact[1000].abs().max()
    assert row < 0.05, float(row)


def test_attention_spiked_rows():
    """online-softmax rescale path: one key dominates late in the sequence (guide rule 26)."""
    N, heads = 520, 2
    npad = 640
    g = torch.Generator().manual_seed(17)
    Q = torch.zeros(heads, npad, 64, dtype=BF)
    K = torch.zeros(heads, npad, 64, dtype=BF)
    V = torch.zeros(heads, 64, npad, dtype=BF)
    Q[:, :N] = (torch.randn(heads, N, 64, generator=g) * 0.3).to(BF)
    K[:, :N] = (torch.randn(heads, N, 64, generator=g) * 0.3).to(BF)
    V[:, :, :N] = torch.randn(heads, 64, N, generator=g).to(BF)
    K[:, 400] = (Q[:, 7].float() * 40).to(BF)      # huge score for query 7 at key 400 (7th KV tile)
    K[:, 3] = (Q[:, 300].float() * 30).to(BF)      # and an early spike for query 300
    E.vt_quad_swap(V)                              # the attention contract: V^T rows in the quad-swapped key order
    ref = E.attention(Q, K, V, N, npad, heads, torch.zeros(N, heads * 64, dtype=BF))
    got = ops.attention(Q.cuda(), K.cuda(), V.cuda(), N, npad, heads, torch.zeros(N, heads * 64, dtype=BF, device="cuda"))
    torch.cuda.synchronize()
    close("attention_spike", got, ref, rtol=3e-2, afrac=8e-3)
    # with the score bound: the spike of query 7 is a score of ~230 - 2^230 overflows the un-shifted exponential, the row sum leaves the
    # pipelined kernel's window, the head marks itself and the SAME call recomputes it with the running maximum
    n2 = _norm2(Q, K, N).cuda()
    assert float(1.01 * (n2[:, 0] * n2[:, 1]).sqrt().min()) > 200.0
    got = ops.attention(Q.cuda(), K.cuda(), V.cuda(), N, npad, heads, torch.full((N, heads * 64), 7.0, dtype=BF, device="cuda"), norm2=n2)
    torch.cuda.synchronize()
    assert ops.attention_head_paths(n2) == ["attn_fwd_kernel"] * heads and bool(torch.isnan(n2[:, 0]).all())
    close("attention_spike_bound_fallback", got, ref, rtol=3e-2, afrac=8e-3)


def _norm2(Q, K, N):
    return torch.stack([(Q[:, :N].float() ** 2).sum(-1).amax(-1), (K[:, :N].float() ** 2).sum(-1).amax(-1)], dim=1).contiguous()


def test_attention_loose_bound():
    """Constant-shift softmax with a bound far above every real score: one long query row and one long key row that are orthogonal put
    the Cauchy-Schwarz bound at ~36 (in base-2 exponent units, just under the kernel's cutoff of 40) while the scores stay within +-3 -
    every probability is then ~2^-33 before the normalisation, which must not cost precision (fp32 range, bf16 keeps its 8 relative bits)."""
    N, heads = 700, 2
    npad = 768
    g = torch.Generator().manual_seed(23)
    Q = torch.zeros(heads, npad, 64, dtype=BF)
    K = torch.zeros(heads, npad, 64, dtype=BF)
    V = torch.zeros(heads, 64, npad, dtype=BF)
    q = torch.randn(heads, N, 64, generator=g) * 0.3
    k = torch.randn(heads, N, 64, generator=g) * 0.3
    q[:, 11] = 0
    q[:, 11, 0] = 6.0
    k[:, :, 0] = 0                                  # nothing answers the long query
    k[:, 500] = 0
    k[:, 500, 1] = 6.0
    q[:, :, 1] = 0                                  # and nothing asks for the long key
    Q[:, :N], K[:, :N] = q.to(BF), k.to(BF)
    V[:, :, :N] = torch.randn(heads, 64, N, generator=g).to(BF)
    E.vt_quad_swap(V)
    n2 = _norm2(Q, K, N).cuda()
    b = 1.01 * (n2[:, 0] * n2[:, 1]).sqrt()
    assert 33.0 < float(b.min()) and float(b.max()) < 40.0, b
    ref = E.attention(Q, K, V, N, npad, heads, torch.zeros(N, heads * 64, dtype=BF))
    got = ops.attention(Q.cuda(), K.cuda(), V.cuda(), N, npad, heads, torch.zeros(N, heads * 64, dtype=BF, device="cuda"), norm2=n2)
    torch.cuda.synchronize()
    assert ops.attention_head_paths(n2) == ["attn_pipe_kernel"] * heads
    close("attention_loose_bound", got, ref, rtol=3e-2, afrac=8e-3)


def test_attention_no_shift_window_edges():
    """The adversarial cases for the no-shift softmax of attn_pipe_kernel (one launch, five heads):
      0  EVERY key anti-aligned with EVERY query (q ~ +a e0, k ~ -a e0), bound just under 80: every score ~ -76, every probability ~ 2^-76
         before the normalisation, row sums ~ 2^-66 - inside the window, must normalise to the exact softmax ON the pipelined kernel;
      1  the same with scores ~ -96: row sums ~ 2^-86 < 2^-80 -> the head marks itself and is recomputed with the running maximum;
      2  every key ALIGNED at +106: row sums ~ 2^116 > 2^100 -> marked, recomputed;
      3  a bound of ~100 from one long query and one long key that are orthogonal to everything, real scores within +-3: the bound is far
         above 80 but the row sums are ordinary -> stays on the pipelined kernel (the fast path does not depend on the bound's size);
      4  as 0, handed over with a NaN bound -> the running maximum from the start.
    (round 5's form of this test pinned a static cutoff at b = 40.)"""
    N, heads = 1000, 5
    npad = 1024
    g = torch.Generator().manual_seed(29)
    Q = torch.zeros(heads, npad, 64, dtype=BF)
    K = torch.zeros(heads, npad, 64, dtype=BF)
    V = torch.zeros(heads, 64, npad, dtype=BF)
    q = torch.randn(heads, N, 64, generator=g) * 0.15
    k = torch.randn(heads, N, 64, generator=g) * 0.15
    for h, (a, sgn) in {0: (8.7, -1.0), 1: (9.8, -1.0), 2: (10.3, 1.0), 4: (8.7, -1.0)}.items():
        q[h, :, 0] = a
        k[h, :, 0] = sgn * a
    q[3], k[3] = q[3] * 2, k[3] * 2
    q[3, 11] = 0
    q[3, 11, 0] = 10.0
    k[3, :, 0] = 0
    k[3, 500] = 0
    k[3, 500, 1] = 10.0
    q[3, :, 1] = 0
    Q[:, :N], K[:, :N] = q.to(BF), k.to(BF)
    V[:, :, :N] = torch.randn(heads, 64, N, generator=g).to(BF)
    E.vt_quad_swap(V)
    n2 = _norm2(Q, K, N).cuda()
    n2[4, 1] = float("nan")
    b = 1.01 * (n2[:, 0] * n2[:, 1]).sqrt()
    assert 74.0 < float(b[0]) < 80.0 < float(b[1]) and 95.0 < float(b[3]), b
    ref = E.attention(Q, K, V, N, npad, heads, torch.zeros(N, heads * 64, dtype=BF))
    got = ops.attention(Q.cuda(), K.cuda(), V.cuda(), N, npad, heads, torch.full((N, heads * 64), 7.0, dtype=BF, device="cuda"), norm2=n2)
    torch.cuda.synchronize()
    assert ops.attention_head_paths(n2) == ["attn_pipe_kernel", "attn_fwd_kernel", "attn_fwd_kernel", "attn_pipe_kernel", "attn_fwd_kernel"], n2
    assert bool(torch.isfinite(got).all())
    close("attention_window_edges", got, ref, rtol=3e-2, afrac=8e-3)
    # a second call with the array the first one marked: the marked heads go straight to the running maximum, same result
    got2 = ops.attention(Q.cuda(), K.cuda(), V.cuda(), N, npad, heads, torch.full((N, heads * 64), 7.0, dtype=BF, device="cuda"), norm2=n2)
    torch.cuda.synchronize()
    assert torch.equal(got, got2)


def test_conv_subpixel_is_the_kernel_and_matches_direct_form():
    """The production upsample shapes dispatch to the sub-pixel variant when the phase-summed weights are handed over; its result equals the
    direct form (upsample folded into the addressing, 9 taps) up to the one bf16 rounding of the summed weights; the fused GroupNorm
    statistics (a partial row per tile, phase and wave) equal a statistics pass over the output; nb instances == nb calls, bit for bit."""
    pc_c, pc_g = pack(256, 256, (3, 3))
    assert pc_g.w_sub is not None and pc_g.w_sub.shape == (4, 4, 256, 256)
    x = rnd(2, 36, 54, 256, seed=5).cuda()
    kw = dict(up=1, pad=(1, 1), tmode=1, t_out=4)
    y = ops.conv(x, pc_g, gn_eps=1e-6, **kw)
    assert y.gn_rows.shape[0] == 4 * 3 * 2 * 16, y.gn_rows.shape     # frames x (3 x 2 low-res tiles) x 4 phases x 4 waves
    ref_stats = ops.groupnorm_stats(y, 1e-6)
    assert torch.allclose(y.gn_stats[0].cpu(), ref_stats.cpu(), rtol=2e-4, atol=2e-5)
    w_sub, pc_g.w_sub = pc_g.w_sub, None                          # the direct form: the same conv without the summed weights
    direct = ops.conv(x, pc_g, **kw)
    pc_g.w_sub = w_sub
    torch.cuda.synchronize()
    close("subpixel_vs_direct", y, direct, rtol=1.6e-2, afrac=4e-3)
    assert not torch.equal(y, direct)                              # (it IS another kernel and another rounding of the weights)
    xb = torch.cat([x, rnd(2, 36, 54, 256, seed=6).cuda()])
    yb = ops.conv(xb, pc_g, nb=2, gn_eps=1e-6, **kw)
    y2 = ops.conv(xb[2:].contiguous(), pc_g, gn_eps=1e-6, **kw)
    torch.cuda.synchronize()
    assert torch.equal(yb[:4], y) and torch.equal(yb[4:], y2)
    assert torch.equal(yb.gn_stats[0][0], y.gn_stats[0]) and torch.equal(yb.gn_stats[0][1], y2.gn_stats[0])


@pytest.mark.parametrize("cin,cout,k,T,H,W,up,resid", [
    (128, 128, (3, 3, 3), 3, 37, 70, 0, False),      # 4 channels / group, ragged edge tiles
    (64, 256, (3, 3, 3), 2, 40, 64, 0, True),        # 8 channels / group, two cout tiles, residual epilogue
    (128, 512, (3, 3, 3), 1, 16, 33, 0, False),      # 16 channels / group, four cout tiles
    (256, 256, (3, 3), 2, 9, 20, 1, False),          # upsample-fused conv (output 18 x 40)
    (128, 128, (3, 3, 3), 9, 48, 96, 0, True),       # more tiles than one per workgroup row
])
def test_conv_fused_gn_stats(cin, cout, k, T, H, W, up, resid):
    """GroupNorm(32) statistics fused into the conv3x3_halo4x epilogue == a separate statistics pass over its bf16 output
    (same tolerance as test_groupnorm_stats_apply: fp32 partials, fp64 combine on both sides)."""
    pc_c, pc_g = pack(cout, cin, k)
    x = rnd(T, H, W, cin, seed=2)
    kw = {}
    if len(k) == 3:
        kw["cache"] = rnd(2, H, W, cin, seed=3).cuda()
    if up:
        kw.update(up=1, pad=(1, 1))
    if resid:
        kw["resid"] = rnd(T, H << up, W << up, cout, seed=4).cuda()
    y = ops.conv(x.cuda(), pc_g, gn_eps=1e-6, **kw)
    fused = getattr(y, "gn_stats", None)
    assert fused is not None, "this shape should dispatch to conv3x3_halo4x and fuse the statistics"
    ref = ops.groupnorm_stats(y, 1e-6)
    plain = ops.conv(x.cuda(), pc_g, **kw)
    torch.cuda.synchronize()
    assert torch.equal(plain, y), "requesting the statistics must not change the conv output"
    assert torch.allclose(fused[0].cpu(), ref.cpu(), rtol=2e-4, atol=2e-5), (fused[0].cpu() - ref.cpu()).abs().max()
    assert torch.equal(ops.groupnorm_stats_of(y, 1e-6), fused[0])
    s_rows, s_pass = ops.groupnorm_sums_of(y), ops.groupnorm_sums(y)      # raw sums for the distributed pair combine
    torch.cuda.synchronize()
    assert torch.allclose(s_rows.cpu(), s_pass.cpu(), rtol=2e-5, atol=1e-2), (s_rows.cpu() - s_pass.cpu()).abs().max()
    assert getattr(ops.conv(x.cuda(), pc_g, out=y, **kw), "gn_stats", None) is None    # re-used output drops stale stats


@pytest.mark.parametrize("cin,cout,k,nb,T,H,W,cache,resid,mask,emu", [
    (128, 128, (3, 3), 1, 16, 512, 40, False, True, 1, True),        # last tile column (W % 32 = 8) in 32 x 16 tiles: 4 -> 3 rounds
    (64, 256, (3, 3, 3), 1, 8, 500, 45, True, False, 1, True),       # ragged height too (500 = 15 x 32 + 20: the last 32 x 16 tile is cut), W % 32 = 13
    (128, 128, (3, 3, 3), 12, 8, 240, 360, True, True, 1, False),    # THE case it was built for: 12 tiles of 240 x 360, 8 frames (tiled VAE, level 0)
    (256, 128, (3, 3, 3), 12, 8, 240, 360, False, False, 1, False),  # ... its 256 -> 128 conv on a first frame-batch (w_first groups)
    (128, 128, (3, 3, 3), 1, 3, 24, 40, True, True, 0, True),        # small calls keep the one launch (a launch costs whole rounds)
])
def test_conv_partial_tiles_bit_identical_to_full_tiles(cin, cout, k, nb, T, H, W, cache, resid, mask, emu):
    """conv3x3_halo4x's PARTIAL-tile launch (the last 16 x 32 tile column walked in 32 x 16 tiles when the image ends within the first half of
    it and the two launches need fewer rounds of the persistent grid: dove_conv_partial_launches, asserted) against the SAME conv on full
    tiles only: the image embedded, top-left, in a zero frame whose size is a multiple of 16 x 32 -
    the zeros are the conv's own zero padding and add exact zeros, so the cropped result must be bit-identical; the fused GroupNorm
    PARTIAL SUMS of the two-launch form are bit-identical to the one-launch form's too (every (tile, wave slot) row sums the same pixels in
    the same order: checked against the same call with the plan's gate closed by splitting the instances), and == a separate pass."""
    pc_c, pc_g = pack(cout, cin, k)
    Hp, Wp = -(-H // 16) * 16, -(-W // 32) * 32
    assert ops.conv_kernel_name((T, H, W, cin), pc_g, resid=resid, nb=nb) == "conv3x3_halo4x_kernel"
    assert ops.conv_kernel_name((T, H, W, cin), pc_g, resid=resid, nb=nb, partial=True) == mask
    assert ops.conv_kernel_name((T, Hp, Wp, cin), pc_g, resid=resid, nb=nb, partial=True) == 0
    g = torch.Generator(device="cuda").manual_seed(71)
    x = torch.randn(nb * T, H, W, cin, device="cuda", generator=g).to(BF)
    xp = torch.zeros(nb * T, Hp, Wp, cin, dtype=BF, device="cuda")
    xp[:, :H, :W] = x
    kw, kwp = {}, {}
    if cache and len(k) == 3:
        c = torch.randn(*((nb, 2) if nb > 1 else (2,)), H, W, cin, device="cuda", generator=g).to(BF)
        cp = torch.zeros(*c.shape[:-3], Hp, Wp, cin, dtype=BF, device="cuda")
        cp[..., :H, :W, :] = c
        kw["cache"], kwp["cache"] = c, cp
    if resid:
        r = torch.randn(nb * T, H, W, cout, device="cuda", generator=g).to(BF)
        rp = torch.zeros(nb * T, Hp, Wp, cout, dtype=BF, device="cuda")
        rp[:, :H, :W] = r
        kw["resid"], kwp["resid"] = r, rp
    y = ops.conv(x, pc_g, gn_eps=1e-6, nb=nb, **kw)
    yp = ops.conv(xp, pc_g, nb=nb, **kwp)
    torch.cuda.synchronize()
    ycrop = yp[:, :H, :W]
    assert torch.equal(y, ycrop), float((y.float() - ycrop.float()).abs().max())
    del xp, yp, ycrop, kwp
    if emu:
        close("partial_tiles_vs_emu", y, E.conv(x.cpu(), pc_c, cache=kw["cache"].cpu() if "cache" in kw else None, resid=kw["resid"].cpu() if resid else None))
    fused = getattr(y, "gn_stats", None)
    assert fused is not None
    ref = ops.groupnorm_stats(y, 1e-6, nb) if nb > 1 else ops.groupnorm_stats(y, 1e-6)
    torch.cuda.synchronize()
    assert torch.allclose(fused[0].cpu(), ref.cpu(), rtol=2e-4, atol=2e-5), (fused[0].cpu() - ref.cpu()).abs().max()
    if nb > 1 and mask:
        # one instance at a time the gate stays closed (one launch): same output bits AND the same statistics bits per instance
        assert ops.conv_kernel_name((T, H, W, cin), pc_g, resid=resid, nb=1, partial=True) == 0
        for b in (0, nb - 1):
            kb = {k_: (v[b] if k_ == "cache" else v[b * T:(b + 1) * T]) for k_, v in kw.items()}
            yb = ops.conv(x[b * T:(b + 1) * T], pc_g, gn_eps=1e-6, **kb)
            torch.cuda.synchronize()
            assert torch.equal(yb, y[b * T:(b + 1) * T])
            assert torch.equal(yb.gn_stats[0].view(-1), fused[0][b].view(-1)), "fused GroupNorm statistics differ between the one- and two-launch forms"


def test_conv_and_linear_fullsize_properties():
    """Headline shapes (128->128 3x3x3 conv on 8x720x1280; 18 226 x 3072 -> 9216 linear): determinism, exact
    power-of-two homogeneity (op(2x) == 2 op(x) without bias: every product and partial sum scales exactly), temporal
    causality of the conv (frames 0..3 of the output do not change when frames 4..7 of the input do)."""
    g = torch.Generator(device="cuda").manual_seed(11)
    pc = ops.pack_conv(torch.randn(128, 128, 3, 3, 3) * (128 * 27) ** -0.5, None, "cuda")
    x = torch.randn(8, 720, 1280, 128, device="cuda", generator=g).to(BF)
    y = ops.conv(x, pc)
    assert torch.equal(y, ops.conv(x, pc)), "conv is not deterministic"
    assert torch.equal(ops.conv((x.float() * 2).to(BF), pc), (y.float() * 2).to(BF))
    x2 = x.clone()
    x2[4:] = torch.randn(4, 720, 1280, 128, device="cuda", generator=g).to(BF)
    assert torch.equal(ops.conv(x2, pc)[:4], y[:4]), "causal conv: early frames depend on later ones"
    del x2, y
    pl = ops.pack_conv(torch.randn(9216, 3072) * 3072 ** -0.5, None, "cuda")
    t = torch.randn(18226, 3072, device="cuda", generator=g).to(BF)
    z = ops.linear(t, pl)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(z.float()).all())
    assert torch.equal(z, ops.linear(t, pl)), "linear is not deterministic"
    assert torch.equal(ops.linear((t.float() * 2).to(BF), pl), (z.float() * 2).to(BF))
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_bound", [False, True], ids=["running_max", "norm2_pipe"])
def test_attention_fullsize_properties(with_bound):
    """N = 18 226 tokens x 48 heads (the headline clip), on the running-maximum kernel (no bound) and on the production path (norm2 ->
    attn_pipe_kernel, asserted): properties that need no reference at that size.
    (i) rows of softmax sum to one: V = 1 must give 1 (P is rounded to bf16 before PV while the normaliser is fp32: 2^-7);
    (ii) exact linearity in V for power-of-two scales: attention(Q, K, 2V) == 2 * attention(Q, K, V) bit for bit;
    (iii) keys in the zero-padded tail (columns N..Npad) never contribute: poisoning them changes nothing."""
    N, heads = 18226, 48
    npad = (N + 127) // 128 * 128
    g = torch.Generator(device="cuda").manual_seed(3)
    Qh = torch.zeros(heads, npad, 64, dtype=BF, device="cuda")
    Kh = torch.zeros(heads, npad, 64, dtype=BF, device="cuda")
    Vt = torch.zeros(heads, 64, npad, dtype=BF, device="cuda")
    Qh[:, :N] = (torch.randn(heads, N, 64, device="cuda", generator=g) * 0.5).to(BF)
    Kh[:, :N] = torch.randn(heads, N, 64, device="cuda", generator=g).to(BF)
    Vt[:, :, :N] = torch.randn(heads, 64, N, device="cuda", generator=g).to(BF)
    out = lambda: torch.zeros(N, heads * 64, dtype=BF, device="cuda")   # noqa: E731
    ones = torch.zeros_like(Vt)
    ones[:, :, :N] = 1.0
    ops.vt_quad_swap(ones)                         # natural -> the quad-swapped key order the kernel reads
    ops.vt_quad_swap(Vt)
    n2 = _norm2(Qh, Kh, N) if with_bound else None
    want_path = ["attn_pipe_kernel" if with_bound else "attn_fwd_kernel"] * heads

    def attn(K_, V_):
        r = ops.attention(Qh, K_, V_, N, npad, heads, out(), norm2=n2)
        torch.cuda.synchronize()
        assert ops.attention_head_paths(n2, heads) == want_path
        return r
    o1 = attn(Kh, ones)
    assert float((o1.float() - 1.0).abs().max()) <= 2 ** -7
    a = attn(Kh, Vt)
    b = attn(Kh, (Vt.float() * 2).to(BF))
    assert torch.equal((a.float() * 2).to(BF), b)
    Kp, Vp = Kh.clone(), ops.vt_quad_swap(Vt.clone())          # Vp back in natural order
    Kp[:, N:] = 7.0
    Vp[:, :, N:] = 1e4                                          # poison every key >= N ...
    ops.vt_quad_swap(Vp)                                        # ... wherever the swapped order puts it
    c = attn(Kp, Vp)                                            # (n2 still describes the real rows: the poisoned pad rows are masked, not scored)
    assert torch.equal(a, c)


def test_layout_and_glue():
    x = torch.randn(3, 4, 10, 12, generator=torch.Generator().manual_seed(18))
    for xx in (x, x.to(BF)):
        close("cl_from_ncthw", ops.cl_from_ncthw(xx.cuda(), 32, 0.5, 0.25), E.cl_from_ncthw(xx, 32, 0.5, 0.25))
    cl = rnd(4, 10, 12, 4, seed=19)
    for dt in (torch.float32, BF):
        close("ncthw_from_cl", ops.ncthw_from_cl(cl.cuda(), 3, dt, 0.5, 0.5, 0.0, 1.0), E.ncthw_from_cl(cl, 3, dt, 0.5, 0.5, 0.0, 1.0))
    cl32 = rnd(3, 5, 6, 32, seed=20)
    close("ncthw_from_cl32", ops.ncthw_from_cl(cl32.cuda(), 32, BF), E.ncthw_from_cl(cl32, 32, BF))
    for T in (2, 5, 8, 9):
        v = rnd(T, 6, 5, 64, seed=21)
        close(f"avgpool_{T}", ops.avgpool_time(v.cuda()), E.avgpool_time(v))
    mom = rnd(3, 5, 6, 32, seed=22)
    noise = torch.randn(16, 3, 5, 6, generator=torch.Generator().manual_seed(23))
    close("posterior", ops.posterior_sample(mom.cuda(), 16, noise.cuda(), BF), E.posterior_sample(mom, 16, noise, BF))
    a, b = rnd(1000, seed=24), rnd(1000, seed=25)
    close("axpby", ops.axpby(a.cuda(), b.cuda(), 0.625, -0.78125), E.axpby(a, b, 0.625, -0.78125))
    h = rnd(4, 16, 6, 10, seed=26)
    tok_ref = E.patchify(h, 2, 2, 128)
    tok = ops.patchify(h.cuda(), 2, 2, 128)
    close("patchify", tok, tok_ref)
    close("unpatchify", ops.unpatchify(tok, 4, 16, 6, 10, 2, 2, BF), E.unpatchify(tok_ref, 4, 16, 6, 10, 2, 2, BF))
    Wm = rnd(700, 512, seed=27, scale=0.05)
    bias = torch.randn(700, generator=torch.Generator().manual_seed(28))
    xv = torch.randn(512, generator=torch.Generator().manual_seed(29))
    for act in (0, 1):
        got = ops.gemv(Wm.cuda(), bias.cuda(), xv.cuda(), act)
        ref = E.gemv(Wm, bias, xv, act)
        assert torch.allclose(got.cpu(), ref, rtol=1e-4, atol=1e-4), (got.cpu() - ref).abs().max()
    torch.cuda.synchronize()


def test_tile_gather_and_im2col_tile_borders():
    """dove_tile_gather_bf16 (ABI 15): same-shaped tiles of a channels-last clip as one tile-major batch, bit for bit; on an im2col'ed clip the
    batch equals the im2col of the CROPPED tiles (zero padding at each tile's own border: what diffusers' tiled_encode hands conv_in;
    /root/reference/inference_script.py:642-645), for interior tiles and tiles that touch the clip border alike."""
    x = torch.randn(3, 7, 40, 56, generator=torch.Generator().manual_seed(61)).clamp(-1, 1).to(BF)
    cl = ops.cl_from_ncthw(x.cuda(), 32)
    origins = [(0, 0), (8, 24), (16, 32), (3, 5)]
    got = ops.tile_gather(cl, 2, 4, 24, 24, origins)
    ref = E.tile_gather(cl.cpu(), 2, 4, 24, 24, origins)
    assert got.shape == (16, 24, 24, 32) and torch.equal(got.cpu(), ref)
    im = ops.cl_im2col3x3_from_ncthw(x.cuda(), 32)
    got = ops.tile_gather(im, 2, 4, 24, 24, origins, im2col_cin=3)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), E.tile_gather(im.cpu(), 2, 4, 24, 24, origins, im2col_cin=3))
    want = torch.cat([E.cl_im2col3x3_from_ncthw(x[:, 2:6, oy:oy + 24, ox:ox + 24], 32) for oy, ox in origins], dim=0)
    assert torch.equal(got.cpu(), want)
    with pytest.raises(RuntimeError, match="leaves the"):
        ops.tile_gather(cl, 0, 2, 24, 24, [(20, 0)])


def test_conv_out_gather_channels_last():
    """dove_conv_out_gather_cl (ABI 15): the tap-split conv_out's 9-tap shifted sum for a spatial tile batch, channels-last bf16 with zeroed
    pad channels, equal to the NCTHW gather's values (the conv's own bf16 output rounding, no range map)."""
    for (T, H, W) in ((3, 9, 70), (2, 17, 64)):
        p = torch.randn(T, H, W, 32, generator=torch.Generator().manual_seed(62))
        bias = torch.randn(3, generator=torch.Generator().manual_seed(63))
        got = ops.conv_out_gather_cl(p.cuda(), 3, bias.cuda(), 8)
        ref_nc = ops.conv_out_gather(p.cuda(), 3, bias.cuda(), BF)
        torch.cuda.synchronize()
        assert got.shape == (T, H, W, 8) and bool((got[..., 3:] == 0).all())
        assert torch.equal(got[..., :3].permute(3, 0, 1, 2).contiguous(), ref_nc)
        close("conv_out_gather_cl", got, E.conv_out_gather_cl(p, 3, bias, 8))


@pytest.mark.parametrize("ld,axis", [(32, 0), (32, 1), (4, 0), (4, 1)])
def test_blend_edge(ld, axis):
    a, b = rnd(3, 9, 11, ld, seed=30), rnd(3, 9, 11, ld, seed=31)
    for extent in (0, 1, 5, 9):
        ref = E.blend_edge(a.clone(), b.clone(), extent, axis)
        got = ops.blend_edge(a.cuda(), b.clone().cuda(), extent, axis)
        torch.cuda.synchronize()
        close(f"blend_{ld}_{axis}_{extent}", got, ref)


@pytest.mark.parametrize("F,H,W,up", [(8, 45, 80, 4), (9, 48, 64, 4), (3, 30, 50, 1), (5, 20, 24, 2)])
def test_pre_post_processing(F, H, W, up):
    from dove_amd import tiling
    g = torch.Generator().manual_seed(40)
    frames = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8)
    pf, ph, pw = tiling.match_padding(F, H, W)
    for dt in (torch.float32, BF):
        ref = E.preprocess_u8(frames, pf, ph, pw, up, dt)
        got = ops.preprocess_u8(frames.cuda(), pf, ph, pw, up, dt)
        torch.cuda.synchronize()
        assert got.shape == ref.shape == (3, F + pf, (H + ph) * up, (W + pw) * up)
        tol = 2e-5 if dt == torch.float32 else 8e-3
        assert float((got.float().cpu() - ref.float()).abs().max()) <= tol
    vid = torch.rand(3, F + pf, (H + ph) * up, (W + pw) * up, generator=g) * 1.2 - 0.1
    Fo, Ho, Wo = F, H * up, W * up
    ref = E.postprocess_u8(vid, Fo, Ho, Wo)
    got = ops.postprocess_u8(vid.cuda(), Fo, Ho, Wo).cpu()
    assert torch.equal(got, ref)                       # uint8: bit-exact


def test_invalid_arguments_raise():
    pc_c, pc_g = pack(64, 64, (3, 3, 3))
    with pytest.raises(RuntimeError, match="channels"):
        ops.conv(torch.zeros(1, 4, 4, 32, dtype=BF, device="cuda"), pc_g)
    with pytest.raises(RuntimeError, match="power of two"):
        ops.groupnorm_stats(torch.zeros(1, 4, 4, 96, dtype=BF, device="cuda"), 1e-6)


# ---- MXFP8 linears (BASELINE configs[4]) -------------------------------------------------------------------------------------
def test_mx_quant_bit_exact():
    """dove_mx_quant_bf16 vs the torch restatement (float8_e4m3fn cast, power-of-two block scales): identical bytes and
    identical E8M0 exponents, incl. all-zero blocks, a block of subnormal-range values, huge and tiny magnitudes."""
    g = torch.Generator().manual_seed(41)
    x = torch.randn(300, 512, generator=g) * torch.exp(torch.randn(300, 1, generator=g) * 3)
    x[5, 32:64] = 0.0
    x[6, :32] = 448.0 * 4
    x[7, 64:96] *= 1e-6
    x[8, 96:128] = torch.tensor([2.0 ** k for k in range(-20, 12)])
    x = x.to(BF)
    pm = ops.mx_quant(x.cuda())
    torch.cuda.synchronize()
    q_ref, e_ref = E.mx_quant_ref(x)
    assert torch.equal(pm.s.cpu(), E.mx_scale_words(e_ref)), "E8M0 scales differ"
    assert torch.equal(pm.q.cpu(), q_ref.view(torch.uint8)), "e4m3 bytes differ"


@pytest.mark.parametrize("M,N,K,act,resid,gate", [
    (300, 256, 512, 0, False, False),           # one ragged row tile, two scale chunks
    (1000, 768, 1024, 1, False, False),         # GELU epilogue, 12 tiles: one per workgroup (the hand-over classes: tests/mx_cases.py)
    (700, 512, 3072, 0, True, True),            # gated residual (attn1.to_out.0 / ff.net.2 epilogue), DiT K
    (513, 256, 12288, 0, True, False),          # deep K (ff.net.2), plain residual
])
def test_linear_mxfp8(M, N, K, act, resid, gate):
    """HIP MXFP8 GEMM (block scales applied inside v_mfma_scale_f32_32x32x64_f8f6f4) vs dequantise-then-fp32-matmul of the
    SAME quantised operands.  Only the accumulation order differs: tolerance as for the bf16 linears."""
    g = torch.Generator().manual_seed(43)
    x = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(1, K, generator=g))).to(BF)      # per-channel spread: scales matter
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.1
    r = torch.randn(M, N, generator=g).to(BF) if resid else None
    gt = torch.randn(2, N, generator=g) if gate else None
    split = 226 if gate else 0
    ref = E.linear_mx_ref(x, w, b, resid=r, gate=gt, gate_split=split, act=act)
    pw = ops.pack_linear_mx(w, b, "cuda")
    got = ops.linear_mx(ops.mx_quant(x.cuda()), pw, resid=None if r is None else r.cuda(), gate=None if gt is None else gt.cuda(),
                        gate_split=split, act=act)
    torch.cuda.synchronize()
    close(f"linear_mxfp8_{M}x{N}x{K}", got, ref)
    # and the quantisation itself costs what MXFP8 should cost against the bf16 linear: a few 1e-2 relative RMS
    full = (x.float() @ w.to(BF).float().t() + b)
    if act == 0 and not resid:
        rel = float((got.float().cpu() - full).pow(2).mean().sqrt() / full.pow(2).mean().sqrt())
        print(f"[mxfp8 {M}x{N}x{K}] rms-rel vs the unquantised product {rel:.3e}")
        assert rel < 6e-2


# ------------------------------------------------------------------------------------------------------------------------
# Production shapes (BASELINE configs[1]: 33x720x1280) against torch-CPU fp32 on SAMPLED outputs.  The property tests above
# (determinism, homogeneity, causality) cannot see a deterministic, homogeneous indexing bug that only appears with > 256
# persistent tiles, 720-row frames or N = 18 226; these compare real values at the positions such a bug would hit: image
# borders, tile seams, the first / last persistent round, the rows either side of the GEMM tail split.
# Reference ops: the CogVideoXCausalConv3d / Upsample3D / Linear / SDPA calls behind /root/reference/inference_script.py:408,
# 483-489, 500.  The reference value is computed here with plain F.conv3d / F.conv2d / matmul / softmax (not tests/emu_ops.py).
# ------------------------------------------------------------------------------------------------------------------------
def _bands(H, picks):
    """[(r0, r1)] inclusive row bands around the picked rows (2 rows each), clipped to the image."""
    return [(max(0, r), min(H - 1, r + 1)) for r in picks]


def test_prodshape_conv3d_128_cache_resid_sampled():
    """128 -> 128 3x3x3 causal conv on one 8 x 720 x 1280 frame-batch with a 2-frame conv cache and the residual epilogue (the
    second conv of an encoder L0 / decoder L3 resnet: 36 of the clip's 268 halo4x launches have exactly this shape)."""
    import torch.nn.functional as F
    T, H, W, Cc = 8, 720, 1280, 128
    g = torch.Generator(device="cuda").manual_seed(101)
    gw = torch.Generator().manual_seed(102)
    w = (torch.randn(Cc, Cc, 3, 3, 3, generator=gw) * (Cc * 27) ** -0.5).to(BF).float()
    b = torch.randn(Cc, generator=gw) * 0.1
    pc = ops.pack_conv(w, b, "cuda")
    x = torch.randn(T, H, W, Cc, device="cuda", generator=g).to(BF)
    cache = torch.randn(2, H, W, Cc, device="cuda", generator=g).to(BF)
    resid = torch.randn(T, H, W, Cc, device="cuda", generator=g).to(BF)
    y = ops.conv(x, pc, cache=cache, resid=resid)
    assert ops.conv_kernel_name(x.shape, pc, resid=True) == "conv3x3_halo4x_kernel"
    torch.cuda.synchronize()
    xin = torch.cat([cache, x], dim=0)                            # frame t of the output reads xin[t : t + 3]
    # rows: image top / bottom, the seams of the 16-row tiles (15|16, 351|352), the last full tile row (703|704); frames 0, 3, 7
    for t in (0, 3, 7):
        for r0, r1 in _bands(H, (0, 15, 351, 703, 718)):
            rows = r1 - r0 + 1
            slab = torch.zeros(3, rows + 2, W + 2, Cc, device="cuda")
            a, bnd = max(r0 - 1, 0), min(r1 + 2, H)
            slab[:, a - (r0 - 1): a - (r0 - 1) + (bnd - a), 1:W + 1] = xin[t:t + 3, a:bnd].float()
            ref = F.conv3d(slab.cpu().permute(3, 0, 1, 2)[None], w, b)[0, :, 0].permute(1, 2, 0)      # [rows, W, Cc]
            ref = (ref + resid[t, r0:r1 + 1].float().cpu()).to(BF)
            close(f"prod_conv3d t{t} rows {r0}-{r1}", y[t, r0:r1 + 1], ref)


def _rms_rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt().clamp_min(1e-20))


def test_prodshape_conv3d_128_no_cache_w_first_sampled():
    """The FIRST frame-batch of a clip: 128 -> 128 3x3x3 causal conv on 9 x 720 x 1280 WITHOUT a conv cache (frame 0 replicated twice in
    front: CogVideoXCausalConv3d's constant-replicate pad, /root/reference/inference_script.py:408, 500).  The product runs frames 0 / 1 of
    such a launch on the temporal weight sums (dove_conv_desc.w_first: W0+W1+W2 on frame 0; W0+W1 on frame 0, then W2 on frame 1) - one / two
    temporal groups instead of three.  Checked against plain F.conv3d of the replicate-padded input at frames 0, 1, 2 and 8, on the rows a
    tile / round indexing bug would hit; and the error of BOTH weight-sum forms (w_first here, w_sub of the upsample conv) is printed next
    to the direct (per-tap) forms of the same launches, so the price of the one extra bf16 rounding of the summed weights has a number."""
    import dataclasses

    import torch.nn.functional as F
    T, H, W, Cc = 9, 720, 1280, 128
    g = torch.Generator(device="cuda").manual_seed(151)
    gw = torch.Generator().manual_seed(152)
    w = (torch.randn(Cc, Cc, 3, 3, 3, generator=gw) * (Cc * 27) ** -0.5).to(BF).float()
    b = torch.randn(Cc, generator=gw) * 0.1
    pc = ops.pack_conv(w, b, "cuda")
    assert pc.w_first is not None
    x = torch.randn(T, H, W, Cc, device="cuda", generator=g).to(BF)
    y = ops.conv(x, pc)                                              # w_first form (no cache handed over)
    y_direct = ops.conv(x, dataclasses.replace(pc, w_first=None))    # the same launch on the per-tap weights (replicated frame read 3 / 2 times)
    assert ops.conv_kernel_name(x.shape, pc) == "conv3x3_halo4x_kernel"
    torch.cuda.synchronize()
    xin = torch.cat([x[:1], x[:1], x], dim=0)                        # frame t of the output reads xin[t : t + 3]
    refs, gots, gots_d = [], [], []
    for t in (0, 1, 2, 8):
        for r0, r1 in _bands(H, (0, 15, 351, 703, 718)):
            rows = r1 - r0 + 1
            slab = torch.zeros(3, rows + 2, W + 2, Cc, device="cuda")
            a, bnd = max(r0 - 1, 0), min(r1 + 2, H)
            slab[:, a - (r0 - 1): a - (r0 - 1) + (bnd - a), 1:W + 1] = xin[t:t + 3, a:bnd].float()
            ref = F.conv3d(slab.cpu().permute(3, 0, 1, 2)[None], w, b)[0, :, 0].permute(1, 2, 0)      # [rows, W, Cc] fp32
            close(f"prod_conv3d_first t{t} rows {r0}-{r1}", y[t, r0:r1 + 1], ref.to(BF))
            close(f"prod_conv3d_first(direct) t{t} rows {r0}-{r1}", y_direct[t, r0:r1 + 1], ref.to(BF))
            if t < 2:
                refs.append(ref); gots.append(y[t, r0:r1 + 1].float().cpu()); gots_d.append(y_direct[t, r0:r1 + 1].float().cpu())
    # frames >= 2 never touch the sums: the two launches agree bit for bit there
    assert torch.equal(y[2:], y_direct[2:])
    R = torch.cat(refs)
    e_sum, e_dir = _rms_rel(torch.cat(gots), R), _rms_rel(torch.cat(gots_d), R)
    print(f"[weight sums] 3x3x3 128->128 no cache, frames 0-1 at 720x1280, rms-rel vs fp32 F.conv3d: w_first {e_sum:.3e}  direct {e_dir:.3e}  "
          f"| vs the bf16-rounded reference: w_first {_rms_rel(torch.cat(gots), R.to(BF)):.3e}  direct {_rms_rel(torch.cat(gots_d), R.to(BF)):.3e}")
    # upsample-fused 256 -> 256 3x3 at 360x640 -> 720x1280 (the launch of test_prodshape_upsample_conv_256_sampled): w_sub vs direct taps
    H2, W2, C2 = 360, 640, 256
    w2 = (torch.randn(C2, C2, 3, 3, generator=gw) * (C2 * 9) ** -0.5).to(BF).float()
    b2 = torch.randn(C2, generator=gw) * 0.1
    pc2 = ops.pack_conv(w2, b2, "cuda")
    x2 = torch.randn(2, H2, W2, C2, device="cuda", generator=g).to(BF)
    y2 = ops.conv(x2, pc2, up=1, pad=(1, 1))
    y2_direct = ops.conv(x2, dataclasses.replace(pc2, w_sub=None), up=1, pad=(1, 1))
    torch.cuda.synchronize()
    r0, r1 = 350, 357
    up = x2[1].float()[(torch.arange(r0 - 1, r1 + 2, device="cuda") >> 1)][:, (torch.arange(-1, 2 * W2 + 1, device="cuda").clamp(0, 2 * W2 - 1) >> 1)]
    up[:, 0] = 0
    up[:, -1] = 0
    ref2 = F.conv2d(up.cpu().permute(2, 0, 1)[None], w2, b2)[0].permute(1, 2, 0)
    e2_sum, e2_dir = _rms_rel(y2[1, r0:r1 + 1], ref2), _rms_rel(y2_direct[1, r0:r1 + 1], ref2)
    print(f"[weight sums] up 3x3 256->256 360x640 -> 720x1280, rows {r0}-{r1}, rms-rel vs fp32 F.conv2d: w_sub {e2_sum:.3e}  direct {e2_dir:.3e}  "
          f"| vs the bf16-rounded reference: w_sub {_rms_rel(y2[1, r0:r1 + 1], ref2.to(BF)):.3e}  direct {_rms_rel(y2_direct[1, r0:r1 + 1], ref2.to(BF)):.3e}")
    # both forms round their result to bf16 (rms 1.1e-3 by itself); the summed weights add one rounding of the WEIGHTS (2^-9 relative per sum)
    assert e_sum < 4e-3 and e_dir < 4e-3 and e2_sum < 4e-3 and e2_dir < 4e-3, (e_sum, e_dir, e2_sum, e2_dir)


def _time_doubled(src, first_single):
    """[Ts,H,W,C] -> Upsample3D's time doubling: every frame twice, the first one once when ``first_single``."""
    Ts = src.shape[0]
    idx = ([0] + [1 + i // 2 for i in range(2 * (Ts - 1))]) if first_single else [i // 2 for i in range(2 * Ts)]
    return src[idx].contiguous()


@pytest.mark.parametrize("name,cin,cout,Ts,H,W,tdup,cached,nb,resid", [
    ("head_odd", 128, 128, 3, 20, 40, 2, False, 1, False),          # 1 + 4 frames, no cache: frame 0 on w012, then {01}{2} / {0}{12} by parity
    ("tail_even_cache", 128, 256, 2, 17, 33, 1, True, 1, True),      # 4 frames behind an equal-pair cache, ragged tiles, residual epilogue
    ("even_no_cache", 64, 128, 2, 16, 32, 1, False, 1, False),       # an even first batch: frames 0 / 1 on w012
    ("one_pair_cache", 256, 128, 1, 16, 64, 1, True, 1, False),      # a single doubled frame (a 1-frame piece of a split batch)
    ("tiles_nb3", 128, 128, 2, 16, 32, 1, True, 3, False),           # three instances (tiled VAE batches), each with its own cache
    ("head_odd_nb2", 128, 128, 2, 18, 34, 2, False, 2, False),
])
def test_conv_frame_pairs_tdup(name, cin, cout, Ts, H, W, tdup, cached, nb, resid):
    """dove_conv_desc.tdup / w_pair: the first causal conv behind CogVideoXUpsample3D's time doubling (decode_latents, /root/reference/
    inference_script.py:500) told that its input frames come in bit-identical pairs runs two temporal groups per frame - against plain
    F.conv3d on the same (doubled) input, against the same launch WITHOUT the declaration (per-tap arithmetic), and the fused GroupNorm
    statistics against a pass over the stored output."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(171)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * (cin * 27) ** -0.5).to(BF).float()
    b = torch.randn(cout, generator=g) * 0.1
    pc = ops.pack_conv(w, b, "cuda", pair=True)
    xs = [_time_doubled(rnd(Ts, H, W, cin, seed=180 + i), tdup == 2) for i in range(nb)]
    T = xs[0].shape[0]
    caches = [_time_doubled(rnd(1, H, W, cin, seed=190 + i), False) for i in range(nb)] if cached else None
    x = torch.cat(xs).cuda()
    cache = None
    if cached:
        cache = torch.stack(caches).cuda() if nb > 1 else caches[0].cuda()
    r = rnd(nb * T, H, W, cout, seed=175).cuda() if resid else None
    y = ops.conv(x, pc, cache=cache, resid=r, nb=nb, tdup=tdup, gn_eps=1e-6)
    y_plain = ops.conv(x, pc, cache=cache, resid=r, nb=nb, weight_sums=False)
    torch.cuda.synchronize()
    assert ops.conv_kernel_name((T, H, W, cin), pc, resid=resid) == "conv3x3_halo4x_kernel"
    for i in range(nb):
        front = caches[i] if cached else torch.cat([xs[i][:1]] * 2)
        xin = torch.cat([front, xs[i]]).float().permute(3, 0, 1, 2)[None]                      # [1, C, T + 2, H, W]
        ref = F.conv3d(F.pad(xin, (1, 1, 1, 1)), w, b)[0].permute(1, 2, 3, 0)                    # [T, H, W, cout]
        if resid:
            ref = ref + r[i * T:(i + 1) * T].float().cpu()
        close(f"tdup_{name} instance {i}", y[i * T:(i + 1) * T], ref.to(BF))
        close(f"tdup_{name} instance {i} (no declaration)", y_plain[i * T:(i + 1) * T], ref.to(BF))
    st = y.gn_stats[0] if getattr(y, "gn_stats", None) is not None else None
    if st is not None:                                            # epilogue statistics == a pass over what was stored
        want = ops.groupnorm_stats(y, 1e-6, nb)
        torch.cuda.synchronize()
        assert float((st - want).abs().max()) < 1e-4 * float(want.abs().max().clamp_min(1.0)), (st - want).abs().max()
    # the declaration is refused where it cannot hold: frame 0 single (2) behind a cache; a declaration without the pair sums
    d = ops.L.ConvDesc()
    d.x = d.w = d.out = x.data_ptr()
    d.t_in = d.t_out = T
    d.h_in = d.h_out = H
    d.w_in = d.w_out = W
    d.cin, d.cout_pad, d.cout_store, d.kt, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.ldo = cin, cout, cout, 3, 3, 3, 1, 1, 1, cout
    d.tdup = 1
    assert ops.L.load().dove_conv_igemm_bf16(d, None) != 0 and b"w_pair" in ops.L.load().dove_last_error()
    d.w_pair, d.tdup, d.cache = pc.w_pair.data_ptr(), 2, x.data_ptr()
    assert ops.L.load().dove_conv_igemm_bf16(d, None) != 0 and b"tdup == 2" in ops.L.load().dove_last_error()


@pytest.mark.parametrize("tmode,T_in,t_out", [(0, 8, 8), (1, 4, 8)])
def test_prodshape_upsample_conv_256_sampled(tmode, T_in, t_out):
    """Upsample-fused 256 -> 256 3x3 conv, 360 x 640 -> 720 x 1280 (CogVideoXUpsample3D of decoder up-block 2: the nearest x2
    resize lives in the conv's addressing).  tmode 1 also doubles the frames (frame t reads input frame t >> 1)."""
    import torch.nn.functional as F
    H, W, Cc = 360, 640, 256
    g = torch.Generator(device="cuda").manual_seed(111)
    gw = torch.Generator().manual_seed(112)
    w = (torch.randn(Cc, Cc, 3, 3, generator=gw) * (Cc * 9) ** -0.5).to(BF).float()
    b = torch.randn(Cc, generator=gw) * 0.1
    pc = ops.pack_conv(w, b, "cuda")
    x = torch.randn(T_in, H, W, Cc, device="cuda", generator=g).to(BF)
    y = ops.conv(x, pc, up=1, pad=(1, 1), tmode=tmode, t_out=t_out)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (t_out, 2 * H, 2 * W, Cc)
    H2, W2 = 2 * H, 2 * W
    cidx = torch.arange(-1, W2 + 1, device="cuda")
    cval = ((cidx >= 0) & (cidx < W2)).float()
    for t in (0, t_out // 2, t_out - 1):
        src = x[E._frame_index(t, tmode)].float()
        for r0, r1 in _bands(H2, (0, 15, 351, 703, 718)):
            ridx = torch.arange(r0 - 1, r1 + 2, device="cuda")
            rval = ((ridx >= 0) & (ridx < H2)).float()
            slab = src[(ridx.clamp(0, H2 - 1) >> 1)][:, (cidx.clamp(0, W2 - 1) >> 1)] * rval[:, None, None] * cval[None, :, None]
            ref = F.conv2d(slab.cpu().permute(2, 0, 1)[None], w, b)[0].permute(1, 2, 0).to(BF)           # [rows, W2, Cc]
            close(f"prod_upconv tmode{tmode} t{t} rows {r0}-{r1}", y[t, r0:r1 + 1], ref)


def test_prodshape_dit_linears_sampled():
    """The DiT's two extreme linears at N = 18 226 rows: qkv (3072 -> 9216, + bias; 2592 tiles = 10 full rounds of gemm8p + a 50-row
    tail on igemm_fast) and ff2 (12 288 -> 3072 with the gated in-place residual, text / video gate rows split at 226; 864 tiles =
    16 384 rows on gemm8p + 1842 on the tail kernel).  Sampled rows: first / last, the 256-row tile seams, both sides of the gate's
    row-class boundary and of each tail split."""
    N = 18226
    g = torch.Generator(device="cuda").manual_seed(121)
    gw = torch.Generator().manual_seed(122)
    rows = torch.tensor([0, 1, 225, 226, 227, 255, 256, 257, 4095, 4096, 9999, 16383, 16384, 16385, 18175, 18176, 18177, 18224, 18225])
    # qkv
    w = (torch.randn(9216, 3072, generator=gw) * 3072 ** -0.5).to(BF).float()
    b = torch.randn(9216, generator=gw) * 0.1
    pl = ops.pack_conv(w, b, "cuda")
    x = torch.randn(N, 3072, device="cuda", generator=g).to(BF)
    z = ops.linear(x, pl)
    torch.cuda.synchronize()
    ref = (x[rows.cuda()].float().cpu() @ w.t() + b).to(BF)
    close("prod_linear_qkv", z[rows.cuda()], ref)
    del z, pl, w
    # ff2, gated residual in place
    w = (torch.randn(3072, 12288, generator=gw) * 12288 ** -0.5).to(BF).float()
    b = torch.randn(3072, generator=gw) * 0.1
    pl = ops.pack_conv(w, b, "cuda")
    x = torch.randn(N, 12288, device="cuda", generator=g).to(BF)
    hs = torch.randn(N, 3072, device="cuda", generator=g).to(BF)
    gate = torch.randn(2, 3072, generator=gw)
    hs0 = hs[rows.cuda()].float().cpu()
    out = ops.linear(x, pl, resid=hs, gate=gate.cuda().contiguous(), gate_split=226, out=hs)
    torch.cuda.synchronize()
    gsel = gate[(rows >= 226).long()]
    ref = (hs0 + gsel * (x[rows.cuda()].float().cpu() @ w.t() + b)).to(BF)
    close("prod_linear_ff2_gated", out[rows.cuda()], ref)


def test_prodshape_dit_linears_mx_sampled():
    """The same two linears on the MXFP8 GEMM of BASELINE configs[4] at N = 18 226 rows (ragged last row tile, 10.1 / 3.4 rounds of 256
    tiles), against dequantise-then-fp32-matmul of the SAME quantised operands at sampled rows (block scales run along K of a row, so
    a row's reference needs that row only)."""
    N = 18226
    g = torch.Generator(device="cuda").manual_seed(123)
    gw = torch.Generator().manual_seed(124)
    rows = torch.tensor([0, 1, 225, 226, 227, 255, 256, 257, 4095, 4096, 9999, 16383, 16384, 16385, 18175, 18176, 18177, 18224, 18225])
    # qkv
    w = torch.randn(9216, 3072, generator=gw) * 3072 ** -0.5
    b = torch.randn(9216, generator=gw) * 0.1
    pw = ops.pack_linear_mx(w, b, "cuda")
    x = (torch.randn(N, 3072, device="cuda", generator=g) * torch.exp(torch.randn(1, 3072, device="cuda", generator=g))).to(BF)
    z = ops.linear_mx(ops.mx_quant(x), pw)
    torch.cuda.synchronize()
    ref = E.linear_mx_ref(x[rows.cuda()].cpu(), w, b)
    close("prod_linear_mx_qkv", z[rows.cuda()], ref)
    del z, pw, w
    # ff2, gated residual
    w = torch.randn(3072, 12288, generator=gw) * 12288 ** -0.5
    b = torch.randn(3072, generator=gw) * 0.1
    pw = ops.pack_linear_mx(w, b, "cuda")
    x = torch.randn(N, 12288, device="cuda", generator=g).to(BF)
    hs = torch.randn(N, 3072, device="cuda", generator=g).to(BF)
    gate = torch.randn(2, 3072, generator=gw)
    out = ops.linear_mx(ops.mx_quant(x), pw, resid=hs, gate=gate.cuda().contiguous(), gate_split=226)
    torch.cuda.synchronize()
    y = E.linear_mx_ref(x[rows.cuda()].cpu(), w, b).float()
    ref = (hs[rows.cuda()].float().cpu() + gate[(rows >= 226).long()] * y)
    # linear_mx_ref rounded y to bf16 before the gate; the kernel applies bias, gate and residual in fp32 and rounds once
    close("prod_linear_mx_ff2_gated", out[rows.cuda()], ref.to(BF))


def _sample_queries(N):
    return torch.tensor([0, 1, 31, 32, 127, 128, 129, 4095, 4096, 9000, 9001, 18175, 18176, 18207, 18208, 18224, 18225])


def test_prodshape_attention_18226_sampled():
    """bf16 flash attention at the headline sequence length (285 KV tiles, ragged last tile of 50 keys, 143 query blocks of 128) on
    2 heads, against the exact fp32 softmax attention of the same bf16 operands at sampled query rows."""
    N, heads = 18226, 2
    npad = (N + 127) // 128 * 128
    g = torch.Generator().manual_seed(131)
    q = (torch.randn(heads, N, 64, generator=g) * 0.5).to(BF)          # Qh carries scale * log2(e): scores ~ N(0, 4) in base 2
    k = (torch.randn(heads, N, 64, generator=g) * 0.7).to(BF)          # |q| |k| stays below the 40 above which the bound is not used
    v = torch.randn(heads, 64, N, generator=g).to(BF)
    Q = torch.zeros(heads, npad, 64, dtype=BF)
    K = torch.zeros(heads, npad, 64, dtype=BF)
    V = torch.zeros(heads, 64, npad, dtype=BF)
    Q[:, :N], K[:, :N], V[:, :, :N] = q, k, v
    E.vt_quad_swap(V)
    got = ops.attention(Q.cuda(), K.cuda(), V.cuda(), N, npad, heads, torch.zeros(N, heads * 64, dtype=BF, device="cuda"))
    torch.cuda.synchronize()
    rows = _sample_queries(N)
    p = torch.softmax(torch.einsum("hqd,hkd->hqk", q.float()[:, rows], k.float()) * math.log(2.0), dim=-1)
    ref = torch.einsum("hqk,hdk->hqd", p, v.float()).permute(1, 0, 2).reshape(len(rows), heads * 64).to(BF)
    close("prod_attention_18226", got[rows.cuda()], ref, rtol=3e-2, afrac=8e-3)
    assert ops.attention_head_paths(None, heads) == ["attn_fwd_kernel"] * heads     # the call above: the running maximum
    n2 = _norm2(Q, K, N).cuda()
    assert 40.0 < float(1.01 * (n2[:, 0] * n2[:, 1]).sqrt().max()) < 80.0          # (round 5 asserted "< 60" against a cutoff of 40: both heads fell back)
    got = ops.attention(Q.cuda(), K.cuda(), V.cuda(), N, npad, heads, torch.zeros(N, heads * 64, dtype=BF, device="cuda"), norm2=n2)
    torch.cuda.synchronize()
    assert ops.attention_head_paths(n2) == ["attn_pipe_kernel"] * heads             # the production kernel served both heads
    close("prod_attention_18226_bound", got[rows.cuda()], ref, rtol=3e-2, afrac=8e-3)


def test_prodshape_attention_mx_18226_sampled():
    """The MXFP8 attention of BASELINE configs[4] at N = 18 226 (its design argument - per-(query, tile) probability scales - is made
    for this length): against the exact softmax attention over the DEQUANTISED fp8 operands, so that what is measured is the
    kernel (P quantisation + accumulation), at sampled query rows; tolerance of test_attention_mx_spike_and_flat_tail."""
    N, heads = 18226, 2
    npad = (N + 127) // 128 * 128
    g = torch.Generator().manual_seed(141)
    q = torch.randn(heads, N, 64, generator=g) * 0.5
    k = torch.randn(heads, N, 64, generator=g)
    v = torch.randn(heads, 64, N, generator=g)
    Q8, K8, V8, Vs = _mx_bufs(heads, npad)
    Q8[:, :N] = (q * 8).to(torch.float8_e4m3fn).view(torch.uint8)
    K8[:, :N] = k.to(torch.float8_e4m3fn).view(torch.uint8)
    vp = torch.zeros(heads * 64, npad)
    vp[:, :N] = v.reshape(heads * 64, N)
    vq, ve = E.mx_quant_ref(vp)
    V8.copy_(E.v8_store_order(vq.view(torch.uint8).reshape(heads, 64, npad)))
    Vs.copy_(ve.reshape(heads, 64, npad // 64, 2).permute(0, 2, 1, 3))
    got = ops.attention_mx(Q8.cuda(), K8.cuda(), V8.cuda(), Vs.cuda(), N, npad, heads, torch.zeros(N, heads * 64, dtype=BF, device="cuda"))
    torch.cuda.synchronize()
    rows = _sample_queries(N)
    qd, kd = _fp8(Q8)[:, :N] * 0.125, _fp8(K8)[:, :N]
    vd = E.mx_dequant(vq, ve).reshape(heads, 64, npad)[:, :, :N]
    p = torch.softmax(torch.einsum("hqd,hkd->hqk", qd[:, rows], kd) * math.log(2.0), dim=-1)
    exact = torch.einsum("hqk,hdk->hqd", p, vd).permute(1, 0, 2).reshape(len(rows), heads * 64)
    close("prod_attention_mx_18226", got[rows.cuda()], exact.to(BF), rtol=4e-2, afrac=1.5e-2)
    rel = float((got[rows.cuda()].float().cpu() - exact).pow(2).mean().sqrt() / exact.pow(2).mean().sqrt())
    print(f"attention_mx N=18226 sampled rows: rel RMS error vs exact (dequantised operands) {rel:.4f}")
    assert rel < 6e-2, rel
