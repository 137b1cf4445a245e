"""Optical flow (csrc/flow.hip, dove_amd/flow.py) on the GPU: every operator against torch in fp64 on the host, the warping error against
goldens made by the reference's flow_warp / fbConsistencyCheck, the whole network against the reference's RAFT run in fp64
(tools/make_flow_goldens.py), and the metric's command line against the test's own composition of the two."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dove_amd import flow, ops
from dove_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


def nhwc(t):            # [N,C,H,W] host fp64 / fp32 -> channels-last float32 on the device
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def nchw64(t):          # channels-last device tensor -> [N,C,H,W] host fp64
    return t.detach().cpu().double().permute(0, 3, 1, 2)


# ---- 1. conv2d_f32 ---------------------------------------------------------------------------------------------------------------------
CONV_CASES = [(7, 7, 2, 3, 64), (3, 3, 1, 64, 64), (3, 3, 2, 64, 96), (1, 1, 2, 64, 96), (3, 3, 2, 96, 128), (1, 1, 1, 128, 256),
              (1, 1, 1, 324, 256), (3, 3, 1, 256, 192), (7, 7, 1, 2, 128), (3, 3, 1, 128, 64), (3, 3, 1, 256, 126), (1, 5, 1, 384, 128),
              (5, 1, 1, 384, 128), (3, 3, 1, 128, 256), (3, 3, 1, 256, 2), (1, 1, 1, 256, 576)]
CONV_SIZES = [(1, 1), (5, 7), (16, 20), (17, 23)]
ACT_REF = {L.ACT_NONE: (lambda v: v, 1.0), L.ACT_RELU: (torch.relu, 1.0), L.ACT_SIGMOID: (torch.sigmoid, 0.25), L.ACT_TANH: (torch.tanh, 1.0)}


def _signed(g, n, lo, hi):
    return (torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "k%dx%d_s%d_%dto%d" % c)
def test_conv2d_f32_against_fp64(case):
    """|err| <= 1e-6 * (sum|x w| + |b|), the sum in fp64, carried through the epilogue: times |scale| plus 1e-6 |shift| for the folded
    BatchNorm (it is part of the linear map), times the activation's Lipschitz constant (1, 1, 1/4 for sigmoid, 1), times |out_mul|.
    Biases are at least 0.5 in magnitude so that the bound never falls below the float32 spacing of a sigmoid's output.  Every size runs
    two variants, so each case sees all four activations, scale / shift, out_mul and the write into a channel slice of a wider buffer."""
    kh, kw, stride, cin, cout = case
    g = torch.Generator().manual_seed(1000 + CONV_CASES.index(case))
    w = (torch.randn(cout, cin, kh, kw, generator=g) / math.sqrt(cin * kh * kw)).double()
    b = _signed(g, cout, 0.5, 1.0)
    scale, shift = _signed(g, cout, 0.5, 1.5), _signed(g, cout, 0.5, 1.0)
    wd, bd = flow.pack_conv_weight(w).to(DEV), b.float().to(DEV)
    w, b, scale, shift = w.float().double(), b.float().double(), scale.float().double(), shift.float().double()
    worst = 0.0
    for si, (H, W) in enumerate(CONV_SIZES):
        x = torch.randn(2, cin, H, W, generator=g).double()
        lin = F.conv2d(x, w, b, stride=stride, padding=(kh // 2, kw // 2))
        mag = F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=(kh // 2, kw // 2))
        xd = nhwc(x)
        for variant in (0, 1):
            act = (2 * si + variant + CONV_CASES.index(case)) % 4
            fn, lip = ACT_REF[act]
            use_scale, mul = variant == 0, (0.25 if variant == 1 and si % 2 == 0 else 1.0)
            pre, bound = lin, 1e-6 * mag
            if use_scale:
                pre = lin * scale[None, :, None, None] + shift[None, :, None, None]
                bound = 1e-6 * (mag * scale.abs()[None, :, None, None] + shift.abs()[None, :, None, None])
            want, bound = mul * fn(pre), mul * lip * bound
            kw_ = dict(stride=stride, act=act, out_mul=mul)
            if use_scale:
                kw_.update(scale=scale.float().to(DEV), shift=shift.float().to(DEV))
            if variant == 0:
                got = ops.conv2d_f32(xd, wd, bd, **kw_)
            else:                                                # a slice at channel 5 of a buffer 12 channels wider, prefilled
                buf = torch.randn(2, want.shape[2], want.shape[3], cout + 12, generator=g).to(DEV)
                before = buf.clone()
                got = ops.conv2d_f32(xd, wd, bd, out=buf[..., 5:5 + cout], **kw_)
                keep = torch.ones(cout + 12, dtype=torch.bool)
                keep[5:5 + cout] = False
                assert torch.equal(buf[..., keep.to(DEV)], before[..., keep.to(DEV)]), "bytes outside the written slice changed"
            assert tuple(got.shape) == (2, want.shape[2], want.shape[3], cout)
            ratio = float(((nchw64(got) - want).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (case, (H, W), act, use_scale, mul, ratio)
    print(f"conv2d_f32 {case}: worst |err| / bound = {worst:.3f}")


def test_conv2d_f32_reads_a_channel_slice_and_batches_independently():
    g = torch.Generator().manual_seed(5)
    buf = torch.randn(3, 9, 11, 40, generator=g).to(DEV)
    w = torch.randn(24, 16, 3, 3, generator=g) / 12
    wd, bd = flow.pack_conv_weight(w).to(DEV), torch.randn(24, generator=g).to(DEV)
    sl = buf[..., 7:23]
    a = ops.conv2d_f32(sl, wd, bd, act=L.ACT_TANH)
    b = ops.conv2d_f32(sl.contiguous(), wd, bd, act=L.ACT_TANH)
    assert torch.equal(a, b)
    one = ops.conv2d_f32(sl[1:2], wd, bd, act=L.ACT_TANH)
    assert torch.equal(one, a[1:2])                              # an image's result does not depend on its place in the batch


# ---- 2. instance norm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 5, 7), (2, 96, 16, 20), (1, 128, 1, 1)])
def test_instance_norm_f32(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(*shape, generator=g) * 1.3 + 0.4).double()
    r = torch.randn(*shape, generator=g).double()
    xd, rd = nhwc(x), nhwc(r)
    mean, var = x.mean((2, 3), keepdim=True), x.var((2, 3), unbiased=False, keepdim=True)
    want = (x - mean) / torch.sqrt(var + 1e-5)                   # InstanceNorm2d: biased variance, no affine
    if shape[2] * shape[3] > 1:
        assert float((want - F.instance_norm(x, eps=1e-5)).abs().max()) < 1e-12
    if shape[2] * shape[3] == 1:
        assert float(want.abs().max()) == 0.0                    # variance zero: the output is 0
    for relu, resid in ((False, None), (True, None), (True, rd)):
        ref = torch.relu(want) if relu else want
        if resid is not None:
            ref = torch.relu(r.float().double() + ref)
        got = ops.instance_norm_f32(xd, relu=relu, resid=resid)
        again = ops.instance_norm_f32(xd, relu=relu, resid=resid)
        assert torch.equal(got, again)
        err = float((nchw64(got) - ref).abs().max())
        print(f"instance_norm {shape} relu={relu} resid={resid is not None}: max err {err:.2e}")
        assert err <= 1e-5


# ---- 3. correlation --------------------------------------------------------------------------------------------------------------------
def _lookup_ref(levels, coords):
    """corr.py's CorrBlock.__call__ written out: levels [(N*h*w, hl, wl) fp64], coords [N,h,w,2] (x, y) -> [N,h,w,324]."""
    N, h, w, _ = coords.shape
    d = torch.arange(-4, 5, dtype=torch.float64)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), -1)             # [a][b] = (d[a], d[b]), ADDED to (x, y)
    out = []
    for i, lv in enumerate(levels):
        c = coords.reshape(N * h * w, 1, 1, 2) / 2 ** i + delta[None]
        hl, wl = lv.shape[-2:]
        grid = torch.stack([2 * c[..., 0] / (wl - 1) - 1, 2 * c[..., 1] / (hl - 1) - 1], -1)
        out.append(F.grid_sample(lv[:, None], grid, align_corners=True).reshape(N, h, w, 81))
    return torch.cat(out, -1)


@pytest.mark.parametrize("hw", [(16, 20), (17, 21)])
def test_correlation_volume_pyramid_and_lookup(hw):
    h, w = hw
    N, Cc = 2, 256
    g = torch.Generator().manual_seed(h * w)
    f1, f2 = torch.randn(N, h, w, Cc, generator=g), torch.randn(N, h, w, Cc, generator=g)
    levels = ops.corr_pyramid_f32(f1.to(DEV), f2.to(DEV))
    a, b = f1.double().reshape(N, h * w, Cc), f2.double().reshape(N, h * w, Cc)
    vol = (a @ b.transpose(1, 2) / 16).reshape(N * h * w, h, w)
    mag = (a.abs() @ b.abs().transpose(1, 2) / 16).reshape(N * h * w, h, w)
    assert float(((levels[0].cpu().double() - vol).abs() / (1e-6 * mag)).max()) <= 1.0       # the conv's bound: the same MFMA chain
    ref = [vol]
    for i in range(3):
        ref.append(F.avg_pool2d(ref[-1][:, None], 2, stride=2)[:, 0])
    sizes = [tuple(l.shape[1:]) for l in levels]
    assert sizes == [(h >> i, w >> i) for i in range(4)] == [tuple(r.shape[1:]) for r in ref]
    vmax = float(vol.abs().max())
    # a pool is three float32 additions and an exact scaling of values that carry the volume's error
    vol_tol = 1e-6 * float(mag.max())
    for level, (got, want) in enumerate(zip(levels[1:], ref[1:]), 1):       # the roundings of the levels below add up
        assert float((got.cpu().double() - want).abs().max()) <= vol_tol + 3 * level * 2.0 ** -24 * vmax
    # coordinates: fractional, exact integers, and up to 12 px outside the map on every side
    coords = torch.stack([torch.rand(N, h, w, generator=g) * (w + 24) - 12, torch.rand(N, h, w, generator=g) * (h + 24) - 12], -1)
    coords[0, :4] = coords[0, :4].round()
    coords[1, 0, 0] = torch.tensor([-12.0, -12.0])
    coords[1, 0, 1] = torch.tensor([w + 11.0, h + 11.0])
    got = ops.corr_lookup_f32(levels, coords.to(DEV)).cpu().double()
    want = _lookup_ref([l.cpu().double() for l in levels], coords.double())
    # the kernel forms x / 2^l + a - 4 in float32: half an ulp of a coordinate below 64 (2^-19 px) times the steepest slope of the bilinear
    # surface (2 max|corr| per px), on either axis, plus a few roundings of the four-tap sum
    tol = 2 * 2.0 ** -19 * 2 * vmax + 8 * 2.0 ** -24 * vmax
    err = float((got - want).abs().max())
    print(f"corr_lookup {hw}: max err {err:.2e} (tol {tol:.2e})")
    assert err <= tol
    # the same samples from a flow with the pixel grid added by the kernel
    grid = torch.stack(torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")[::-1], -1).float()
    fl = (coords - grid[None]).float()
    buf = torch.zeros(N, h, w, 6)
    buf[..., 4:] = fl
    got2 = ops.corr_lookup_f32(levels, buf.to(DEV)[..., 4:], add_grid=True).cpu().double()
    want2 = _lookup_ref([l.cpu().double() for l in levels], (fl + grid[None]).double())
    assert float((got2 - want2).abs().max()) <= tol


def test_corr_lookup_channel_order_one_hot():
    """Level-major, then the window's FIRST index moves x (the reference adds meshgrid(dy, dx) to (x, y))."""
    h, w = 16, 20
    p, (cx, cy) = 7 * w + 9, (9.0, 7.0)
    for level, (x0, y0) in ((0, (11, 4)), (1, (2, 5)), (2, (3, 1)), (3, (1, 0))):
        levels = [torch.zeros(h * w, h >> i, w >> i) for i in range(4)]
        levels[level][p, y0, x0] = 1.0
        coords = torch.zeros(1, h, w, 2)
        coords[0, 7, 9] = torch.tensor([cx, cy])
        out = ops.corr_lookup_f32([l.to(DEV) for l in levels], coords.to(DEV)).cpu()[0, 7, 9]
        ax, by = x0 - cx / 2 ** level + 4, y0 - cy / 2 ** level + 4           # fractional from level 1 on: two or four taps share the one
        want = torch.zeros(324)
        for a in (math.floor(ax), math.floor(ax) + 1):
            for b in (math.floor(by), math.floor(by) + 1):
                wgt = (1 - abs(ax - a)) * (1 - abs(by - b))
                if 0 <= a < 9 and 0 <= b < 9 and wgt > 0:
                    want[level * 81 + a * 9 + b] = wgt
        assert want.sum() > 0 and torch.allclose(out, want, atol=1e-6), (level, out.nonzero().flatten().tolist(), want.nonzero().flatten().tolist())


# ---- 4. glue and convex upsampling -----------------------------------------------------------------------------------------------------
def test_gru_glue_and_add():
    g = torch.Generator().manual_seed(9)
    hx = torch.randn(2, 5, 7, 40, generator=g).to(DEV)
    zr = torch.rand(2, 5, 7, 32, generator=g).to(DEV)
    q = torch.randn(2, 5, 7, 16, generator=g).to(DEV)
    rhx = torch.full_like(hx, 7.0)
    ops.gru_gate_f32(zr[..., 16:], hx, 16, rhx)
    assert torch.equal(rhx[..., :16], zr[..., 16:] * hx[..., :16]) and torch.equal(rhx[..., 16:], hx[..., 16:])
    want = (1 - zr[..., :16]) * hx[..., :16] + zr[..., :16] * q
    tail = hx[..., 16:].clone()
    ops.gru_update_f32(zr[..., :16], q, hx)
    assert float((hx[..., :16] - want).abs().max()) <= 2 * 2.0 ** -23 * float(want.abs().max()) and torch.equal(hx[..., 16:], tail)
    d = torch.randn(2, 5, 7, 2, generator=g).to(DEV)
    want = hx[..., 38:] + d
    head = hx[..., :38].clone()
    ops.add_f32(hx[..., 38:], d, out=hx[..., 38:])
    assert torch.equal(hx[..., 38:], want) and torch.equal(hx[..., :38], head)
    assert torch.equal(ops.add_f32(hx, rhx, relu=True), torch.relu(hx + rhx))


def test_convex_upsample_against_the_formula_fp64():
    g = torch.Generator().manual_seed(4)
    N, H, W = 2, 5, 7
    fl = (torch.randn(N, 2, H, W, generator=g) * 6).double()
    mask = (torch.randn(N, 576, H, W, generator=g) * 3).double()
    mask[0, :, 1, 2] *= 30                                       # logits of +-200: a softmax that is not stabilised overflows
    mask[1, 64 * 4:64 * 5, 3, 3] += 90
    fl, mask = fl.float().double(), mask.float().double()
    m = torch.softmax(mask.view(N, 1, 9, 8, 8, H, W), dim=2)
    up = F.unfold(8 * fl, [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
    want = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * H, 8 * W)
    buf = torch.zeros(N, H, W, 5)
    buf[..., 3:] = fl.permute(0, 2, 3, 1).float()
    got = ops.convex_upsample_f32(buf.to(DEV)[..., 3:], nhwc(mask)).cpu().double()
    # weights exp(m - max): the float32 difference of logits that matter (above -16) is exact to 2^-20, expf to 2 ulp, nine terms and a division
    tol = 4e-6 * 8 * float(fl.abs().max())
    err = float((got - want).abs().max())
    print(f"convex_upsample: max err {err:.2e} (tol {tol:.2e})")
    assert torch.isfinite(got).all() and err <= tol


# ---- 5. flow_warp_error ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def warp_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "warp_golden.npz"))


@pytest.mark.parametrize("size", ["37x53", "64x96"])
def test_flow_warp_error_against_the_reference(warp_golden, size):
    G = {k[:-len(size) - 1]: warp_golden[k] for k in warp_golden.files if k.endswith("_" + size)}
    h, w = G["mask"].shape
    fw, bw = (torch.from_numpy(G[k])[None].to(DEV) for k in ("fw", "bw"))
    i1, i2 = (torch.from_numpy(G[k])[None].to(DEV) for k in ("img1", "img2"))
    sums, warped, mask = ops.flow_warp_error(i1, i2, fw, bw, want_warped=True, want_mask=True)
    f1, f2 = ((t.cpu().float() / 255.0).to(DEV) for t in (i1, i2))             # IEEE division, on the host
    sums_f, warped_f, mask_f = ops.flow_warp_error(f1, f2, fw, bw, want_warped=True, want_mask=True)
    assert torch.equal(sums, sums_f) and torch.equal(warped, warped_f) and torch.equal(mask, mask_f)        # u8 and f32 inputs agree
    again = ops.flow_warp_error(i1, i2, fw, bw)[0]
    assert torch.equal(again, sums)
    warped, mask, sums = warped[0].cpu().double().numpy(), mask[0].cpu().numpy(), sums[0].cpu().numpy()
    werr = np.abs(warped - G["warped"]).max()
    print(f"flow_warp_error {size}: warped max err {werr:.2e}")
    assert werr <= 1e-4
    near = np.abs(G["d"] - G["thr"]) <= 1e-4 * G["thr"]
    assert near.mean() <= 1e-3, near.mean()
    assert np.array_equal((mask & 1)[~near], G["mask"][~near])
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    sx, sy = xx + G["fw"][0].astype(np.float64), yy + G["fw"][1].astype(np.float64)
    inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    assert np.array_equal((mask >> 1) & 1, inside.astype(np.uint8))
    img1 = G["img1"].astype(np.float32).astype(np.float64) / 255.0

    def energy(wimg, m):
        m = m & ~near
        return (((img1 - wimg) ** 2).sum(-1) * m).sum() / (3.0 * m.sum())

    e_ref = energy(G["warped"], (G["mask"] == 1) & inside)
    e_gpu = energy(warped, (mask == 3))
    print(f"flow_warp_error {size}: E {e_gpu:.9e} vs {e_ref:.9e}, mask share {float((mask == 3).mean()):.3f}")
    assert 0 < e_ref and abs(e_gpu - e_ref) <= 1e-5 * e_ref
    # the kernel's own sums are the sums of what it returned (float32 images, fp64 accumulation)
    i1f = (G["img1"].astype(np.float32) / np.float32(255.0)).astype(np.float64)
    full = (((i1f - warped) ** 2).sum(-1) * (mask == 3)).sum()
    assert sums[1] == (mask == 3).sum() and abs(sums[0] - full) <= 1e-6 * full


def test_flow_warp_error_zero_flow():
    g = torch.Generator().manual_seed(2)
    imgs = torch.randint(0, 256, (3, 37, 53, 3), generator=g, dtype=torch.uint8)
    z = torch.zeros(2, 2, 37, 53, device=DEV)
    sums, warped, mask = ops.flow_warp_error(imgs[:2].to(DEV), imgs[1:].to(DEV), z, z, want_warped=True, want_mask=True)
    assert bool((mask == 3).all()) and torch.equal(warped.cpu(), imgs[1:].float() / 255.0)
    for n in range(2):
        d = imgs[n].double() / 255.0 - imgs[n + 1].double() / 255.0
        e = float(sums[n, 0]) / (3 * float(sums[n, 1]))
        assert float(sums[n, 1]) == 37 * 53 and abs(e - float((d ** 2).mean())) <= 1e-7 * float((d ** 2).mean())


# ---- 6. raft_flow ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raft():
    return flow.RaftWeights.from_state_dict(flow.random_raft_state(1234))       # tools/make_flow_goldens.py's SEED


def _images(G):
    img = 2.0 * (torch.from_numpy(G["frames"]).permute(0, 3, 1, 2).float() / 255.0) - 1.0
    pairs = G["pairs"]
    return img[torch.from_numpy(pairs[:, 0])].to(DEV), img[torch.from_numpy(pairs[:, 1])].to(DEV)


def _stage_report(G, taps):
    lines = []
    for key in ("fmap1", "corr0", "delta0"):
        t = nchw64(taps[key]).reshape(-1)
        assert tuple(G[key + "_shape"]) == tuple(nchw64(taps[key]).shape), key
        err = float((t[torch.from_numpy(G[key + "_idx"])] - torch.from_numpy(G[key + "_val"])).abs().max())
        lines.append(f"{key}: sampled max err {err:.2e}" + ("  <-- leaves 1e-4" if err > 1e-4 else ""))
    return "; ".join(lines)


@pytest.mark.parametrize("name", ["flow_golden.npz", "flow_golden_pad.npz"])
def test_raft_flow_against_the_reference_fp64(golden_dir, raft, name):
    """Gate: max-abs error <= 20 x the deviation of the reference's own fp32 run from its fp64 run, per case, output and iteration
    count (stored by the generator).  flow_up is stored rounded to float32: below 1e-6 px on these flows."""
    G = np.load(os.path.join(golden_dir, name))
    i1, i2 = _images(G)
    report, bad = None, []
    for iters in (4, 20):
        taps = {} if iters == 4 else None
        low, up = flow.raft_flow(raft, i1, i2, iters=iters, taps=taps)
        if taps is not None:
            report = _stage_report(G, taps)
        for what, got in (("low", low), ("up", up)):
            want = torch.from_numpy(G[f"flow_{what}_{iters}"]).double()
            assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
            err, gate = float((got.cpu().double() - want).abs().max()), 20 * float(G[f"dev_{what}_{iters}"])
            print(f"raft_flow {name} iters {iters} flow_{what}: max err {err:.3e} px, gate {gate:.3e} (|flow| max {float(want.abs().max()):.1f})")
            if not err <= gate:
                bad.append((what, iters, err, gate))
    print("stages at the first round:", report)
    assert not bad, (bad, report)


def test_raft_flow_grouping_repeat_and_flow_init(golden_dir, raft):
    G = np.load(os.path.join(golden_dir, "flow_golden.npz"))
    i1, i2 = _images(G)
    low2, up2 = flow.raft_flow(raft, i1, i2, iters=3, group=2)
    low1, up1 = flow.raft_flow(raft, i1, i2, iters=3, group=1)
    assert torch.equal(low1, low2) and torch.equal(up1, up2)                     # groups of 1 and of 2
    lowa, upa = flow.raft_flow(raft, i1, i2, iters=3)
    assert torch.equal(lowa, low2) and torch.equal(upa, up2)                     # two calls, and the planner's own grouping
    lowz, upz = flow.raft_flow(raft, i1, i2, iters=3, flow_init=torch.zeros_like(low2))
    assert torch.equal(lowz, low2) and torch.equal(upz, up2)
    lows, _ = flow.raft_flow(raft, i1[1:], i2[1:], iters=3)
    assert torch.equal(lows, low2[1:])                                           # a pair alone
    with pytest.raises(ValueError, match="at least 128"):
        flow.raft_flow(raft, i1[..., :96, :], i2[..., :96, :], iters=1)


# ---- 7. warping_error and the command line ---------------------------------------------------------------------------------------------
def test_eval_ewarp_cli_is_the_composition(tmp_path, golden_dir):
    """A 3-frame 131 x 165 clip and rule-generated weights saved with the ``module.`` prefix.  With random weights the two flows of a pair
    are unrelated and a few px long, so almost no pixel would pass the forward-backward check: the last conv of the flow head is scaled
    by 1/256 here, which keeps the flows at a fraction of a pixel and the masks populated.  This pins the composition, not a value."""
    from dove_amd import eval_ewarp as E
    fr = np.load(os.path.join(golden_dir, "flow_golden_pad.npz"))["frames"]                      # 2 frames of 131 x 165
    frames = np.concatenate([fr, np.roll(fr[:1], 3, axis=2)])                                    # 3 frames
    pred = tmp_path / "pred"
    pred.mkdir()
    np.save(pred / "clip.npy", frames)
    sd = flow.random_raft_state(77)
    for leaf in ("weight", "bias"):
        sd[f"update_block.flow_head.conv2.{leaf}"] = sd[f"update_block.flow_head.conv2.{leaf}"] / 256
    torch.save({"module." + k: v for k, v in sd.items()}, tmp_path / "raft.pth")
    before = dict(flow.COUNTERS)
    out = E.main(["--pred", str(pred), "--model", str(tmp_path / "raft.pth"), "--out", str(tmp_path / "out"), "--iters", "3"])
    assert flow.COUNTERS["fnet_frames"] - before["fnet_frames"] == 3                             # once per frame, not per pair and direction
    assert flow.COUNTERS["cnet_frames"] - before["cnet_frames"] == 3
    with open(tmp_path / "out" / "metrics_ewarp.json") as f:
        got = json.load(f)
    assert got == json.loads(json.dumps(out)) and got["count"] == 1 and set(got["per_sample"]["clip"]) == {"warping_error"}
    # the test's own composition: raft_flow per pair and direction, flow_warp_error, the formula
    W = flow.RaftWeights.from_state_dict(sd)
    ft = torch.from_numpy(frames).to(DEV)
    img = flow.frames_to_images(ft)
    _, fw = flow.raft_flow(W, img[:-1], img[1:], iters=3)
    _, bw = flow.raft_flow(W, img[1:], img[:-1], iters=3)
    sums, _, _ = ops.flow_warp_error(ft[:-1], ft[1:], fw, bw)
    sums = sums.cpu().numpy()
    assert (sums[:, 1] > 0).all(), sums
    want = 1000.0 * float(np.mean(sums[:, 0] / (3.0 * sums[:, 1])))
    direct = flow.warping_error(torch.from_numpy(frames), W, iters=3)
    print(f"warping_error: {direct['warping_error']:.6f} (composition {want:.6f}), valid pixels per pair {sums[:, 1].tolist()}")
    assert abs(direct["warping_error"] - want) <= 1e-9 * want
    assert got["per_sample"]["clip"]["warping_error"] == round(want, 4) and got["average"]["warping_error"] == round(round(want, 4), 4)
