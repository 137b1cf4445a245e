"""LPIPS and DISTS on the GPU (csrc/percep.hip, dove_amd/percep.py): the fast trunk conv bit for bit against flow.hip's kernel, the general
walk and the small operators against torch in fp64 on the host, the two heads against the fp64 restatement (tests/percep_ref.py) fed the
same fp32 features, the whole networks against the restatement with the gate taken from the restatement's own fp32-vs-fp64 deviation,
and the surfaces against the test's own composition."""
import json
import math
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import percep_ref as R
from dove_amd import flow, ops, percep
from dove_amd import lib as L
from dove_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAST, GENERAL = "convnet3x3_f32_kernel", "conv_f32_kernel"


def nhwc(t):            # [N,C,H,W] host -> channels-last float32 on the device
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def nchw64(t):          # channels-last device tensor -> [N,C,H,W] host fp64
    return t.detach().cpu().double().permute(0, 3, 1, 2)


# ---- 1. the fast walk: the bits of conv_f32_kernel ---------------------------------------------------------------------------------------
# cout below 128 runs on conv_f32_kernel (the fast walk was measured to lose there): those cases stay, and check the routing; ragged N
# on the fast walk is cout 132, 200 and 260
FAST_CASES = [(64, 64), (64, 128), (128, 128), (256, 256), (256, 512), (512, 512), (64, 96), (64, 200), (64, 132), (128, 260)]


def _walk_of(cout):
    return FAST if cout >= 128 else GENERAL
FAST_SIZES = [(1, 1), (5, 7), (16, 20), (17, 23), (9, 140)]      # the last: rows wider than a tile's 128 pixels, and a ragged last tile


@pytest.mark.parametrize("case", FAST_CASES, ids=lambda c: "%dto%d" % c)
def test_fast_conv_is_bit_identical_to_conv2d_f32(case):
    cin, cout = case
    g = torch.Generator().manual_seed(2000 + FAST_CASES.index(case))
    w = flow.pack_conv_weight(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).to(DEV)
    b = (0.1 * torch.randn(cout, generator=g)).to(DEV)
    for si, (H, W) in enumerate(FAST_SIZES):
        x = nhwc(torch.randn(2, cin, H, W, generator=g))
        want = ops.conv2d_f32(x, w, b, act=L.ACT_RELU)
        got, name = ops.convnet_conv_f32(x, w, b, relu=True, want_name=True)
        assert name == _walk_of(cout), (case, H, W, name)
        same = torch.equal(got, want)
        print(f"{name} {cin}->{cout} @ 2x{H}x{W}: equal bits {same}, max |diff| {float((got - want).abs().max()):.3e}")
        assert same
        # without the ReLU (and without a bias), into a channel slice at channel 8 of a buffer 12 channels wider, prefilled
        buf = torch.randn(2, H, W, cout + 12, generator=g).to(DEV)
        before = buf.clone()
        got, name = ops.convnet_conv_f32(x, w, None if si % 2 else b, relu=False, out=buf[..., 8:8 + cout], want_name=True)
        assert name == _walk_of(cout)
        assert torch.equal(got, ops.conv2d_f32(x, w, None if si % 2 else b, act=L.ACT_NONE))
        keep = torch.ones(cout + 12, dtype=torch.bool)
        keep[8:8 + cout] = False
        assert torch.equal(buf[..., keep.to(DEV)], before[..., keep.to(DEV)]), "bytes outside the written slice changed"
    # the input as a channel slice of a wider buffer (pixel stride 2 cin), and two calls give the same bits
    wide = nhwc(torch.randn(2, 2 * cin, 17, 23, generator=g))
    xs = wide[..., cin:]
    got, name = ops.convnet_conv_f32(xs, w, b, want_name=True)
    assert name == _walk_of(cout) and torch.equal(got, ops.conv2d_f32(xs, w, b, act=L.ACT_RELU))
    assert torch.equal(got, ops.convnet_conv_f32(xs.contiguous(), w, b))
    # an image's result does not depend on the batch
    assert torch.equal(got[1:], ops.convnet_conv_f32(xs[1:], w, b))


# ---- 2. the general walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(11, 4, 2, 3, 64), (5, 1, 2, 64, 192)], ids=lambda c: "k%d_s%d_p%d_%dto%d" % c)
def test_general_conv_against_fp64(case):
    """|err| <= 1e-6 * (sum|x w| + |b|), the sum in fp64 (the bound of conv2d_f32's test; the ReLU's Lipschitz constant is 1)."""
    k, stride, pad, cin, cout = case
    g = torch.Generator().manual_seed(2100 + k)
    w = (torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)).float()
    b = (0.5 * torch.randn(cout, generator=g)).float()
    wd, bd = flow.pack_conv_weight(w).to(DEV), b.to(DEV)
    for H, W in ((31, 31), (35, 47), (64, 96)):
        x = torch.randn(2, cin, H, W, generator=g)
        want = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad))
        bound = 1e-6 * F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=stride, padding=pad)
        got, name = ops.convnet_conv_f32(nhwc(x), wd, bd, stride=stride, pad=(pad, pad), relu=True, want_name=True)
        assert name == GENERAL and tuple(got.shape) == (2, want.shape[2], want.shape[3], cout)
        ratio = float(((nchw64(got) - want).abs() / bound).max())
        print(f"general conv k{k} s{stride} p{pad} {cin}->{cout} @ 2x{H}x{W}: worst err / bound {ratio:.4f}")
        assert ratio <= 1.0


# ---- 3. prep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lpips", "dists"])
def test_prep(which):
    mul, add, mean, std = (2.0, -1.0, percep.LPIPS_SHIFT, percep.LPIPS_SCALE) if which == "lpips" else \
        (1.0, 0.0, percep.DISTS_MEAN, percep.DISTS_STD)
    g = torch.Generator().manual_seed(7)
    frames = torch.randint(0, 256, (2, 19, 23, 3), generator=g, dtype=torch.uint8)
    frames[0, :, :, 0] = torch.arange(19 * 23).reshape(19, 23) % 256          # every byte value
    u8 = frames.to(DEV).permute(0, 3, 1, 2)                                    # an NCHW view of NHWC frames: strides, no copy
    f32 = (frames.float() / 255.0).to(DEV).permute(0, 3, 1, 2)
    a, b = ops.percep_prep_f32(u8, mul, add, mean, std), ops.percep_prep_f32(f32, mul, add, mean, std)
    assert tuple(a.shape) == (2, 19, 23, 3) and torch.equal(a, b)
    assert torch.equal(ops.percep_prep_f32(f32.contiguous(), mul, add, mean, std), a)
    crop = u8[:, :, 3:17, 2:21]
    assert torch.equal(ops.percep_prep_f32(crop, mul, add, mean, std), a[:, 3:17, 2:21])
    one = ops.percep_prep_f32(u8[:, 1:2], mul, add, mean, std)
    assert torch.equal(one, ops.percep_prep_f32(u8[:, 1:2].expand(-1, 3, -1, -1), mul, add, mean, std))
    # against fp64 from the same fp32 pixel values and the fp32 constants the operator receives: two roundings (the subtraction, the division)
    v = (frames.float() / 255.0).double()
    m32, s32 = torch.tensor(mean, dtype=torch.float32).double(), torch.tensor(std, dtype=torch.float32).double()
    want = ((mul * v + add) - m32) / s32
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(1e-30))) - 23)
    err = float(((a.cpu().double() - want).abs() / ulp).max())
    print(f"prep {which}: worst error {err:.3f} ulp of the result")
    assert err <= 4.0


# ---- 4. / 5. pools ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
def test_maxpool(k, s):
    g = torch.Generator().manual_seed(11)
    for H, W, Cc in ((7, 9, 5), (8, 10, 64), (17, 23, 3), (16, 20, 70), (3, 3, 2)):
        x = torch.randn(2, Cc, H, W, generator=g)
        got = ops.maxpool_f32(nhwc(x), k, s)
        want = F.max_pool2d(x, k, s)
        assert torch.equal(got.cpu().permute(0, 3, 1, 2), want), (H, W, Cc)
    x = torch.randn(1, 4, 9, 9, generator=g)                                   # a NaN is the result of every window that holds it
    x[0, 1, 4, 4] = float("nan")
    got, want = ops.maxpool_f32(nhwc(x), k, s).cpu().permute(0, 3, 1, 2), F.max_pool2d(x, k, s)
    assert bool(want.isnan().any()) and torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))
    wide = nhwc(torch.randn(2, 40, 9, 11, generator=g))
    assert torch.equal(ops.maxpool_f32(wide[..., 8:29], k, s), ops.maxpool_f32(wide[..., 8:29].contiguous(), k, s))


def test_l2pool():
    g = torch.Generator().manual_seed(12)
    for H, W in ((5, 7), (16, 20), (17, 23), (1, 1)):
        x = torch.randn(2, 37, H, W, generator=g)
        x[1, 3] = 0                                                            # an all-zero plane: sqrt(1e-12) everywhere
        got = nchw64(ops.l2pool_f32(nhwc(x)))
        want = R.l2pool_ref(x.double())
        assert got.shape == want.shape
        rel = float(((got - want).abs() / want).max())
        print(f"l2pool @ {H}x{W}: worst relative error {rel:.3e}")
        assert rel <= 1e-6
        assert float((got[1, 3] - 1e-6).abs().max()) <= 1e-12


# ---- 6. the heads ----------------------------------------------------------------------------------------------------------------------
HEAD_SIZES = [(1, 1), (7, 9), (45, 80)]


def _head_features(g, Cc, H, W):
    x, y = torch.randn(3, Cc, H, W, generator=g), torch.randn(3, Cc, H, W, generator=g)
    x[0, :, 0, 0] = 0                                                          # a pixel that is all zeros, in one map and in both
    y[0, :, H - 1, W - 1] = 0
    x[0, :, H - 1, W - 1] = 0
    x[0, Cc - 1] = 0.75                                                        # a constant channel, in one map and in both
    x[2, 0] = -1.5
    y[2, 0] = 0.25
    y[1] = x[1]                                                                # a pair of identical maps
    return x.float(), y.float()


@pytest.mark.parametrize("Cc", [3, 64, 192, 512])
def test_lpips_layer(Cc):
    g = torch.Generator().manual_seed(300 + Cc)
    lin = torch.rand(Cc, generator=g).float() + 0.05
    for H, W in HEAD_SIZES:
        x, y = _head_features(g, Cc, H, W)
        want = R.lpips_head_ref(x.double(), y.double(), lin.double())
        out = torch.zeros(3, dtype=torch.float64, device=DEV)
        xd, yd = nhwc(x), nhwc(y)
        ops.lpips_layer(xd, yd, lin.to(DEV), out)
        err = float((out.cpu() - want).abs().max())
        print(f"lpips_layer C={Cc} @ {H}x{W}: values {out.tolist()}, worst |err| {err:.3e}")
        assert err <= 1e-9 and float(out[1]) == 0.0
        again = torch.zeros_like(out)
        ops.lpips_layer(xd, yd, lin.to(DEV), again)
        assert torch.equal(again, out)
        # a second layer accumulates into out; an image's value does not depend on the batch
        ops.lpips_layer(yd, xd, (2 * lin).to(DEV), out)
        assert float((out.cpu() - 3 * want).abs().max()) <= 1e-9
        solo = torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.lpips_layer(xd[2:], yd[2:], lin.to(DEV), solo)
        assert torch.equal(solo, again[2:])


@pytest.mark.parametrize("Cc", [3, 64, 192, 512])
def test_dists_layer(Cc):
    g = torch.Generator().manual_seed(400 + Cc)
    alpha, beta = torch.rand(Cc, generator=g, dtype=torch.float64) + 0.05, torch.rand(Cc, generator=g, dtype=torch.float64) + 0.05
    tot = alpha.sum() + beta.sum()
    alpha, beta = alpha / tot, beta / tot
    for H, W in HEAD_SIZES:
        x, y = _head_features(g, Cc, H, W)
        x, y = x + 0.5, y + 0.25                                               # means away from zero, as after a ReLU
        y[1] = x[1]
        want = R.dists_head_ref(x.double(), y.double(), alpha, beta)
        out = torch.zeros(3, dtype=torch.float64, device=DEV)
        xd, yd = nhwc(x), nhwc(y)
        ops.dists_layer(xd, yd, alpha.to(DEV), beta.to(DEV), out)
        err = float((out.cpu() - want).abs().max())
        print(f"dists_layer C={Cc} @ {H}x{W}: values {out.tolist()}, worst |err| {err:.3e}")
        assert err <= 1e-9 and abs(float(out[1]) - 1.0) <= 1e-12
        again = torch.zeros_like(out)
        ops.dists_layer(xd, yd, alpha.to(DEV), beta.to(DEV), again)
        assert torch.equal(again, out)
        ops.dists_layer(yd, xd, beta.to(DEV), alpha.to(DEV), out)
        want2 = want + R.dists_head_ref(y.double(), x.double(), beta, alpha)
        assert float((out.cpu() - want2).abs().max()) <= 1e-9
        solo = torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.dists_layer(xd[2:], yd[2:], alpha.to(DEV), beta.to(DEV), solo)
        assert torch.equal(solo, again[2:])


# ---- 7. whole networks -----------------------------------------------------------------------------------------------------------------
NET_SIZES = [(37, 53), (67, 91)]
_STATE = {}


def _state(which):
    if which not in _STATE:
        if which == "dists":
            sd = percep.random_dists_state(21)
            _STATE[which] = (sd, percep.DistsWeights.from_state_dicts(*sd))
        else:
            net = "vgg" if which == "lpips-vgg" else "alex"
            sd = percep.random_lpips_state(21, net)
            _STATE[which] = (sd, percep.LpipsWeights.from_state_dicts(*sd, net))
    return _STATE[which]


def _images(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(9 * xx + 5 * yy), 0.5 + 0.4 * torch.cos(7 * yy * xx + 1), 0.2 + 0.6 * xx * yy])
    ref = (base + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    pred = torch.stack([(ref + s * torch.randn(3, H, W, generator=g)).clamp(0, 1) for s in (0.02, 0.1, 0.3)])
    return pred.float(), ref[None].expand(3, -1, -1, -1).contiguous().float()


def _run(which, W, pred, ref, **kw):
    return percep.dists(W, pred, ref, **kw) if which == "dists" else percep.lpips(W, pred, ref, **kw)


def _ref(which, sd, pred, ref):
    return R.dists_ref(*sd, pred, ref) if which == "dists" else R.lpips_ref(*sd, "vgg" if which == "lpips-vgg" else "alex", pred, ref)


@pytest.mark.parametrize("size", NET_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("which", ["lpips", "lpips-vgg", "dists"])
def test_whole_network_against_the_restatement(which, size):
    """Gate: 20 x the largest deviation of the restatement's own fp32 host run from its fp64 host run over this test's images."""
    sd, W = _state(which)
    pred, ref = _images(*size)
    want = _ref(which, sd, pred.double(), ref.double())
    dev32 = float((_ref(which, sd, pred, ref).double() - want).abs().max())
    got = _run(which, W, pred.to(DEV), ref.to(DEV))
    assert got.dtype == torch.float64 and tuple(got.shape) == (3,)
    err = float((got.cpu() - want).abs().max())
    print(f"{which} @ {size}: values {got.tolist()}, restatement fp32-vs-fp64 deviation {dev32:.3e}, gate {20 * dev32:.3e}, kernels' error {err:.3e}")
    assert err <= 20 * dev32
    assert float(want[0]) < float(want[1]) < float(want[2])                    # more noise scores worse
    # identical images
    same = _run(which, W, ref.to(DEV), ref.to(DEV))
    print(f"{which} @ {size}: identical images -> {same.tolist()}")
    assert (float(same.abs().max()) == 0.0) if which != "dists" else (float(same.abs().max()) <= 1e-9)
    # grouping 1, 2 and 3 frame pairs per trunk batch gives the same bits
    for grp in (1, 2, 3):
        assert torch.equal(_run(which, W, pred.to(DEV), ref.to(DEV), group=grp), got), grp
    # a strided crop view equals its contiguous copy; uint8 frames equal their float form
    big_p, big_r = F.pad(pred, (3, 2, 1, 4)).to(DEV), F.pad(ref, (3, 2, 1, 4)).to(DEV)
    H, Wd = size
    assert torch.equal(_run(which, W, big_p[:, :, 1:1 + H, 3:3 + Wd], big_r[:, :, 1:1 + H, 3:3 + Wd]), got)
    u8p, u8r = (pred * 255).round().to(torch.uint8).to(DEV), (ref * 255).round().to(torch.uint8).to(DEV)
    frames = _run(which, W, u8p.permute(0, 2, 3, 1).contiguous(), u8r.permute(0, 2, 3, 1).contiguous())
    host = lambda t: (t.cpu().float() / 255.0).to(DEV)                         # u / 255 as an IEEE division, formed on the host
    assert torch.equal(frames, _run(which, W, host(u8p), host(u8r)))


def test_too_small_images_are_refused():
    _, W = _state("lpips-vgg")
    x = torch.zeros(1, 3, 15, 40, device=DEV)
    with pytest.raises(ValueError, match="minimum side is 16"):
        percep.lpips(W, x, x)
    _, W = _state("lpips")
    with pytest.raises(ValueError, match="minimum side is 31"):
        percep.lpips(W, torch.zeros(1, 3, 40, 30, device=DEV), torch.zeros(1, 3, 40, 30, device=DEV))
    x = torch.rand(1, 3, 31, 31, device=DEV)
    assert float(percep.lpips(W, x, x)) == 0.0                                  # the minimum itself runs: the last tap is 1 x 1
    _, W = _state("dists")
    x = torch.rand(1, 3, 16, 16, device=DEV)
    assert abs(float(percep.dists(W, x, x))) <= 1e-9


# ---- 8. surfaces -----------------------------------------------------------------------------------------------------------------------
def _clips(seed, F_=3, H=48, W=56):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, 256, (F_, H, W, 3), generator=g, dtype=torch.uint8)
    pred = (gt.int() + torch.randint(-20, 21, gt.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return pred, gt


def test_create_metric_and_clip_metrics():
    _, Wd = _state("dists")
    _, Wl = _state("lpips")
    pred, gt = _clips(5)
    p, r = pred.to(DEV).permute(0, 3, 1, 2).float() / 255.0, gt.to(DEV).permute(0, 3, 1, 2).float() / 255.0
    m = M.create_metric("dists", weights=Wd)
    assert m.lower_better is True
    assert torch.equal(m(p, r), percep.dists(Wd, p, r))
    assert torch.equal(M.create_metric("lpips", weights=Wl)(p.cpu(), r.cpu()), percep.lpips(Wl, p, r))    # host images are moved
    vals = M.clip_metrics(pred, gt, ["psnr", "lpips", "dists"], crop=4, test_y_channel=True, weights={"lpips": Wl, "dists": Wd})
    pc, gc = pred.to(DEV)[:, 4:-4, 4:-4], gt.to(DEV)[:, 4:-4, 4:-4]
    py, gy = M.rgb_to_y(pc), M.rgb_to_y(gc)
    assert tuple(py.shape) == (3, 1, 40, 48)
    assert vals["lpips"] == float(percep.lpips(Wl, py, gy).mean()) and vals["dists"] == float(percep.dists(Wd, py, gy).mean())
    assert vals["psnr"] == M.clip_metrics(pred, gt, ["psnr"], crop=4, test_y_channel=True)["psnr"]
    rgb = M.clip_metrics(pred, gt, ["lpips"], weights={"lpips": Wl})
    assert rgb["lpips"] == float(percep.lpips(Wl, pred.to(DEV), gt.to(DEV)).mean()) and rgb["lpips"] != vals["lpips"]


def test_eval_metrics_command_line(tmp_path):
    from dove_amd import eval_metrics
    gt_dir, pred_dir, wdir = tmp_path / "gt", tmp_path / "pred", tmp_path / "w"
    for d in (gt_dir, pred_dir, wdir):
        d.mkdir()
    (sd_a, lin_a), _ = _state("lpips")
    (sd_v, ab), _ = _state("dists")
    torch.save(sd_a, wdir / "alexnet-owt-7be5be79.pth")
    torch.save(lin_a, wdir / "LPIPS_v0.1_alex-df73285e.pth")
    torch.save(sd_v, wdir / "vgg16-397923af.pth")
    torch.save(ab, wdir / "DISTS_weights-f5e65c96.pth")
    clips = {"a": _clips(1), "b": _clips(2)}
    for name, (pred, gt) in clips.items():
        np.save(gt_dir / f"{name}.npy", gt.numpy())
        np.save(pred_dir / f"{name}.npy", pred.numpy())
    out = eval_metrics.main(["--gt", str(gt_dir), "--pred", str(pred_dir), "--out", str(tmp_path), "--metrics", "psnr,lpips,dists",
                             "--metric_weights", str(wdir)])
    Wl, Wd = percep.load_metric_weights(str(wdir), "lpips"), percep.load_metric_weights(str(wdir), "dists")
    want = {}
    for name, (pred, gt) in clips.items():
        want[name] = {"psnr": round(M.clip_metrics(pred, gt, ["psnr"])["psnr"], 4),
                      "lpips": round(float(percep.lpips(Wl, pred.to(DEV), gt.to(DEV)).mean()), 4),
                      "dists": round(float(percep.dists(Wd, pred.to(DEV), gt.to(DEV)).mean()), 4)}
    with open(tmp_path / "metrics_psnr_lpips_dists.json") as f:
        on_disk = json.load(f)
    assert on_disk == out and out["count"] == 2 and out["per_sample"] == want
    assert out["average"] == {k: round(float(np.mean([want[n][k] for n in want])), 4) for k in ("psnr", "lpips", "dists")}
    assert all(want[n]["lpips"] > 0 and 0 < want[n]["dists"] < 1 for n in want)


# ---- 9. the fast walk is no slower than the kernel it replaces ------------------------------------------------------------------------
def test_fast_conv_is_not_slower_than_conv_f32_kernel():
    """256 -> 256 at 2 x 180 x 320: the median of 10 launches after warm-up, each bracketed by synchronisations, on both kernels."""
    g = torch.Generator().manual_seed(9)
    x = nhwc(torch.randn(2, 256, 180, 320, generator=g))
    w = flow.pack_conv_weight(torch.randn(256, 256, 3, 3, generator=g) / 48.0).to(DEV)
    b = torch.zeros(256, device=DEV)
    out = torch.empty(2, 180, 320, 256, device=DEV)

    def median_ms(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2]

    assert ops.convnet_conv_kernel_name(tuple(x.shape), tuple(w.shape)) == FAST
    # the one VGG16 shape on which the fast walk loses (docs/kernels.md) stays on conv_f32_kernel
    assert ops.convnet_conv_kernel_name((2, 720, 1280, 64), (3, 3, 64, 64)) == GENERAL
    fast = median_ms(lambda: ops.convnet_conv_f32(x, w, b, out=out))
    general = median_ms(lambda: ops.conv2d_f32(x, w, b, act=L.ACT_RELU, out=out))
    flop = 2.0 * 2 * 180 * 320 * 256 * 256 * 9
    print(f"256->256 @ 2x180x320: convnet3x3_f32_kernel {fast:.3f} ms ({flop / fast / 1e9:.1f} TFLOP/s), "
          f"conv_f32_kernel {general:.3f} ms ({flop / general / 1e9:.1f} TFLOP/s)")
    assert fast <= general
