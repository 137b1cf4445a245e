"""CLIP-IQA on the GPU (csrc/clipiqa.hip, dove_amd/clipiqa.py): the tower's conv entry bit for bit against the general walk of
dove_convnet_conv_f32 with pool, residual and ReLU applied as exact fp32 torch ops, the attention pool against the full attention of the
fp64 restatement (tests/clipiqa_ref.py) with the gate taken from the restatement's own fp32-vs-fp64 deviation, the score in fp64, the whole
network against the restatement, and the surfaces."""
import json
import math
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clipiqa_ref as R
import test_clipiqa_cpu as T
from dove_amd import clipiqa as Q
from dove_amd import flow, ops
from dove_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
POINTWISE, N64, FAST, GENERAL = "pointwise_f32_kernel", "convnet3x3_n64_f32_kernel", "convnet3x3_f32_kernel", "conv_f32_kernel"
AP_SLICE = 256                                  # tokens per reduction slice of the attention pool (csrc/clipiqa.hip)
_CACHE = {}


def nhwc(t):            # [N,C,H,W] host -> channels-last float32 on the device
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def nchw64(t):          # channels-last device tensor -> [N,C,H,W] host fp64
    return t.detach().cpu().double().permute(0, 3, 1, 2)


def pool2(x):           # the 2 x 2 average of a channels-last tensor in the kernels' order, exact fp32 ops on the device
    H2, W2 = x.shape[1] // 2 * 2, x.shape[2] // 2 * 2
    a, b, c, d = x[:, 0:H2:2, 0:W2:2], x[:, 0:H2:2, 1:W2:2], x[:, 1:H2:2, 0:W2:2], x[:, 1:H2:2, 1:W2:2]
    return (((a + b) + (c + d)) * 0.25).contiguous()


def weights():
    if "W" not in _CACHE:
        _CACHE["W"] = Q.ClipIqaWeights.from_state_dict(*T.state())
    return _CACHE["W"]


# ---- 1. pointwise_f32_kernel: the bits of conv_f32_kernel -------------------------------------------------------------------------------
POINTWISE_CASES = [(64, 256), (256, 64), (2048, 512), (32, 20)]           # the last: ragged N, cout % 4 == 0 only
POINTWISE_SIZES = [(2, 5, 7), (1, 13, 21), (2, 16, 16)]                   # M below one tile; odd H and W; M a multiple of the tile


@pytest.mark.parametrize("case", POINTWISE_CASES, ids=lambda c: "%dto%d" % c)
def test_pointwise_is_bit_identical_to_the_general_walk(case):
    cin, cout = case
    g = torch.Generator().manual_seed(3000 + cin + cout)
    w = flow.pack_conv_weight(torch.randn(cout, cin, 1, 1, generator=g) / math.sqrt(cin)).to(DEV)
    b = (0.1 * torch.randn(cout, generator=g)).to(DEV)
    for N, H, Wd in POINTWISE_SIZES:
        x = nhwc(torch.randn(N, cin, H, Wd, generator=g))
        for pool in (1, 2):
            xin = pool2(x) if pool == 2 else x
            base = ops.convnet_conv_f32(xin, w, b, pad=(0, 0), relu=False)                 # acc + bias on conv_f32_kernel
            assert ops.convnet_conv_kernel_name(tuple(xin.shape), tuple(w.shape), pad=(0, 0)) == GENERAL
            res = torch.randn(base.shape, generator=g).to(DEV)
            for residual, relu in ((None, False), (None, True), (res, False), (res, True)):
                want = base if residual is None else base + residual
                want = want.clamp_min(0) if relu else want
                got, name = ops.resnet_conv_f32(x, w, b, pool=pool, residual=residual, relu=relu, want_name=True)
                assert name == POINTWISE, (case, N, H, Wd, pool, name)
                assert tuple(got.shape) == (N, H // pool, Wd // pool, cout)
                assert torch.equal(got, want), (case, N, H, Wd, pool, residual is not None, relu,
                                                float((got - want).abs().max()))
            # the sum written over the identity, as the tower does it
            ident = res.clone()
            assert ops.resnet_conv_f32(x, w, b, pool=pool, residual=ident, out=ident).data_ptr() == ident.data_ptr()
            assert torch.equal(ident, (base + res).clamp_min(0))
        # x, residual and out as channel slices of wider buffers; the bytes outside out's slice stay
        wide = nhwc(torch.randn(N, cin + 32, H, Wd, generator=g))
        xs = wide[..., 32:]
        base = ops.convnet_conv_f32(xs.contiguous(), w, None, pad=(0, 0), relu=False)
        rbuf = torch.randn(N, H, Wd, cout + 7, generator=g).to(DEV)
        obuf = torch.randn(N, H, Wd, cout + 12, generator=g).to(DEV)
        before = obuf.clone()
        got, name = ops.resnet_conv_f32(xs, w, None, residual=rbuf[..., 3:3 + cout], relu=True, out=obuf[..., 8:8 + cout], want_name=True)
        assert name == POINTWISE and torch.equal(got, (base + rbuf[..., 3:3 + cout]).clamp_min(0))
        keep = torch.ones(cout + 12, dtype=torch.bool)
        keep[8:8 + cout] = False
        assert torch.equal(obuf[..., keep.to(DEV)], before[..., keep.to(DEV)]), "bytes outside the written slice changed"
        # an image's result does not depend on the batch
        if N > 1:
            assert torch.equal(ops.resnet_conv_f32(x, w, b)[1:], ops.resnet_conv_f32(x[1:], w, b))


# ---- 2. the 3 x 3 walks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(32, 32), (32, 64), (64, 64)], ids=lambda c: "%dto%d" % c)
def test_n64_conv_is_bit_identical_to_the_general_walk(case):
    cin, cout = case
    g = torch.Generator().manual_seed(3100 + cin + cout)
    w = flow.pack_conv_weight(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).to(DEV)
    b = (0.1 * torch.randn(cout, generator=g)).to(DEV)
    for H, Wd in ((1, 1), (1, 3), (9, 11), (17, 16)):
        x = nhwc(torch.randn(2, cin, H, Wd, generator=g))
        base, yard = ops.convnet_conv_f32(x, w, b, relu=False, want_name=True)
        assert yard == GENERAL
        for relu in (False, True):
            got, name = ops.resnet_conv_f32(x, w, b, relu=relu, want_name=True)
            assert name == N64, (case, H, Wd, name)
            assert torch.equal(got, base.clamp_min(0) if relu else base), (case, H, Wd, relu)
    wide = nhwc(torch.randn(2, cin + 32, 9, 11, generator=g))
    got, name = ops.resnet_conv_f32(wide[..., 32:], w, b, want_name=True)
    assert name == N64 and torch.equal(got, ops.convnet_conv_f32(wide[..., 32:], w, b))


def test_wide_3x3_runs_on_the_existing_fast_kernel():
    g = torch.Generator().manual_seed(3200)
    for cin, cout in ((64, 128), (128, 132)):
        w = flow.pack_conv_weight(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).to(DEV)
        b = (0.1 * torch.randn(cout, generator=g)).to(DEV)
        x = nhwc(torch.randn(2, cin, 17, 23, generator=g))
        want, yard = ops.convnet_conv_f32(x, w, b, relu=True, want_name=True)
        got, name = ops.resnet_conv_f32(x, w, b, relu=True, want_name=True)
        assert yard == FAST and name == FAST and torch.equal(got, want)
    assert ops.resnet_conv_kernel_name((2, 180, 320, 512), (3, 3, 512, 512)) == FAST
    assert ops.convnet_conv_kernel_name((2, 180, 320, 64), (3, 3, 64, 64)) == GENERAL       # dove_convnet_conv_f32's dispatch is as it was


@pytest.mark.parametrize("size", [(32, 48), (31, 31), (35, 47)], ids=lambda s: "%dx%d" % s)
def test_stem_conv_against_fp64(size):
    """3 -> 32, stride 2, on the general walk: |err| <= 1e-6 * (sum|x w| + |b|), the sum in fp64 (the bound of
    tests/test_percep_gpu.py's test_general_conv_against_fp64)."""
    H, Wd = size
    g = torch.Generator().manual_seed(3300 + H)
    w = (torch.randn(32, 3, 3, 3, generator=g) / math.sqrt(27)).float()
    b = (0.5 * torch.randn(32, generator=g)).float()
    x = torch.randn(2, 3, H, Wd, generator=g)
    want = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1))
    bound = 1e-6 * F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2, padding=1)
    got, name = ops.resnet_conv_f32(nhwc(x), flow.pack_conv_weight(w).to(DEV), b.to(DEV), stride=2, relu=True, want_name=True)
    assert name == GENERAL and tuple(got.shape) == (2, want.shape[2], want.shape[3], 32)
    ratio = float(((nchw64(got) - want).abs() / bound).max())
    print(f"stem conv @ 2x{H}x{Wd}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0


def test_conv_refusals_and_fallbacks():
    g = torch.Generator().manual_seed(3400)
    x = nhwc(torch.randn(1, 32, 8, 8, generator=g))
    w3 = flow.pack_conv_weight(torch.randn(32, 32, 3, 3, generator=g)).to(DEV)
    with pytest.raises(RuntimeError, match="pool 2 belongs to a 1 x 1 conv"):
        ops.resnet_conv_f32(x, w3, None, pool=2)
    assert ops.resnet_conv_kernel_name((1, 8, 8, 32), (3, 3, 32, 32), pool=2) == ""
    with pytest.raises(RuntimeError, match="residual need pointwise_f32_kernel"):
        ops.resnet_conv_f32(x, w3, None, residual=torch.zeros(1, 8, 8, 32, device=DEV))
    # k = 1 with cin % 32 != 0 falls to the general walk; with pool 2 or a residual it is refused
    x48 = nhwc(torch.randn(2, 48, 9, 11, generator=g))
    w48 = flow.pack_conv_weight(torch.randn(64, 48, 1, 1, generator=g) / 7.0).to(DEV)
    got, name = ops.resnet_conv_f32(x48, w48, None, relu=False, want_name=True)
    assert name == GENERAL and torch.equal(got, ops.convnet_conv_f32(x48, w48, None, pad=(0, 0), relu=False))
    assert ops.resnet_conv_kernel_name((2, 9, 11, 48), (1, 1, 48, 64), pool=2) == ""
    with pytest.raises(RuntimeError, match="need pointwise_f32_kernel"):
        ops.resnet_conv_f32(x48, w48, None, pool=2)
    with pytest.raises(RuntimeError, match="need pointwise_f32_kernel"):
        ops.resnet_conv_f32(x48, w48, None, residual=torch.zeros(2, 9, 11, 64, device=DEV))
    # a slice that breaks the 16-byte alignment of x takes the general walk too, with the same bits
    wide = nhwc(torch.randn(2, 66, 9, 11, generator=g))
    w64 = flow.pack_conv_weight(torch.randn(64, 64, 1, 1, generator=g) / 8.0).to(DEV)
    got, name = ops.resnet_conv_f32(wide[..., 1:65], w64, None, want_name=True)
    assert name == GENERAL and torch.equal(got, ops.resnet_conv_f32(wide[..., 1:65].contiguous(), w64, None))
    with pytest.raises(ValueError, match="too small for pool"):
        ops.resnet_conv_f32(nhwc(torch.zeros(1, 64, 1, 8)), w64, None, pool=2)


# ---- 3. avgpool --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(2, 2), (7, 9), (16, 21)], ids=lambda s: "%dx%d" % s)
def test_avgpool(size):
    H, Wd = size
    g = torch.Generator().manual_seed(3500 + H)
    x = nhwc(torch.randn(2, 40, H, Wd, generator=g))
    got = ops.avgpool_cl_f32(x)
    assert tuple(got.shape) == (2, H // 2, Wd // 2, 40) and torch.equal(got, pool2(x))
    xs = x[..., 5:29]                                                          # a channel slice in, a channel slice out
    buf = torch.randn(2, H // 2, Wd // 2, 30, generator=g).to(DEV)
    before = buf.clone()
    ops.avgpool_cl_f32(xs, out=buf[..., 2:26])
    assert torch.equal(buf[..., 2:26], pool2(xs.contiguous()))
    assert torch.equal(buf[..., :2], before[..., :2]) and torch.equal(buf[..., 26:], before[..., 26:])
    with pytest.raises(ValueError, match="smaller than the window"):
        ops.avgpool_cl_f32(x[:, :1].contiguous())


# ---- 4. the attention pool ---------------------------------------------------------------------------------------------------------------
def _attn_feat(h, w, seed, n=3):
    g = torch.Generator().manual_seed(seed)
    return F.relu(torch.randn(n, 2048, h, w, generator=g) * 0.7 + 0.2).float()


def _attn_check(feat, what):
    """The embedding against the restatement's full attention in fp64; gate: 20 x the restatement's own fp32-vs-fp64 deviation."""
    sd, _ = T.state()
    want = R.attnpool(sd, feat.double())
    dev32 = float((R.attnpool(sd, feat).double() - want).abs().max())
    got = ops.clip_attnpool_f32(nhwc(feat), weights().to(DEV).attn)
    assert got.dtype == torch.float32 and tuple(got.shape) == (feat.shape[0], 1024) and bool(torch.isfinite(got).all())
    err = float((got.cpu().double() - want).abs().max())
    print(f"attnpool {what}: |e| max {float(want.abs().max()):.3f}, restatement fp32-vs-fp64 deviation {dev32:.3e}, gate {20 * dev32:.3e}, "
          f"kernels' error {err:.3e}")
    assert err <= 20 * dev32
    return got


@pytest.mark.parametrize("hw", [(1, 1), (1, 3), (3, 5), (AP_SLICE // 16 + 1, 16)], ids=lambda s: "%dx%d" % s)
def test_attnpool_against_full_attention(hw):
    """1 x 1: two identical tokens; the last map has more tokens than one reduction slice, so the merge over slices runs."""
    h, w = hw
    assert (h * w > AP_SLICE) == (hw == (AP_SLICE // 16 + 1, 16))
    feat = _attn_feat(h, w, 3600 + h * w)
    got = _attn_check(feat, f"{h}x{w}")
    # image k alone has the bits of image k in the batch; a channel slice of a wider map has the bits of its copy
    x = nhwc(feat)
    proj = weights().to(DEV).attn
    for k in range(3):
        assert torch.equal(ops.clip_attnpool_f32(x[k:k + 1], proj)[0], got[k]), k
    wide = torch.zeros(3, h, w, 2048 + 8, device=DEV)
    wide[..., 8:] = x
    assert torch.equal(ops.clip_attnpool_f32(wide[..., 8:], proj), got)
    assert torch.equal(ops.clip_attnpool_f32(x, proj), got)                    # and twice gives the same bits


def test_attnpool_softmax_range():
    """A map scaled until the pre-softmax scores reach +-60 stays finite and inside the same gate."""
    sd, _ = T.state()
    feat = _attn_feat(3, 5, 3700) - 0.4                                        # both signs, so that the scores spread both ways
    for _ in range(3):                                                         # the scores are not exactly quadratic in the map's scale
        s = R.attnpool(sd, feat.double(), want_scores=True)[:, :, 0]
        feat = feat * math.sqrt(66.0 / float(s.abs().max()))
    s = R.attnpool(sd, feat.double(), want_scores=True)[:, :, 0]
    print(f"scores of the query token: min {float(s.min()):.1f}, max {float(s.max()):.1f}")
    assert float(s.abs().max()) >= 60.0
    _attn_check(feat, "3x5 scaled")


# ---- 5. the score -------------------------------------------------------------------------------------------------------------------------
def test_clipiqa_score():
    g = torch.Generator().manual_seed(3800)
    emb = torch.randn(7, 1024, generator=g)
    pos = torch.randn(5, 1024, generator=g, dtype=torch.float64)
    neg = pos + 0.3 * torch.randn(5, 1024, generator=g, dtype=torch.float64)
    text = torch.stack([pos, neg], dim=1).reshape(10, 1024)
    text = text / text.norm(dim=1, keepdim=True)
    got = ops.clipiqa_score(emb.to(DEV), text.to(DEV), 100.0)
    want = R.score(emb.double(), text, 100.0)
    err = float((got.cpu() - want).abs().max())
    print(f"clipiqa_score: values {got.tolist()}, error {err:.3e}")
    assert got.dtype == torch.float64 and err <= 1e-12 and 0.01 < float(want.min()) and float(want.max()) < 0.99
    same = torch.stack([pos, pos], dim=1).reshape(10, 1024)
    same = same / same.norm(dim=1, keepdim=True)
    assert ops.clipiqa_score(emb.to(DEV), same.to(DEV), 100.0).tolist() == [0.5] * 7
    one = ops.clipiqa_score(emb[:1].to(DEV), text[:2].to(DEV), 100.0)          # one pair
    assert abs(float(one) - float(R.score(emb[:1].double(), text[:2], 100.0))) <= 1e-12
    with pytest.raises(ValueError, match="float64"):
        ops.clipiqa_score(emb.to(DEV), text[:3].to(DEV), 100.0)


# ---- 6. the whole network ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", T.NET_SIZES, ids=lambda s: "%dx%d" % s)
def test_whole_network_against_the_restatement(size):
    """Gates: 20 x the deviation of the restatement's own fp32 host run from its fp64 host run over this test's images, on the score and on
    the normalised embedding (which cannot saturate)."""
    sd, text = T.state()
    W = weights()
    pred = T.images(*size)
    want, f_want, _ = R.clipiqa_ref(sd, text, pred.double(), want_parts=True)
    s32, f32, _ = R.clipiqa_ref(sd, text, pred, want_parts=True)
    dev_s, dev_f = float((s32.double() - want).abs().max()), float((f32.double() - f_want).abs().max())
    got, emb = Q.clipiqa(W, pred.to(DEV), want_embedding=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3,) and tuple(emb.shape) == (3, 1024)
    f_got = emb.cpu().double()
    f_got = f_got / f_got.norm(dim=1, keepdim=True)
    err_s, err_f = float((got.cpu() - want).abs().max()), float((f_got - f_want).abs().max())
    print(f"clipiqa @ {size}: values {got.tolist()}; score: restatement fp32-vs-fp64 deviation {dev_s:.3e}, gate {20 * dev_s:.3e}, kernels' "
          f"error {err_s:.3e}; embedding: deviation {dev_f:.3e}, gate {20 * dev_f:.3e}, kernels' error {err_f:.3e}")
    assert err_s <= 20 * dev_s
    assert err_f <= 20 * dev_f
    # grouping 1, 2 and 3 frames per tower batch gives the same bits
    for grp in (1, 2, 3):
        assert torch.equal(Q.clipiqa(W, pred.to(DEV), group=grp), got), grp
    # a strided crop view equals its contiguous copy; uint8 frames equal their float form
    H, Wd = size
    big = F.pad(pred, (3, 2, 1, 4)).to(DEV)
    assert torch.equal(Q.clipiqa(W, big[:, :, 1:1 + H, 3:3 + Wd]), got)
    u8 = (pred * 255).round().to(torch.uint8).to(DEV)
    frames = Q.clipiqa(W, u8.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(frames, Q.clipiqa(W, (u8.cpu().float() / 255.0).to(DEV)))            # u / 255 as an IEEE division, formed on the host
    # one channel is repeated
    assert torch.equal(Q.clipiqa(W, pred[:, :1].to(DEV)), Q.clipiqa(W, pred[:, :1].expand(-1, 3, -1, -1).contiguous().to(DEV)))


def test_sizes_too_small_and_full_frame():
    W = weights()
    with pytest.raises(ValueError, match="minimum side is 31"):
        Q.clipiqa(W, torch.zeros(1, 3, 40, 30, device=DEV))
    with pytest.raises(TypeError, match="ClipIqaWeights"):
        Q.clipiqa(object(), torch.zeros(1, 3, 40, 40, device=DEV))
    frame = F.interpolate(T.images(90, 160)[1:2], size=(720, 1280), mode="bilinear").clamp(0, 1)
    v = Q.clipiqa(W, frame.to(DEV))
    print(f"one 720 x 1280 frame: {v.tolist()}")
    assert tuple(v.shape) == (1,) and 0.0 < float(v) < 1.0


# ---- 7. surfaces -------------------------------------------------------------------------------------------------------------------------
def _clips(seed, F_=3, H=48, W=56):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, 256, (F_, H, W, 3), generator=g, dtype=torch.uint8)
    pred = (gt.int() + torch.randint(-20, 21, gt.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return pred, gt


def _weights_dir(path):
    sd, text = T.state()
    path.mkdir()
    torch.save(sd, path / "RN50.pth")
    Q.save_text(str(path / "clipiqa_text.npz"), text["features"], text["prompts"], text["logit_scale"])
    return str(path)


def test_create_metric_and_clip_metrics():
    W = weights()
    pred, gt = _clips(5)
    p = pred.to(DEV).permute(0, 3, 1, 2).float() / 255.0
    m = M.create_metric("clipiqa", weights=W)
    assert m.lower_better is False
    want = Q.clipiqa(W, p)
    assert torch.equal(m(p), want) and torch.equal(m(p.cpu()), want)            # host images are moved
    assert torch.equal(m.to(DEV).eval()(p[0]), want[:1])                         # one [C,H,W] image
    vals = M.nr_clip_metrics(pred, ["clipiqa"], {"clipiqa": W})
    assert vals == {"clipiqa": float(Q.clipiqa(W, pred.to(DEV)).mean())}
    # beside a full-reference metric, clipiqa sees the prediction as it is: no crop, no y channel
    both = M.clip_metrics(pred, gt, ["psnr", "clipiqa"], crop=4, test_y_channel=True, weights={"clipiqa": W})
    assert both["clipiqa"] == vals["clipiqa"] and both["psnr"] == M.clip_metrics(pred, gt, ["psnr"], crop=4, test_y_channel=True)["psnr"]
    assert both["clipiqa"] != float(Q.clipiqa(W, pred.to(DEV)[:, 4:-4, 4:-4]).mean())


def test_eval_metrics_command_line(tmp_path, capsys):
    from dove_amd import eval_metrics
    gt_dir, pred_dir = tmp_path / "gt", tmp_path / "pred"
    gt_dir.mkdir()
    pred_dir.mkdir()
    wdir = _weights_dir(tmp_path / "w")
    clips = {"a": _clips(1), "b": _clips(2)}
    for name, (pred, gt) in clips.items():
        np.save(gt_dir / f"{name}.npy", gt.numpy())
        np.save(pred_dir / f"{name}.npy", pred.numpy())
    W = Q.ClipIqaWeights.load(wdir)
    want = {n: round(float(Q.clipiqa(W, p.to(DEV)).mean()), 4) for n, (p, _) in clips.items()}
    # the VideoLQ line: no ground truth
    out = eval_metrics.main(["--pred", str(pred_dir), "--out", str(tmp_path / "nr"), "--metrics", "clipiqa", "--metric_weights", wdir])
    with open(tmp_path / "nr" / "metrics_clipiqa.json") as f:
        assert json.load(f) == out
    assert out["count"] == 2 and out["per_sample"] == {n: {"clipiqa": v} for n, v in want.items()}
    assert out["average"] == {"clipiqa": round(float(np.mean(list(want.values()))), 4)} and want["a"] != want["b"]
    # with ground truth and a crop: clipiqa sees the uncropped prediction
    out = eval_metrics.main(["--gt", str(gt_dir), "--pred", str(pred_dir), "--out", str(tmp_path / "fr"), "--metrics", "psnr,clipiqa",
                             "--crop", "4", "--metric_weights", wdir])
    assert {n: v["clipiqa"] for n, v in out["per_sample"].items()} == want
    assert all(v["psnr"] == round(M.clip_metrics(*clips[n], ["psnr"], crop=4)["psnr"], 4) for n, v in out["per_sample"].items())
    assert os.path.exists(tmp_path / "fr" / "metrics_psnr_clipiqa.json")
    # without the weights the metric fails to initialise with the usual message, and the others go on
    capsys.readouterr()
    out = eval_metrics.main(["--gt", str(gt_dir), "--pred", str(pred_dir), "--out", str(tmp_path / "no"), "--metrics", "psnr,clipiqa"])
    assert "Failed to initialize metric 'clipiqa'" in capsys.readouterr().out and set(out["average"]) == {"psnr"}


def test_score_command_line(tmp_path, capsys):
    from PIL import Image
    wdir = _weights_dir(tmp_path / "w")
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    pred, _ = _clips(7, F_=2)
    for i in range(2):
        Image.fromarray(pred[i].numpy()).save(img_dir / f"f{i}.png")
    scores = Q.main(["score", "--pred", str(img_dir), "--metric_weights", wdir])
    want = Q.clipiqa(weights(), pred.to(DEV))
    assert scores == {"f0.png": float(want[0]), "f1.png": float(want[1])} and "average:" in capsys.readouterr().out


def test_cli_eval_metrics_clipiqa_without_gt_dir(golden_dir, tmp_path, capsys):
    """The inference command line accepts clipiqa and scores its own output without ground truth (16 x 16 in, 64 x 64 out)."""
    from dove_amd import cli
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    wdir = _weights_dir(tmp_path / "w")
    np.save(inp / "clip0.npy", np.random.default_rng(5).integers(0, 256, size=(5, 16, 16, 3), dtype=np.uint8))
    emb = os.path.join(golden_dir, "empty_prompt_embedding.safetensors")
    cli.main(["--input_dir", str(inp), "--random_init", "--num_layers", "1", "--prompt_embedding", emb, "--output_path", str(out),
              "--eval_metrics", "clipiqa", "--metric_weights", wdir])
    res = np.load(out / "clip0.npy")
    assert res.shape == (5, 64, 64, 3)
    with open(out / "metrics_clipiqa.json") as f:
        js = json.load(f)
    want = float(Q.clipiqa(weights(), torch.from_numpy(res)).mean())
    assert js["count"] == 1 and js["per_sample"]["clipiqa"] == [want] and js["average"]["clipiqa"] == want and 0.0 < want < 1.0
    assert "[clip0.npy] CLIPIQA=" in capsys.readouterr().out


# ---- 8. the new walks are no slower than the kernel they replace --------------------------------------------------------------------------
def _median_ms(fn):
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


@pytest.mark.parametrize("k,cin,want", [(1, 256, POINTWISE), (3, 64, N64)], ids=["pointwise", "n64"])
def test_new_walks_are_not_slower_than_conv_f32_kernel(k, cin, want):
    """cin -> 64 at 1 x 180 x 320: the median of 10 launches after warm-up, each bracketed by synchronisations, on both kernels (the method
    of tests/test_percep_gpu.py's test_fast_conv_is_not_slower_than_conv_f32_kernel)."""
    g = torch.Generator().manual_seed(9)
    x = nhwc(torch.randn(1, cin, 180, 320, generator=g))
    w = flow.pack_conv_weight(torch.randn(64, cin, k, k, generator=g) / math.sqrt(k * k * cin)).to(DEV)
    b = torch.zeros(64, device=DEV)
    out = torch.empty(1, 180, 320, 64, device=DEV)
    assert ops.resnet_conv_kernel_name(tuple(x.shape), tuple(w.shape)) == want
    assert ops.convnet_conv_kernel_name(tuple(x.shape), tuple(w.shape), pad=(k // 2, k // 2)) == GENERAL
    new = _median_ms(lambda: ops.resnet_conv_f32(x, w, b, out=out))
    general = _median_ms(lambda: ops.convnet_conv_f32(x, w, b, pad=(k // 2, k // 2), out=out))
    flop = 2.0 * 180 * 320 * cin * 64 * k * k
    print(f"{cin}->64 k{k} @ 1x180x320: {want} {new:.3f} ms ({flop / new / 1e9:.1f} TFLOP/s), conv_f32_kernel {general:.3f} ms "
          f"({flop / general / 1e9:.1f} TFLOP/s)")
    assert new <= general
