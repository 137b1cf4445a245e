"""MUSIQ on the GPU (csrc/musiq.hip, dove_amd/musiq.py): every new kernel against fp64 (the patch gather to one fp32 ulp of the fp64
restatement, the others inside 20 x the deviation of torch's own fp32 run from fp64 on the same inputs), the Linears bit for bit against
the general conv walk, the whole network against the restatement (tests/musiq_ref.py), the production token count, and the surfaces."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import musiq_ref as R
import test_musiq_cpu as T
from dove_amd import metrics as M
from dove_amd import musiq as Q
from dove_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory():
    """This module keeps two sets of weights (125 MB each) and the token tables on the device and allocates odd-sized activations (the
    64 KiB-per-token maps of a 720 x 1280 frame).  Left alive, the weights pin their segments for the rest of the session, and the freed
    blocks stay in torch's caching allocator, where a later request that almost fits takes a whole block; tests that compare peak allocated
    bytes (the streaming tool's bounded-memory test) then see this module's leftovers.  Drop the tensors and hand the blocks back when the
    module is done."""
    live = torch.cuda.memory_allocated()
    yield
    import gc
    _CACHE.clear()
    for geo in Q._GEOMETRY.values():
        geo["device"].clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert torch.cuda.memory_allocated() <= live, "this module left tensors on the device"


def weights(num_classes=1):
    if num_classes not in _CACHE:
        _CACHE[num_classes] = Q.MusiqWeights.from_state_dict(T.state(num_classes))
    return _CACHE[num_classes]


def gate_check(what, got, want64, torch32):
    """``got`` (device fp32) against ``want64`` inside 20 x the deviation of ``torch32`` (torch's own fp32 result) from ``want64``."""
    dev = float((torch32.double() - want64).abs().max())
    err = float((got.detach().cpu().double() - want64).abs().max())
    print(f"{what}: fp32-vs-fp64 deviation {dev:.3e}, gate {20 * dev:.3e}, kernel's error {err:.3e}")
    assert math.isfinite(err) and err <= 20 * dev, what                  # a single key (T = 1) has deviation 0 and must have error 0
    return err


# ---- 1. the patch gather ----------------------------------------------------------------------------------------------------------------
GATHER_SIZES = [(32, 32), (33, 47), (70, 45), (64, 96), (5, 300), (1, 1), (225, 385)]


# The fp64 restatement is itself a rounded evaluation: a 16-tap sum with sum |cy| sum |cx| <= 2.6 and |v'| <= 1 carries up to about 32
# roundings of 2^-53 * 2.6 = 1e-14, on either side.  Where the exact value is 0 (a resized pixel that falls on a source pixel with
# v = 0.5, which bf16 inputs hit) both results are such noise of either sign, and one fp32 ulp of noise is no criterion; there, and only
# there, the allowance below is wider than the ulp.
FP64_NOISE = 5e-14


def _within_one_ulp(got, want64):
    w = want64.float()
    lo, hi = torch.nextafter(w, torch.full_like(w, -math.inf)), torch.nextafter(w, torch.full_like(w, math.inf))
    return bool((((got >= lo) & (got <= hi)) | ((got.double() - want64).abs() <= FP64_NOISE)).all())


def _gather_case(view_dev, img64, what):
    """``view_dev``: the [N,C,H,W] view handed to the kernel; ``img64``: the same values as a host fp64 [N,C,H,W] tensor."""
    N, _, H, W = img64.shape
    geo = Q.token_geometry(H, W)
    want, spatial, scale, _ = R.multiscale_patches(img64, padded=False)                      # [N,L,3,32,32]
    pad = R.multiscale_patches(torch.ones_like(img64), padded=False)[0] == 0                 # the zero padding: 2 * 1 - 1 resizes to about 1
    got, geo2 = Q.patches(view_dev)
    assert geo2 is geo and tuple(got.shape) == (N * (geo["length"] - 1), 32, 32, 3), what
    assert geo["tokens"][:, 0].tolist() == scale.tolist() and geo["tokens"][:, 3].tolist() == spatial.tolist()
    g = got.cpu().view(N, -1, 32, 32, 3).permute(0, 1, 4, 2, 3)
    assert _within_one_ulp(g, want), (what, float((g.double() - want).abs().max()))
    assert bool((g[pad] == 0).all()) and bool((want[pad] == 0).all()), what
    framed = Q.patches(view_dev, Q.STEM_BEFORE, Q.STEM_SIDE)[0]                              # the stem conv's frame: 2 zeros before, 3 after
    assert torch.equal(framed[:, 2:34, 2:34], got), what
    border = framed.clone()
    border[:, 2:34, 2:34] = 0
    assert not bool(border.any()), what
    return got


@pytest.mark.parametrize("size", GATHER_SIZES, ids=lambda s: "%dx%d" % s)
def test_patch_gather(size):
    H, W = size
    g = torch.Generator().manual_seed(4000 + 7 * H + W)
    img = torch.rand(2, 3, H, W, generator=g)
    _gather_case(img.to(DEV), img.double(), "f32")
    u8 = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    _gather_case(u8.to(DEV).permute(0, 3, 1, 2), u8.permute(0, 3, 1, 2).double() / 255.0, "u8 frames")
    bf = img.bfloat16()
    _gather_case(bf.to(DEV), bf.double(), "bf16")
    big = torch.rand(2, H + 5, W + 3, 3, generator=g)                                        # a cropped and permuted view
    _gather_case(big.to(DEV)[:, 2:2 + H, 1:1 + W].permute(0, 3, 1, 2), big[:, 2:2 + H, 1:1 + W].permute(0, 3, 1, 2).double(), "crop")
    one = _gather_case(img[:, :1].to(DEV), img[:, :1].double(), "one channel")
    assert torch.equal(one, Q.patches(img[:, :1].expand(-1, 3, -1, -1).contiguous().to(DEV))[0])
    assert torch.equal(Q.patches(img[1:].to(DEV))[0], Q.patches(img.to(DEV))[0][Q.token_geometry(H, W)["length"] - 1:])   # batch-independent


# ---- 2. GroupNorm -----------------------------------------------------------------------------------------------------------------------
GN_SHAPES = [(16, 64), (8, 64), (8, 256)]


def _gn64(x, gamma, beta, eps, dtype=torch.float64):
    return F.group_norm(x.to(dtype).permute(0, 3, 1, 2), 32, gamma.to(dtype), beta.to(dtype), eps)


def _pool(t):
    return F.max_pool2d(F.pad(t, (0, 1, 0, 1)), 3, 2)


@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "%dx%dx%d" % (s[0], s[0], s[1]))
@pytest.mark.parametrize("maps", [1, 3, 130])
def test_groupnorm(shape, maps):
    S, Cc = shape
    g = torch.Generator().manual_seed(4100 + S + Cc + maps)
    x, y = torch.randn(maps, S, S, Cc, generator=g) * 2 + 0.5, torch.randn(maps, S, S, Cc, generator=g)
    hard = 1e3 + torch.randn(1, S, S, Cc, generator=g)                                      # mean 1e3, spread 1: a one-pass variance fails here
    gam, bet, gy, by = (torch.rand(Cc, generator=g) + 0.5, 0.1 * torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5,
                        0.1 * torch.randn(Cc, generator=g))
    d = lambda t: t.to(DEV)
    cl = lambda t: t.permute(0, 2, 3, 1)
    eps = 1e-4
    for relu in (False, True):
        act = F.relu if relu else (lambda t: t)
        got = ops.musiq_groupnorm_f32(d(x), d(gam), d(bet), eps, relu=relu)
        gate_check(f"groupnorm {shape} x {maps} relu {relu}", got, cl(act(_gn64(x, gam, bet, eps))), cl(act(_gn64(x, gam, bet, eps, torch.float32))))
        assert torch.equal(ops.musiq_groupnorm_f32(d(x), d(gam), d(bet), eps, relu=relu), got)
        assert torch.equal(ops.musiq_groupnorm_f32(d(x)[-1:].contiguous(), d(gam), d(bet), eps, relu=relu), got[-1:])     # batch-independent
        buf = d(x).clone()
        assert torch.equal(ops.musiq_groupnorm_f32(buf, d(gam), d(bet), eps, relu=relu, out=buf), got)                    # in place
        got = ops.musiq_groupnorm_f32(d(x), d(gam), d(bet), eps, relu=relu, pool=True)
        assert tuple(got.shape) == (maps, S // 2, S // 2, Cc)
        gate_check(f"groupnorm + pool {shape} x {maps} relu {relu}", got, cl(_pool(act(_gn64(x, gam, bet, eps)))),
                   cl(_pool(act(_gn64(x, gam, bet, eps, torch.float32)))))
        got = ops.musiq_groupnorm_f32(d(x), d(gam), d(bet), eps, relu=relu, y=d(y), gamma_y=d(gy), beta_y=d(by))
        gate_check(f"groupnorm sum {shape} x {maps} relu {relu}", got, cl(act(_gn64(x, gam, bet, eps) + _gn64(y, gy, by, eps))),
                   cl(act(_gn64(x, gam, bet, eps, torch.float32) + _gn64(y, gy, by, eps, torch.float32))))
    # the statistics are two-pass: on the mean-1e3 map the error stays at the rounding of the output, where a one-pass fp32 variance is off by percents
    got = ops.musiq_groupnorm_f32(d(hard), d(gam), d(bet), eps)
    err = gate_check(f"groupnorm {shape}, mean 1e3", got, cl(_gn64(hard, gam, bet, eps)), cl(_gn64(hard, gam, bet, eps, torch.float32)))
    assert err < 1e-5


# ---- 3. LayerNorm -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 7, 129])
def test_layernorm(rows):
    g = torch.Generator().manual_seed(4200 + rows)
    x = torch.randn(rows, 384, generator=g) * 3 + 0.2
    hard = 1e3 + torch.randn(1, 384, generator=g)                                            # a row with mean 1e3, spread 1
    gam, bet = torch.rand(384, generator=g) + 0.5, 0.1 * torch.randn(384, generator=g)
    want = F.layer_norm(x.double(), (384,), gam.double(), bet.double(), 1e-6)
    got = ops.layernorm_f32(x.to(DEV), gam.to(DEV), bet.to(DEV), 1e-6)
    gate_check(f"layernorm {rows} rows", got, want, F.layer_norm(x, (384,), gam, bet, 1e-6))
    hard64 = F.layer_norm(hard.double(), (384,), gam.double(), bet.double(), 1e-6)
    err = gate_check("layernorm, mean 1e3", ops.layernorm_f32(hard.to(DEV), gam.to(DEV), bet.to(DEV), 1e-6), hard64,
                     F.layer_norm(hard, (384,), gam, bet, 1e-6))
    assert err < 1e-5
    wide = torch.zeros(rows, 3, 384, device=DEV)                                             # rows at a stride, as token 0 of every frame is
    wide[:, 0] = x.to(DEV)
    assert torch.equal(ops.layernorm_f32(wide[:, 0], gam.to(DEV), bet.to(DEV), 1e-6), got)
    assert torch.equal(ops.layernorm_f32(x.to(DEV), gam.to(DEV), bet.to(DEV), 1e-6), got)


# ---- 4. attention -----------------------------------------------------------------------------------------------------------------------
def _attention_lengths():
    qt, kvt = ops.mha_f32_tiles()
    return sorted({1, 2, 63, 64, 65, 127, 129, 257} | {t + d for t in (qt, kvt) for d in (-1, 0, 1)})


def _attn64(q, k, v, dtype=torch.float64):
    B, Tn, _ = q.shape
    sp = lambda t: t.to(dtype).view(B, Tn, 6, 64).transpose(1, 2)
    s = sp(q) @ sp(k).transpose(-1, -2) / 8
    return (torch.softmax(s, dim=-1) @ sp(v)).transpose(1, 2).reshape(B, Tn, 384), s


def test_attention_tiles_are_reported():
    assert ops.mha_f32_tiles() == (64, 32)


@pytest.mark.parametrize("Tn", _attention_lengths())
def test_attention(Tn):
    g = torch.Generator().manual_seed(4300 + Tn)
    qkv = torch.randn(2, Tn, 1152, generator=g)
    for boost, what in ((1.0, "unit scores"), (15.0, "scores to +-60")):
        buf = qkv.clone()
        buf[..., :384] *= boost
        q, k, v = buf[..., :384], buf[..., 384:768], buf[..., 768:]
        want, s = _attn64(q, k, v)
        dbuf = buf.to(DEV)
        got = ops.mha_f32(dbuf[..., :384], dbuf[..., 384:768], dbuf[..., 768:])
        assert bool(torch.isfinite(got).all())
        gate_check(f"attention T {Tn}, {what} (|s| <= {float(s.abs().max()):.1f})", got, want, _attn64(q, k, v, torch.float32)[0])
        assert torch.equal(ops.mha_f32(dbuf[..., :384], dbuf[..., 384:768], dbuf[..., 768:]), got)                          # a repeat call
        alone = dbuf[1:].contiguous()
        assert torch.equal(ops.mha_f32(alone[..., :384], alone[..., 384:768], alone[..., 768:]), got[1:])                   # frame 1 alone
        assert torch.equal(ops.mha_f32(q.contiguous().to(DEV), k.contiguous().to(DEV), v.contiguous().to(DEV)), got)        # dense operands
    if Tn >= 63:
        assert float(s.abs().max()) > 40


# ---- 5. Linears and GELU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [384, 1152, 16384])
def test_linears_are_the_pointwise_walk(K):
    """linear_f32 is resnet_conv_f32's 1 x 1 walk with the rows as pixels and no new epilogue: its bits are the general walk's, with the
    residual and ReLU as exact torch ops, and it sits inside the gate against fp64."""
    Nn = 1152 if K == 384 else 384
    g = torch.Generator().manual_seed(4400 + K)
    w = (torch.randn(Nn, K, generator=g) / math.sqrt(K))
    b = 0.1 * torch.randn(Nn, generator=g)
    wp = w.t().contiguous()[None, None].to(DEV)
    for Mm in (1, 127, 129):
        x, res = torch.randn(Mm, K, generator=g), torch.randn(Mm, Nn, generator=g)
        assert ops.resnet_conv_kernel_name((1, 1, Mm, K), (1, 1, K, Nn)) == "pointwise_f32_kernel"
        base = ops.convnet_conv_f32(x.to(DEV)[None, None], wp, b.to(DEV), pad=(0, 0), relu=False)[0, 0]      # conv_f32_kernel: acc + bias
        got = ops.linear_f32(x.to(DEV), wp, b.to(DEV))
        assert torch.equal(got, base), (K, Mm)
        gate_check(f"linear {K} -> {Nn}, {Mm} rows", got, F.linear(x.double(), w.double(), b.double()), F.linear(x, w, b))
        acc = res.to(DEV).clone()
        assert ops.linear_f32(x.to(DEV), wp, b.to(DEV), residual=acc, out=acc).data_ptr() == acc.data_ptr()
        assert torch.equal(acc, base + res.to(DEV))
        assert torch.equal(ops.linear_f32(x.to(DEV), wp, b.to(DEV), relu=True), base.clamp_min(0))


@pytest.mark.parametrize("count", [1, 255, 129 * 1152])
def test_gelu_pass(count):
    x = torch.randn(count, generator=torch.Generator().manual_seed(4500 + count)) * 3
    got = ops.gelu_f32(x.to(DEV))
    gate_check(f"gelu {count}", got, F.gelu(x.double()), F.gelu(x))
    buf = x.to(DEV)
    assert ops.gelu_f32(buf, out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, got)


def test_embed_and_score():
    g = torch.Generator().manual_seed(4600)
    geo = Q.token_geometry(33, 47)
    tok = geo["tokens"]
    Tn = tok.shape[0]
    emb, pos, sc, cls = (torch.randn(2 * Tn, 384, generator=g), torch.randn(100, 384, generator=g), torch.randn(3, 384, generator=g),
                         torch.randn(384, generator=g))
    got = ops.musiq_embed_f32(emb.to(DEV), pos.to(DEV), sc.to(DEV), cls.to(DEV), tok.to(DEV)).cpu()
    want = torch.cat([cls.expand(2, 1, 384), (emb.view(2, Tn, 384) + pos[tok[:, 3].long()]) + sc[tok[:, 0].long()]], dim=1)
    assert torch.equal(got, want)
    f = torch.randn(5, 384, generator=g)
    for K in (1, 10):
        w, b = torch.randn(K, 384, generator=g) / 8, torch.randn(K, generator=g)
        row = F.linear(f.double(), w.double(), b.double())
        want = row[:, 0] if K == 1 else (torch.softmax(row, -1) * torch.arange(1, K + 1).double()).sum(-1)
        got = ops.musiq_score(f.to(DEV), w.to(DEV), b.to(DEV))
        assert got.dtype == torch.float64 and float((got.cpu() - want).abs().max()) <= 1e-13 * float(want.abs().max())


# ---- 6. the whole network ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", T.NET_SIZES, ids=lambda s: "%dx%d" % s)
def test_whole_network_against_the_restatement(size):
    """All 14 layers and the rule-generated state.  Gates: 20 x the deviation of the restatement's own fp32 host run from its fp64 host run
    over this test's images, on the score and on the 384-wide normalised token 0."""
    ref, W, pred = T.reference(size), weights(), T.images(*size)
    dev_s, dev_f = float((ref["s32"] - ref["s64"]).abs().max()), float((ref["f32"] - ref["f64"]).abs().max())
    got, feat = Q.musiq(W, pred.to(DEV), want_features=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3,) and tuple(feat.shape) == (3, 384)
    err_s, err_f = float((got.cpu() - ref["s64"]).abs().max()), float((feat.cpu().double() - ref["f64"]).abs().max())
    print(f"musiq @ {size}: values {got.tolist()}; score: restatement fp32-vs-fp64 deviation {dev_s:.3e}, gate {20 * dev_s:.3e}, kernels' "
          f"error {err_s:.3e}; token 0: deviation {dev_f:.3e}, gate {20 * dev_f:.3e}, kernels' error {err_f:.3e}")
    assert err_s <= 20 * dev_s
    assert err_f <= 20 * dev_f
    before = Q.COUNTERS["groups"]
    assert torch.equal(Q.musiq(W, pred.to(DEV), group=1), got) and Q.COUNTERS["groups"] == before + 3      # one frame per group: the same bits
    assert torch.equal(Q.musiq(W, pred.to(DEV), group=2), got)
    u8 = (pred * 255).round().to(torch.uint8).to(DEV)
    assert torch.equal(Q.musiq(W, u8.permute(0, 2, 3, 1).contiguous()), Q.musiq(W, u8))                    # [F,H,W,3] frames are taken as such


def test_ava_head():
    size = T.NET_SIZES[2]
    sd, pred = T.state(10), T.images(*size)
    s64, _ = R.musiq(sd, pred, torch.float64)
    s32, _ = R.musiq(sd, pred, torch.float32)
    dev = float((s32.double() - s64).abs().max())
    got = Q.musiq(weights(10), pred.to(DEV))
    err = float((got.cpu() - s64).abs().max())
    print(f"musiq, 10-class head @ {size}: values {got.tolist()}; deviation {dev:.3e}, gate {20 * dev:.3e}, kernels' error {err:.3e}")
    assert bool(((got > 1) & (got < 10)).all()) and err <= 20 * dev


# ---- 7. the production token count ------------------------------------------------------------------------------------------------------
def test_production_token_count(monkeypatch):
    """One 720 x 1280 frame, 1033 tokens: ragged tiles on every kernel.  Two layers against the restatement; the full depth is finite."""
    frame = F.interpolate(T.images(90, 160)[1:2], size=(720, 1280), mode="bilinear").clamp(0, 1)
    W = weights()
    full = Q.musiq(W, frame.to(DEV))
    print(f"one 720 x 1280 frame, {Q.NUM_LAYERS} layers: {full.tolist()}")
    assert tuple(full.shape) == (1,) and bool(torch.isfinite(full).all()) and Q.token_geometry(720, 1280)["length"] == 1033
    monkeypatch.setattr(Q, "NUM_LAYERS", 2)
    s64, f64 = R.musiq(T.state(), frame, torch.float64, layers=2)
    s32, f32 = R.musiq(T.state(), frame, torch.float32, layers=2)
    dev_s, dev_f = float((s32.double() - s64).abs().max()), float((f32.double() - f64).abs().max())
    got, feat = Q.musiq(W, frame.to(DEV), want_features=True)
    err_s, err_f = float((got.cpu() - s64).abs().max()), float((feat.cpu().double() - f64).abs().max())
    print(f"two layers: value {got.tolist()}; score: deviation {dev_s:.3e}, gate {20 * dev_s:.3e}, kernels' error {err_s:.3e}; token 0: "
          f"deviation {dev_f:.3e}, gate {20 * dev_f:.3e}, kernels' error {err_f:.3e}")
    assert err_s <= 20 * dev_s and err_f <= 20 * dev_f
    assert float(got) != float(full)


# ---- 8. surfaces ------------------------------------------------------------------------------------------------------------------------
def _clips(seed, F_=3, H=40, W=56):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, 256, (F_, H, W, 3), generator=g, dtype=torch.uint8)
    pred = (gt.int() + torch.randint(-20, 21, gt.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return pred, gt


def _weights_dir(path):
    path.mkdir()
    torch.save({"params": T.state()}, path / "musiq_koniq_ckpt.pth")
    return str(path)


def test_create_metric_and_clip_metrics():
    W = weights()
    pred, gt = _clips(5)
    p = pred.to(DEV).permute(0, 3, 1, 2).float() / 255.0
    m = M.create_metric("musiq", weights=W)
    want = Q.musiq(W, p)
    assert want.dtype == torch.float64 and tuple(want.shape) == (3,)
    assert torch.equal(m(p), want) and torch.equal(m(p.cpu()), want)            # host images are moved
    assert torch.equal(m.to(DEV).eval()(p[0]), want[:1])                         # one [C,H,W] image
    vals = M.nr_clip_metrics(pred, ["musiq"], {"musiq": W})
    assert vals == {"musiq": float(Q.musiq(W, pred.to(DEV)).mean())}
    both = M.clip_metrics(pred, gt, "psnr,musiq".split(","), crop=4, test_y_channel=True, weights={"musiq": W})
    assert both["musiq"] == vals["musiq"] and both["psnr"] == M.clip_metrics(pred, gt, ["psnr"], crop=4, test_y_channel=True)["psnr"]


def test_command_lines(tmp_path, capsys):
    from PIL import Image
    from dove_amd import eval_metrics
    pred_dir, img_dir = tmp_path / "pred", tmp_path / "img"
    pred_dir.mkdir()
    img_dir.mkdir()
    wdir = _weights_dir(tmp_path / "w")
    clips = {n: _clips(s)[0] for n, s in (("a", 1), ("b", 2), ("c", 3))}
    for name, pred in clips.items():
        np.save(pred_dir / f"{name}.npy", pred.numpy())
    W = Q.MusiqWeights.load(wdir)
    want = {n: round(float(Q.musiq(W, p.to(DEV)).mean()), 4) for n, p in clips.items()}
    out = eval_metrics.main(["--pred", str(pred_dir), "--out", str(tmp_path / "nr"), "--metrics", "musiq", "--metric_weights", wdir])
    with open(tmp_path / "nr" / "metrics_musiq.json") as f:
        assert json.load(f) == out
    assert out["count"] == 3 and out["per_sample"] == {n: {"musiq": v} for n, v in want.items()} and len(set(want.values())) == 3
    capsys.readouterr()
    for i in range(2):
        Image.fromarray(clips["a"][i].numpy()).save(img_dir / f"f{i}.png")
    scores = Q.main(["score", "--pred", str(img_dir), "--metric_weights", wdir])
    direct = Q.musiq(weights(), clips["a"].to(DEV))
    assert scores == {"f0.png": float(direct[0]), "f1.png": float(direct[1])} and "average:" in capsys.readouterr().out
