"""FasterVQA / FAST-VQA on the GPU (csrc/swin3d.hip, dove_amd/fastvqa.py): the gathers and the merge bit for bit against the restatement
(tests/fastvqa_ref.py), the window attention and the networks inside 20 x the deviation of the restatement's own fp32 run from its fp64
run on the same inputs (an operator whose deviation is 0 must have error 0), the head against fp64, the production shapes and the tool."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fastvqa_ref as R
import test_fastvqa_cpu as T
from dove_amd import eval_fastvqa as E
from dove_amd import fastvqa as Q
from dove_amd import ops, prepost, y4m

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory():
    """Weights (110 MB per production preset) and the geometry tables stay on the device while the module runs; drop them and hand the
    blocks back when it is done, and check that nothing else was left: device memory returns to its level before the module."""
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


def weights(cfg, seed=5):
    if cfg.name not in _CACHE:
        sd = Q.random_state(cfg, seed)
        _CACHE[cfg.name] = (sd, Q.VqaWeights.from_state_dict(sd, cfg))
    return _CACHE[cfg.name]


def gate_check(what, got, want64, torch32):
    """``got`` (device fp32 or a float) against ``want64`` inside 20 x the deviation of ``torch32`` (the fp32 restatement) from ``want64``."""
    as64 = lambda t: t.detach().cpu().double() if isinstance(t, torch.Tensor) else torch.tensor(float(t), dtype=torch.float64)
    want64 = as64(want64)
    dev = float((as64(torch32) - want64).abs().max())
    err = float((as64(got) - want64).abs().max())
    print(f"{what}: fp32-vs-fp64 deviation {dev:.3e}, gate {20 * dev:.3e}, kernels' error {err:.3e}")
    assert math.isfinite(err) and err <= 20 * dev, what
    return err


# ---- 1. the fragment gather -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,fsize,tg", [((2, 2), (8, 8), 2), ((7, 7), (4, 4), 1)], ids=["2x2of8x8", "7x7of4x4"])
def test_fragment_gather(grid, fsize, tg):
    cfg = {"fragments": grid, "fsize": fsize, "t_groups": tg}
    (gh, gw), (fh, fw) = grid, fsize
    Fn, Tn, H, W = 5, 4, gh * fh + 5, gw * fw + 9
    g = torch.Generator().manual_seed(5000 + gh)
    idx = np.array([4, 0, 0, 3], dtype=np.int32)
    org = np.zeros((gh, gw, tg, 2), dtype=np.int32)                       # offsets at 0 and at their maximum, and some between
    pick = torch.randint(0, 3, (gh, gw, tg, 2), generator=g).numpy()
    org[..., 0] = np.choose(pick[..., 0], [0, H - fh, (H - fh) // 2])
    org[..., 1] = np.choose(pick[..., 1], [0, W - fw, (W - fw) // 3])
    org[0, 0, 0], org[-1, -1, -1] = (0, 0), (H - fh, W - fw)
    didx, dorg = torch.from_numpy(idx).to(DEV), torch.from_numpy(org).to(DEV)

    def case(view_dev, host, what):
        want = R.fragments(host, idx, org, cfg)
        got = ops.vqa_fragments_f32(view_dev, didx, dorg, fsize, Q.MEAN, Q.STD)
        assert tuple(got.shape) == (Tn, gh * fh, gw * fw, 3) and torch.equal(got.cpu(), want), what
        cols = ops.vqa_fragments_f32(view_dev, didx, dorg, fsize, Q.MEAN, Q.STD, cols=True)
        Hc, Wc = gh * fh, gw * fw
        assert torch.equal(cols.cpu().view(Tn // 2, Hc // 4, Wc // 4, 3, 2, 4, 4),
                           want.view(Tn // 2, 2, Hc // 4, 4, Wc // 4, 4, 3).permute(0, 2, 4, 6, 1, 3, 5)), what
        return got

    u8 = torch.randint(0, 256, (Fn, H, W, 3), generator=g, dtype=torch.uint8)
    a = case(u8.to(DEV).permute(0, 3, 1, 2), u8, "u8 frames")
    assert torch.equal(case(u8.to(DEV).permute(0, 3, 1, 2).contiguous(), u8, "u8 planes"), a)
    f32 = torch.rand(Fn, 3, H, W, generator=g)
    case(f32.to(DEV), f32, "f32")
    bf = f32.bfloat16()
    case(bf.to(DEV), bf, "bf16")
    big = torch.rand(Fn, H + 5, W + 3, 3, generator=g)                     # a cropped and permuted view
    crop = big[:, 2:2 + H, 1:1 + W].permute(0, 3, 1, 2)
    case(big.to(DEV)[:, 2:2 + H, 1:1 + W].permute(0, 3, 1, 2), crop, "crop")
    unit = (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()           # 255 (u / 255) is not always u: the two intakes are two definitions
    case(unit.to(DEV), unit, "u / 255 as f32")


# ---- 2. window gather and scatter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,window", [((4, 8, 8), (2, 4, 4)), ((4, 7, 7), (4, 4, 4)), ((2, 7, 5), (2, 3, 3))], ids=str)
@pytest.mark.parametrize("shifted", [False, True])
def test_window_gather_scatter(dims, window, shifted):
    geo = Q.geometry(dims, window, (7, 7), shifted)
    ws, ss, (Dp, Hp, Wp) = geo["window"], geo["shift"], geo["padded"]
    if dims == (4, 7, 7):
        assert ws == (4, 4, 4) and ss[0] == 0 and (Hp, Wp) == (8, 8)       # D clamped: no shift there; 7 padded to 8
    B, C = 2, 8
    D, H, W = dims
    g = torch.Generator().manual_seed(5100 + D * H * W + shifted)
    x = torch.randn(B, D, H, W, C, generator=g)
    h = F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H, 0, Dp - D))
    want = R.window_partition(torch.roll(h, shifts=tuple(-s for s in ss), dims=(1, 2, 3)), ws)
    got = ops.swin3d_window_gather_f32(x.to(DEV), ws, ss)
    assert tuple(got.shape) == (B * geo["windows"], geo["length"], C) and torch.equal(got.cpu(), want)
    ones = ops.swin3d_window_gather_f32(torch.ones_like(x).to(DEV), ws, ss)
    assert int((ones == 0).sum()) == B * C * (Dp * Hp * Wp - D * H * W)    # the padded slots read zero
    wins, short = torch.randn(want.shape, generator=g), torch.randn(x.shape, generator=g)
    back = torch.roll(R.window_reverse(wins, ws, B, Dp, Hp, Wp), shifts=ss, dims=(1, 2, 3))[:, :D, :H, :W]
    merged = ops.swin3d_window_scatter_f32(wins.to(DEV), short.to(DEV), ws, ss)
    assert torch.equal(merged.cpu(), short + back)
    assert torch.equal(ops.swin3d_window_scatter_f32(got, short.to(DEV), ws, ss).cpu(), short + x)      # scatter(gather(x)) + shortcut
    buf = short.to(DEV).clone()
    assert ops.swin3d_window_scatter_f32(wins.to(DEV), buf, ws, ss, out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, merged)
    assert torch.equal(ops.swin3d_window_gather_f32(x[1:].to(DEV), ws, ss), got[geo["windows"]:])       # batch-independent


# ---- 3. window attention ----------------------------------------------------------------------------------------------------------------
def _attention_lengths():
    qt, kvt, mx = ops.swin3d_attention_tiles()
    return sorted({1, 18, 64, 392} | {t + d for t in (qt, kvt) for d in (-1, 0, 1)} | {mx - 1, mx})


def _attn_ref(qkv, heads, ta, tb, index, frag, region, dtype):
    """softmax((q scale) k^T + bias + mask) v as the restatement's window_attention writes it; also returns the scores."""
    Wn, N, _ = qkv.shape
    t = qkv.to(dtype).reshape(Wn, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    s = (t[0] * 32 ** -0.5) @ t[1].transpose(-2, -1)
    bias = ta.to(dtype)[index.reshape(-1).long()].reshape(N, N, heads).permute(2, 0, 1)[None]
    if tb is not None:
        other = tb.to(dtype)[index.reshape(-1).long()].reshape(N, N, heads).permute(2, 0, 1)[None]
        fr = frag.repeat(Wn // frag.shape[0], 1)
        bias = torch.where((fr[:, :, None] != fr[:, None, :])[:, None], other, bias)
    s = s + bias
    if region is not None:
        rg = region.repeat(Wn // region.shape[0], 1)
        s = s + torch.where(rg[:, :, None] != rg[:, None, :], R.MASK_VALUE, 0.0).to(dtype)[:, None]
    return (torch.softmax(s, dim=-1) @ t[2]).transpose(1, 2).reshape(Wn, N, heads * 32), s


def test_attention_tiles_are_reported():
    assert ops.swin3d_attention_tiles() == (32, 32, 392)


@pytest.mark.parametrize("N", _attention_lengths())
def test_window_attention(N):
    rows, peak = 75, 0.0
    for heads, Wn in ((1, 1), (3, 5)):
        g = torch.Generator().manual_seed(5200 + 7 * N + heads)
        D = heads * 32
        qkv = torch.randn(Wn, N, 3 * D, generator=g)
        qkv[..., :D] *= 7.0                                                # scores to about +-30
        pad = N // 4                                                       # zero-padded tokens: their q, k, v are the Linear's bias
        if pad:
            qkv[:, N - pad:] = 0.3 * torch.randn(3 * D, generator=g)
        ta, tb = torch.randn(rows, heads, generator=g), torch.randn(rows, heads, generator=g)
        index = torch.randint(0, rows, (N, N), generator=g, dtype=torch.int32)
        frag = torch.randint(0, 4, (Wn, N), generator=g, dtype=torch.int32)
        region = torch.randint(0, 3, (Wn, N), generator=g, dtype=torch.int32)
        dq, d = qkv.to(DEV), lambda t: None if t is None else t.to(DEV)
        for masked in (False, True):
            for gated in (False, True):
                for shared in ((False, True) if Wn > 1 and masked and gated else (False,)):     # one id table for every window
                    fr, rg = (frag[:1] if shared else frag) if gated else None, (region[:1] if shared else region) if masked else None
                    want, s = _attn_ref(qkv, heads, ta, tb if gated else None, index, fr, rg, torch.float64)
                    w32, _ = _attn_ref(qkv, heads, ta, tb if gated else None, index, fr, rg, torch.float32)
                    got = ops.swin3d_window_attention_f32(dq, heads, d(ta), d(index), table_b=d(tb) if gated else None, frag=d(fr), region=d(rg))
                    assert bool(torch.isfinite(got).all())
                    peak = max(peak, 0.0 if masked else float(s.abs().max()))
                    gate_check(f"window attention N {N}, heads {heads}, windows {Wn}, mask {masked}, gate {gated}, shared ids {shared} "
                               f"(|s| <= {float(s.abs().max()):.1f})", got, want, w32)
                    again = ops.swin3d_window_attention_f32(dq, heads, d(ta), d(index), table_b=d(tb) if gated else None, frag=d(fr), region=d(rg))
                    assert torch.equal(again, got)                                                # a repeat call
                    if Wn > 1 and not shared:                                                     # a batch split: window 3 alone
                        cut = lambda t: None if t is None else t[3:4].contiguous().to(DEV)
                        alone = ops.swin3d_window_attention_f32(dq[3:4].contiguous(), heads, d(ta), d(index), table_b=d(tb) if gated else None,
                                                                frag=cut(fr), region=cut(rg))
                        assert torch.equal(alone, got[3:4])
    if N >= 64:
        assert peak > 25                                                   # without the mask's -100


@pytest.mark.parametrize("N", [18, 64, 392])
def test_window_attention_single_admissible_key(N):
    """Every token its own shift region: the mask leaves each row its own key, and the output is that key's V row exactly."""
    heads, Wn = 3, 2
    g = torch.Generator().manual_seed(5300 + N)
    qkv = torch.randn(Wn, N, 9 * 32, generator=g)
    ta = torch.randn(40, heads, generator=g)
    index = torch.randint(0, 40, (N, N), generator=g, dtype=torch.int32)
    region = torch.arange(N, dtype=torch.int32)[None]
    got = ops.swin3d_window_attention_f32(qkv.to(DEV), heads, ta.to(DEV), index.to(DEV), region=region.to(DEV))
    assert torch.equal(got.cpu(), qkv[..., 6 * 32:])


# ---- 4. patch merge and head ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(4, 6), (5, 7), (4, 7), (5, 6), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_patch_merge(hw):
    H, W = hw
    x = torch.randn(2, 3, H, W, 8, generator=torch.Generator().manual_seed(5400 + 10 * H + W))
    p = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    want = torch.cat([p[:, :, 0::2, 0::2], p[:, :, 1::2, 0::2], p[:, :, 0::2, 1::2], p[:, :, 1::2, 1::2]], -1)
    got = ops.swin3d_patch_merge_f32(x.to(DEV))
    assert tuple(got.shape) == (2, 3, (H + 1) // 2, (W + 1) // 2, 32) and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("shape", [(1, 1, 32, 1), (2, 37, 256, 16), (3, 784, 768, 64)], ids=str)
def test_head(shape):
    n, tokens, dim, hid = shape
    g = torch.Generator().manual_seed(5500 + tokens)
    f = torch.randn(n, tokens, dim, generator=g)
    sd = {"vqa_head.fc_hid.weight": torch.randn(hid, dim, 1, 1, 1, generator=g) / math.sqrt(dim), "vqa_head.fc_hid.bias": torch.randn(hid, generator=g),
          "vqa_head.fc_last.weight": torch.randn(1, hid, 1, 1, 1, generator=g), "vqa_head.fc_last.bias": torch.randn(1, generator=g)}
    want = R.head(f.double(), sd, torch.float64)
    got = ops.vqa_head_f64(f.to(DEV), sd["vqa_head.fc_hid.weight"].flatten(1).to(DEV), sd["vqa_head.fc_hid.bias"].to(DEV),
                           sd["vqa_head.fc_last.weight"].flatten().to(DEV), sd["vqa_head.fc_last.bias"].to(DEV))
    err = float((got.cpu() - want).abs().max())
    print(f"head {shape}: values {got.tolist()}, error {err:.3e}")
    assert got.dtype == torch.float64 and err <= 1e-13 * float(want.abs().max())
    assert torch.equal(ops.vqa_head_f64(f[-1:].to(DEV), sd["vqa_head.fc_hid.weight"].flatten(1).to(DEV), sd["vqa_head.fc_hid.bias"].to(DEV),
                                        sd["vqa_head.fc_last.weight"].flatten().to(DEV), sd["vqa_head.fc_last.bias"].to(DEV)), got[-1:])


# ---- 5. the whole network, tiny ---------------------------------------------------------------------------------------------------------
def _frames(seed, Fn, H, W):
    """uint8 [F,H,W,3]: a smooth moving pattern plus noise, so that fragments differ by where and when they are cut."""
    g = torch.Generator().manual_seed(seed)
    t, y, x = torch.meshgrid(torch.arange(Fn).float(), torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    base = torch.stack([torch.sin(0.11 * x + 0.3 * t), torch.cos(0.07 * y - 0.2 * t), torch.sin(0.05 * (x + y) + 0.1 * t)], -1)
    return ((0.5 + 0.35 * base + 0.15 * torch.rand(Fn, H, W, 3, generator=g)).clamp(0, 1) * 255).round().to(torch.uint8)


@pytest.mark.parametrize("cfg,size", [(T.TINY_A, (12, 40, 50)), (T.TINY_B, (10, 37, 45))], ids=["A", "B"])
def test_whole_network_tiny(cfg, size):
    sd, W = weights(cfg)
    frames = _frames(5600 + size[0], *size)
    plan = Q.sample_plan(*size, cfg, seed=11)
    cfgd = T.as_dict(cfg)
    clips = torch.stack([R.fragments(frames, plan[0][c], plan[1][c], cfgd) for c in range(cfg.num_clips)])
    f64, f32 = R.backbone(clips, sd, cfgd, torch.float64), R.backbone(clips, sd, cfgd, torch.float32)
    s64 = R.head(f64.flatten(1, 3), sd, torch.float64).mean()
    s32 = R.head(f32.flatten(1, 3), sd, torch.float32).mean()
    assert float(s64) == float(R.raw_score(sd, frames, cfgd, plan, torch.float64))
    dev_frames = frames.to(DEV)
    Wd = W.to(torch.device(DEV))
    view = Q.clip_view(dev_frames)
    maps = torch.cat([Q.embed(Wd, view, torch.from_numpy(plan[0][c]).to(DEV), torch.from_numpy(plan[1][c]).to(DEV)) for c in range(cfg.num_clips)])
    gate_check(f"{cfg.name}: patch embedding", maps, R.patch_embed(clips, sd, torch.float64), R.patch_embed(clips, sd, torch.float32))
    gate_check(f"{cfg.name}: final map {tuple(f64.shape)}", Q.backbone(Wd, maps), f64, f32)
    raw, scaled = Q.score_clip(dev_frames, W, plan=plan)
    print(f"{cfg.name}: raw {raw!r}, rescaled {scaled!r}, restatement fp64 {float(s64)!r}")
    gate_check(f"{cfg.name}: raw score", raw, s64, s32)
    assert isinstance(raw, float) and scaled == R.rescale(raw, *cfg.rescale) and 0.0 < scaled < 1.0
    assert Q.score_clip(dev_frames, W, plan=plan) == (raw, scaled)                               # a repeat call
    assert Q.score_clip(frames, W, plan=plan) == (raw, scaled)                                   # host frames are uploaded
    assert Q.score_clip(dev_frames, W, seed=11) == (raw, scaled)                                 # the plan drawn from the seed
    before = Q.COUNTERS["groups"]
    assert Q.score_clip(dev_frames, W, plan=plan, group=1) == (raw, scaled) and Q.COUNTERS["groups"] == before + cfg.num_clips
    if cfg.num_clips > 1:                                                                        # one batch split and another
        assert Q.score_clip(dev_frames, W, plan=plan, group=cfg.num_clips) == (raw, scaled)
    assert Q.score_clip(dev_frames, W, plan=plan, rescale=(0.0, 1.0))[1] == 1.0 / (1.0 + math.exp(-raw))
    with pytest.raises(ValueError, match="smaller than the"):
        Q.score_clip(dev_frames[:, :cfg.canvas[0] - 1], W)


# ---- 6. the production shape ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["FasterVQA", "FAST-VQA"])
def test_production_shape(name):
    """One clip of the preset on the 32 x 224 x 224 canvas: the patch embedding and one block per shift parity of stage 0 (784 windows of 64
    tokens, or 128 of 392) against the fp64 restatement; the full depth is finite and identical across two calls."""
    cfg = Q.preset(name)
    sd, W = weights(cfg)
    frames = _frames(5700, 70, 240, 256)
    plan = Q.sample_plan(70, 240, 256, cfg, seed=3)
    cfgd = T.as_dict(cfg)
    clip = R.fragments(frames, plan[0][0], plan[1][0], cfgd)[None]
    f64, f32 = R.backbone(clip, sd, cfgd, torch.float64, stages=1), R.backbone(clip, sd, cfgd, torch.float32, stages=1)
    Wd = W.to(torch.device(DEV))
    dev_frames = frames.to(DEV)
    x = Q.embed(Wd, Q.clip_view(dev_frames), torch.from_numpy(plan[0][0]).to(DEV), torch.from_numpy(plan[1][0]).to(DEV))
    assert tuple(x.shape) == (1, 16, 56, 56, 96)
    geo = Q.geometry((16, 56, 56), cfg.window, cfg.fragments, True)
    assert (geo["windows"], geo["length"]) == ((784, 64) if name == "FasterVQA" else (128, 392)) and geo["region"] is not None
    gate_check(f"{name}: stage 0 {tuple(f64.shape)}", Q.backbone(Wd, x, stages=1), f64, f32)
    del x
    a, b = Q.score_clip(dev_frames, W, seed=3), Q.score_clip(dev_frames, W, seed=3)
    print(f"{name}: full depth, {cfg.num_clips} clip(s): raw {a[0]!r}, rescaled {a[1]!r}")
    assert math.isfinite(a[0]) and 0.0 <= a[1] <= 1.0 and a == b


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, monkeypatch):
    from PIL import Image
    cfg = T.TINY_A
    monkeypatch.setitem(Q.PRESETS, "FasterVQA", cfg)                      # the tool on the tiny network: a 110 MB file teaches nothing more
    sd, _ = weights(cfg)
    torch.save({"state_dict": sd}, tmp_path / "tiny.pth")
    pred = tmp_path / "pred"
    (pred / "png").mkdir(parents=True)
    frames = _frames(5800, 6, 40, 48)
    for i, fr in enumerate(frames):
        Image.fromarray(fr.numpy()).save(pred / "png" / f"{i:04d}.png")
    g = torch.Generator().manual_seed(5801)
    with y4m.Y4MWriter(str(pred / "clip.y4m"), 48, 40, 25, "444") as wr:
        wr.write(torch.randint(16, 236, (5, 3 * 40 * 48), generator=g, dtype=torch.uint8))
    live = torch.cuda.memory_allocated()
    out = E.main(["--pred", str(pred), "--model", str(tmp_path / "tiny.pth"), "--seed", "9", "--out", str(tmp_path / "o")])
    W = Q.VqaWeights.load(str(tmp_path / "tiny.pth"), cfg)
    want = {}
    for name in ("clip.y4m", "png"):
        raw, scaled = Q.score_clip(prepost.load_frames(str(pred / name)), W, seed=9)
        want[name.split(".")[0]] = {"fastervqa": round(scaled, 4), "fastervqa_raw": round(raw, 4)}
    assert out["per_sample"] == want and out["count"] == 2 and want["clip"] != want["png"]
    with open(tmp_path / "o" / "metrics_fastervqa.json") as f:
        assert json.load(f) == out
    assert torch.equal(prepost.load_frames(str(pred / "png")), frames)
    over = E.main(["--pred", str(pred), "--model", str(tmp_path / "tiny.pth"), "--seed", "9", "--out", str(tmp_path / "o2"), "--rescale_mean", "0",
                   "--rescale_std", "1"])
    assert over["per_sample"]["png"] == {"fastervqa": round(1.0 / (1.0 + math.exp(-Q.score_clip(frames, W, seed=9)[0])), 4),
                                         "fastervqa_raw": want["png"]["fastervqa_raw"]}
    del W
    import gc
    for geo in Q._GEOMETRY.values():
        geo["device"].clear()
    gc.collect()
    assert torch.cuda.memory_allocated() <= live, "the tool left tensors on the device"
