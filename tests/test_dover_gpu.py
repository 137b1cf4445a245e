"""DOVER on the GPU (csrc/convnext3d.hip, dove_amd/dover.py): the depthwise conv, the downsampling and the networks inside 20 x the deviation
of the restatement's (tests/dover_ref.py) own fp32 run from its fp64 run on the same inputs (test_fastvqa_gpu.gate_check), the depthwise
conv's exact cases bit for bit, the resized view against the fp64 restatement rounded once, the production shapes and the tool."""
import gc
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dover_ref as D
import fastvqa_ref as R
import test_dover_cpu as T
from dove_amd import dover as Q
from dove_amd import eval_dover as E
from dove_amd import fastvqa, ops, prepost, y4m
from test_fastvqa_gpu import _frames, gate_check

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}


def _drop_device_tables():
    for geo in fastvqa._GEOMETRY.values():
        geo["device"].clear()
    for taps in ops._RESIZE_TAPS.values():
        taps["device"].clear()


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory():
    """test_fastvqa_gpu's fixture for this module: the weights, the geometry tables and the tap tables stay on the device while the module
    runs; drop them when it is done and check that device memory returns to its level before the module.  The module allocates from a
    memory pool of its own, released with it, so that the caching allocator is left exactly as it was found, its cached free blocks
    included: torch counts a block that it hands out unsplit at the block's size, so a test that compares peaks of ``memory_allocated``
    (test_stream_gpu.test_bounded_memory) sees which blocks earlier modules left cached, and ``empty_cache()`` here would change that."""
    live, reserved = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        _CACHE.clear()
        _drop_device_tables()
        gc.collect()
        torch.cuda.synchronize()
    del pool
    print(f"device memory after the module: allocated {torch.cuda.memory_allocated()} (before: {live}), reserved "
          f"{torch.cuda.memory_reserved()} (before: {reserved})")
    assert torch.cuda.memory_allocated() <= live, "this module left tensors on the device"
    assert torch.cuda.memory_reserved() <= reserved, "this module left segments in the allocator"


def weights(key, cfg, tech, seed=5):
    if key not in _CACHE:
        sd = Q.random_state(cfg, seed, tech)
        _CACHE[key] = (sd, Q.DoverWeights.from_state_dict(sd, cfg, tech))
    return _CACHE[key]


# ---- 1. the depthwise conv --------------------------------------------------------------------------------------------------------------
def _dw_case(shape, seed):
    B, Dd, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), torch.randn(C, 1, 3, 7, 7, generator=g) / 12.0, torch.randn(C, generator=g)


# (1,3,17,15,96): row tiles 9 + 8 and column tiles 8 + 7 (ops.dwconv3d_tile(17, 15) == (9, 8)), C of 1.5 waves of float4 lanes;
# (1,3,9,13,96): column tiles 7 + 6; (1,2,16,16,100): a last channel block of one float4 lane
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 4), (2, 2, 3, 5, 8), (1, 3, 17, 15, 96), (1, 3, 9, 13, 96), (2, 4, 7, 7, 768), (1, 1, 2, 1, 256),
                                   (1, 2, 16, 16, 100)], ids=str)
def test_dwconv_against_conv3d(shape):
    x, w, b = _dw_case(shape, 6000 + sum(shape))
    got = ops.dwconv3d_f32(x.to(DEV), Q.pack_dwconv_weight(w).to(DEV), b.to(DEV))
    assert tuple(got.shape) == shape
    gate_check(f"dwconv3d {shape}", got, D.dwconv(x, w, b, torch.float64), D.dwconv(x, w, b, torch.float32))


def test_dwconv_exact_cases():
    shape = (2, 3, 9, 10, 8)
    x, w, b = _dw_case(shape, 6100)
    wp, zero_b = Q.pack_dwconv_weight(w).to(DEV), torch.zeros(8, device=DEV)
    for pos in ((1, 4, 5), (0, 0, 0), (2, 8, 9)):                         # interior, a corner, the last frame
        imp = torch.zeros(shape)
        imp[1, pos[0], pos[1], pos[2]] = 1.0
        want = torch.zeros(shape)
        for kd in range(3):
            for kh in range(7):
                for kw in range(7):
                    d, h, ww = pos[0] + 1 - kd, pos[1] + 3 - kh, pos[2] + 3 - kw
                    if 0 <= d < 3 and 0 <= h < 9 and 0 <= ww < 10:
                        want[1, d, h, ww] = w[:, 0, kd, kh, kw]
        assert torch.equal(ops.dwconv3d_f32(imp.to(DEV), wp, zero_b).cpu(), want), pos
    assert torch.equal(ops.dwconv3d_f32(x.to(DEV), torch.zeros_like(wp), b.to(DEV)).cpu(), b.expand(shape))       # zero weights: the bias
    xd = x.to(DEV)
    got = ops.dwconv3d_f32(xd, wp, b.to(DEV))
    assert torch.equal(ops.dwconv3d_f32(xd[1:].contiguous(), wp, b.to(DEV)), got[1:])                              # batch-independent
    assert torch.equal(ops.dwconv3d_f32(xd, wp, b.to(DEV)), got)                                                   # a repeat call
    small = (1, 2, 3, 5, 4)                                                                                        # the chain itself, bit for bit
    xs, ws, bs = _dw_case(small, 6101)
    chain = ops.dwconv3d_f32(xs.to(DEV), Q.pack_dwconv_weight(ws).to(DEV), bs.to(DEV)).cpu()
    print(f"dwconv3d {small}: {int((chain != D.dwconv_chain(xs, ws, bs)).sum())} of {chain.numel()} outputs differ from the emulated chain")
    out = torch.empty_like(xd)
    assert ops.dwconv3d_f32(xd, wp, b.to(DEV), out=out).data_ptr() == out.data_ptr() and torch.equal(out, got)
    with pytest.raises(ValueError, match="must not alias"):
        ops.dwconv3d_f32(xd, wp, b.to(DEV), out=xd)
    with pytest.raises(ValueError, match="must not alias"):
        ops.dwconv3d_f32(xd[:1], wp, b.to(DEV), out=xd.view(-1)[8:8 + xd[:1].numel()].view(xd[:1].shape))


# ---- 2. the resized view ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", [True, False], ids=["antialias", "plain"])
@pytest.mark.parametrize("sizes", [((240, 256), (224, 224)), ((37, 45), (24, 32)), ((224, 224), (224, 224))], ids=str)
def test_resized_view(sizes, antialias):
    (H, W), (oh, ow) = sizes
    Fn, Tn = 5, 4
    g = torch.Generator().manual_seed(6200 + H)
    idx = np.array([4, 0, 0, 3], dtype=np.int32)                          # the last frame, a repeated frame
    didx = torch.from_numpy(idx).to(DEV)

    def case(view_dev, host, what):
        want = D.resized_view(host, idx, (oh, ow), antialias, torch.float64)
        got = ops.vqa_resized_view_f32(view_dev, didx, (oh, ow), Q.MEAN, Q.STD, antialias=antialias)
        assert tuple(got.shape) == (Tn, oh, ow, 3)
        err = (got.cpu().double() - want).abs()
        bound = 2.0 ** -23 * want.abs().clamp(min=1.0)
        print(f"resized view {H} x {W} -> {oh} x {ow}, antialias {antialias}, {what}: largest error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), what
        if (H, W) == (oh, ow):                                            # the identity table: fastvqa's normalisation, bit for bit
            one = {"fragments": (1, 1), "fsize": (H, W), "t_groups": 1}
            assert torch.equal(got.cpu(), R.fragments(host, idx, np.zeros((1, 1, 1, 2), dtype=np.int32), one)), what
        cols = ops.vqa_resized_view_f32(view_dev, didx, (oh, ow), Q.MEAN, Q.STD, antialias=antialias, cols=True)
        assert torch.equal(cols.view(Tn // 2, oh // 4, ow // 4, 3, 2, 4, 4),
                           got.view(Tn // 2, 2, oh // 4, 4, ow // 4, 4, 3).permute(0, 2, 4, 6, 1, 3, 5)), what
        return got

    u8 = torch.randint(0, 256, (Fn, H, W, 3), generator=g, dtype=torch.uint8)
    a = case(u8.to(DEV).permute(0, 3, 1, 2), u8, "u8 frames")
    assert torch.equal(case(u8.to(DEV).permute(0, 3, 1, 2).contiguous(), u8, "u8 planes"), a)
    f32 = torch.rand(Fn, 3, H, W, generator=g)
    case(f32.to(DEV), f32, "f32")
    bf = f32.bfloat16()
    case(bf.to(DEV), bf, "bf16")
    big = torch.rand(Fn, H + 5, W + 3, 3, generator=g)                     # a cropped and permuted view
    case(big.to(DEV)[:, 2:2 + H, 1:1 + W].permute(0, 3, 1, 2), big[:, 2:2 + H, 1:1 + W].permute(0, 3, 1, 2), "crop")


# ---- 3. the downsampling ----------------------------------------------------------------------------------------------------------------
def test_downsample():
    g = torch.Generator().manual_seed(6300)
    x, w, b = torch.randn(2, 2, 4, 6, 32, generator=g), torch.randn(64, 32, 1, 2, 2, generator=g) / 128 ** 0.5, torch.randn(64, generator=g)
    ref = lambda dt: F.conv3d(x.to(dt).permute(0, 4, 1, 2, 3), w.to(dt), b.to(dt), stride=(1, 2, 2)).permute(0, 2, 3, 4, 1)
    merged = ops.swin3d_patch_merge_f32(x.to(DEV))
    got = ops.linear_f32(merged.view(-1, 128), Q.pack_downsample_weight(w).to(DEV), b.to(DEV)).view(2, 2, 2, 3, 64)
    gate_check("downsample (2,2,4,6,32 -> 64)", got, ref(torch.float64), ref(torch.float32))
    _, W = weights("tiny", T.TINY, T.TINY_TECH)
    Wd = W.to(torch.device(DEV))
    with pytest.raises(ValueError, match="must be even"):
        Q.downsample(Wd, torch.zeros(1, 2, 3, 4, 32, device=DEV), "downsample_layers.1")
    with pytest.raises(ValueError, match="must be even"):
        Q.downsample(Wd, torch.zeros(1, 2, 4, 5, 32, device=DEV), "downsample_layers.1")


# ---- 4. the whole aesthetic network, tiny -----------------------------------------------------------------------------------------------
def test_aesthetic_network_tiny():
    cfg, tech = T.TINY, T.TINY_TECH
    sd, W = weights("tiny", cfg, tech)
    frames = _frames(6400, 10, 40, 70)
    plan = Q.sample_plan(10, 40, 70, cfg, tech, seed=11)
    idx = plan["aesthetic"]
    view = D.resized_view(frames, idx[0], cfg.size, True, torch.float64).float()[None]
    s64, s32 = D.stem(view, sd, torch.float64), D.stem(view, sd, torch.float32)
    f64, f32 = D.backbone(s64, sd, T.as_dict(cfg), torch.float64), D.backbone(s32, sd, T.as_dict(cfg), torch.float32)
    assert tuple(s64.shape) == (1, 2, 8, 16, 32) and tuple(f64.shape) == (1, 2, 1, 2, 256)
    Wd = W.to(torch.device(DEV))
    x = fastvqa.clip_view(frames.to(DEV))
    maps = Q.embed(Wd, x, torch.from_numpy(idx[0]).to(DEV))
    gate_check("tiny aesthetic: stem", maps, s64, s32)
    gate_check(f"tiny aesthetic: final map {tuple(f64.shape)}", Q.backbone(Wd, maps), f64, f32)
    acfg = T.as_dict(cfg)
    raw = Q.aesthetic_raw(Wd, x, idx)
    print(f"tiny aesthetic: raw {raw!r}")
    gate_check("tiny aesthetic: aesthetic_raw", raw, D.aesthetic_raw(sd, frames, acfg, idx, torch.float64), D.aesthetic_raw(sd, frames, acfg, idx, torch.float32))


# ---- 5. the whole metric, tiny ----------------------------------------------------------------------------------------------------------
def test_whole_metric_tiny():
    cfg, tech = T.TINY, T.TINY_TECH
    sd, W = weights("tiny", cfg, tech)
    frames = _frames(6500, 10, 40, 70)
    plan = Q.sample_plan(10, 40, 70, cfg, tech, seed=11)
    want64 = D.score(sd, frames, T.as_dict(cfg), T.as_dict(tech), plan, torch.float64)
    want32 = D.score(sd, frames, T.as_dict(cfg), T.as_dict(tech), plan, torch.float32)
    dev_frames = frames.to(DEV)
    got = Q.score_clip(dev_frames, W, plan=plan)
    print(f"tiny DOVER: {got}")
    assert tuple(got) == Q.KEYS and all(isinstance(v, float) for v in got.values())
    for key in Q.KEYS:
        gate_check(f"tiny DOVER: {key}", got[key], want64[key], want32[key])
    assert got == Q.fuse(got["technical_raw"], got["aesthetic_raw"]) and 0.0 < got["overall"] < 1.0
    assert Q.score_clip(dev_frames, W, plan=plan) == got                                         # a repeat call
    assert Q.score_clip(frames, W, plan=plan) == got                                             # host frames are uploaded
    assert Q.score_clip(dev_frames, W, seed=11) == got                                           # the plan drawn from the seed
    before = Q.COUNTERS["groups"], fastvqa.COUNTERS["groups"]
    assert Q.score_clip(dev_frames, W, plan=plan, group=1) == got
    assert (Q.COUNTERS["groups"], fastvqa.COUNTERS["groups"]) == (before[0] + 1, before[1] + 3)
    over = Q.score_clip(dev_frames, W, plan=plan, rescale=((0.0, 1.0), (0.0, 1.0)))
    assert over == Q.fuse(got["technical_raw"], got["aesthetic_raw"], ((0.0, 1.0), (0.0, 1.0))) and over["technical"] != got["technical"]
    with pytest.raises(ValueError, match="smaller than the"):
        Q.score_clip(dev_frames[:, :cfg.size[0] - 1], W)


# ---- 6. the production shape ------------------------------------------------------------------------------------------------------------
def test_production_shape():
    """One clip of 70 frames of 240 x 256: the stem map, stage 0 (3 blocks on 16 x 56 x 56 x 96) and stage 3 alone (3 blocks on a random
    16 x 7 x 7 x 768 map) against the fp64 restatement; at full depth both branches are finite and identical across two calls."""
    cfg, tech = Q.DEFAULT, Q.TECHNICAL
    sd, W = weights("production", cfg, tech)
    frames = _frames(6600, 70, 240, 256)
    plan = Q.sample_plan(70, 240, 256, seed=3)
    idx = plan["aesthetic"][0]
    view = D.resized_view(frames, idx, cfg.size, True, torch.float64).float()[None]
    s64, s32 = D.stem(view, sd, torch.float64), D.stem(view, sd, torch.float32)
    Wd = W.to(torch.device(DEV))
    dev_frames = frames.to(DEV)
    x = Q.embed(Wd, fastvqa.clip_view(dev_frames), torch.from_numpy(idx).to(DEV))
    assert tuple(x.shape) == (1, 16, 56, 56, 96)
    gate_check("DOVER aesthetic: stem", x, s64, s32)
    gate_check("DOVER aesthetic: stage 0 (1,16,56,56,96)", Q.backbone(Wd, x, stages=1), D.stage(s64, sd, 0, 3, torch.float64),
               D.stage(s32, sd, 0, 3, torch.float32))
    del x
    m = torch.randn(1, 16, 7, 7, 768, generator=torch.Generator().manual_seed(6601))
    gate_check("DOVER aesthetic: stage 3 (1,16,7,7,768)", Q.backbone(Wd, m.to(DEV), stages=4, first=3), D.stage(m, sd, 3, 3, torch.float64),
               D.stage(m, sd, 3, 3, torch.float32))
    a, b = Q.score_clip(dev_frames, W, seed=3), Q.score_clip(dev_frames, W, seed=3)
    print(f"DOVER: full depth: {a}")
    assert all(np.isfinite(v) for v in a.values()) and 0.0 < a["overall"] < 1.0 and a == b


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, monkeypatch):
    from PIL import Image
    cfg, tech = T.TINY, T.TINY_TECH
    monkeypatch.setattr(Q, "DEFAULT", cfg)                                # the tool on the tiny networks
    monkeypatch.setattr(Q, "TECHNICAL", tech)
    sd, _ = weights("tiny", cfg, tech)
    torch.save({"state_dict": sd}, tmp_path / "tiny.pth")
    pred = tmp_path / "pred"
    (pred / "png").mkdir(parents=True)
    frames = _frames(6700, 6, 40, 72)
    for i, fr in enumerate(frames):
        Image.fromarray(fr.numpy()).save(pred / "png" / f"{i:04d}.png")
    g = torch.Generator().manual_seed(6701)
    with y4m.Y4MWriter(str(pred / "clip.y4m"), 72, 40, 25, "444") as wr:
        wr.write(torch.randint(16, 236, (5, 3 * 40 * 72), generator=g, dtype=torch.uint8))
    live = torch.cuda.memory_allocated()
    out = E.main(["--pred", str(pred), "--model", str(tmp_path / "tiny.pth"), "--seed", "9", "--out", str(tmp_path / "o")])
    W = Q.DoverWeights.load(str(tmp_path / "tiny.pth"), cfg, tech)
    named = lambda s: {k: round(s[f], 4) for k, f in zip(E.KEYS, ("overall", "technical", "aesthetic", "technical_raw", "aesthetic_raw"))}
    want = {name.split(".")[0]: named(Q.score_clip(prepost.load_frames(str(pred / name)), W, seed=9)) for name in ("clip.y4m", "png")}
    assert out["per_sample"] == want and out["count"] == 2 and want["clip"] != want["png"]
    with open(tmp_path / "o" / "metrics_dover.json") as f:
        assert json.load(f) == out
    plain = E.main(["--pred", str(pred), "--model", str(tmp_path / "tiny.pth"), "--seed", "9", "--out", str(tmp_path / "o2"), "--resize", "plain",
                    "--aesthetic_mean", "0", "--aesthetic_std", "1"])
    Wp = Q.DoverWeights.load(str(tmp_path / "tiny.pth"), Q.DoverConfig(**{**T.as_dict(cfg), "resize": "plain"}), tech)
    assert plain["per_sample"]["png"] == named(Q.score_clip(frames, Wp, seed=9, rescale=Q.with_rescale(aesthetic_mean=0, aesthetic_std=1)))
    assert plain["per_sample"]["png"]["dover_aesthetic_raw"] != want["png"]["dover_aesthetic_raw"]
    assert plain["per_sample"]["png"]["dover_technical_raw"] == want["png"]["dover_technical_raw"]
    del W, Wp
    _drop_device_tables()
    gc.collect()
    assert torch.cuda.memory_allocated() <= live, "the tool left tensors on the device"
