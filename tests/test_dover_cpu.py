"""DOVER without a GPU (dove_amd/dover.py, dove_amd/eval_dover.py): the sampling plan against the restatement (tests/dover_ref.py), the
resize tap tables against F.interpolate in fp64, the packing and the loader, the fusion, the command line's JSON and refusals, and the new
exports."""
import dataclasses
import json
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dover_ref as D
import test_fastvqa_cpu as T
from dove_amd import dover as Q
from dove_amd import eval_dover as E
from dove_amd import lib as L
from dove_amd import ops

CFG = Q.DoverConfig()
# The tiny networks of the GPU tests.  Aesthetic: a 4 x 32 x 64 view, maps 2 x 8 x 16 -> 2 x 4 x 8 -> 2 x 2 x 4 -> 2 x 1 x 2 (the last stage
# is all padding).  Technical: test_fastvqa_cpu.TINY_B with 3 clips.
TINY = Q.DoverConfig(size=(32, 64), clip_len=4, t_frag=4, width=32, depths=(1, 1, 2, 1), head_hidden=16)
TINY_TECH = dataclasses.replace(T.TINY_B, name="tiny-technical", num_clips=3)


def as_dict(cfg):
    return dataclasses.asdict(cfg)


# ---- the sampling plan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_frames", [1, 8, 33, 64, 65, 100])
@pytest.mark.parametrize("hw", [(224, 224), (720, 1280), (1280, 720)], ids=lambda s: "%dx%d" % s)
def test_plan_is_seeded_in_range_and_equals_the_restatement(num_frames, hw):
    H, W = hw
    tech = Q.TECHNICAL
    plan, again = Q.sample_plan(num_frames, H, W, seed=7), Q.sample_plan(num_frames, H, W, CFG, tech, seed=7)
    (idx, org), view = plan["technical"], plan["aesthetic"]
    assert np.array_equal(idx, again["technical"][0]) and np.array_equal(org, again["technical"][1]) and np.array_equal(view, again["aesthetic"])
    assert idx.dtype == np.int32 and idx.shape == (3, 32) and idx.min() >= 0 and idx.max() < num_frames
    assert view.dtype == np.int32 and view.shape == (1, 32) and view.min() >= 0 and view.max() < num_frames
    assert org.dtype == np.int32 and org.shape == (3, 7, 7, 1, 2)
    assert org.min() >= 0 and (org[..., 0] + 32).max() <= H and (org[..., 1] + 32).max() <= W
    if num_frames <= 64:                                                    # no room for a random start: the technical clips start at 0
        assert (idx[:, 0] == 0).all() and np.array_equal(idx[0], 2 * np.arange(32) % num_frames)
    else:
        assert (idx[:, 0] < num_frames - 64).all() and all((np.diff(row) == 2).all() for row in idx)
    draws = Q.sample_draws(num_frames, H, W, CFG, tech, 7)
    ref = D.plan_from_draws(num_frames, H, W, as_dict(CFG), as_dict(tech), draws)
    assert np.array_equal(idx, ref["technical"][0]) and np.array_equal(org, ref["technical"][1]) and np.array_equal(view, ref["aesthetic"])
    fed = Q.sample_plan(num_frames, H, W, draws=draws)
    assert np.array_equal(fed["technical"][0], idx) and np.array_equal(fed["aesthetic"], view)


def test_plan_draws_move_with_the_seed():
    a, b = Q.sample_plan(200, 720, 1280, seed=1), Q.sample_plan(200, 720, 1280, seed=2)
    assert not np.array_equal(a["technical"][0], b["technical"][0]) and not np.array_equal(a["technical"][1], b["technical"][1])
    assert not np.array_equal(a["aesthetic"], b["aesthetic"])
    assert len(set(a["technical"][0][:, 0].tolist())) > 1                   # one start per clip, not one for all
    cells = a["aesthetic"][0] - 200 // 32 * np.arange(32)                   # 32 cells of 6 frames, starts in [0, 4)
    assert cells.min() >= 0 and cells.max() < 4 and len(np.unique(cells)) > 1
    tiny = Q.sample_plan(10, 40, 70, TINY, TINY_TECH, seed=3)
    assert tiny["aesthetic"].shape == (1, 4) and tiny["technical"][0].shape == (3, 8) and tiny["technical"][1].shape == (3, 7, 7, 1, 2)


# ---- the tap tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", [True, False], ids=["antialias", "plain"])
@pytest.mark.parametrize("sizes", [((240, 256), (224, 224)), ((720, 1280), (224, 224)), ((224, 224), (224, 224)), ((37, 45), (24, 24)),
                                   ((20, 20), (24, 24))], ids=str)
def test_tap_tables_equal_interpolate(sizes, antialias):
    (H, W), (oh, ow) = sizes

    def matrix(n_in, n_out):
        t = ops.resize_taps(n_in, n_out, antialias)
        assert t["first"].min() >= 0 and (t["first"] + t["count"]).max() <= n_in and t["count"].min() >= 1 and t["weights"].shape == (n_out, t["max"])
        M = np.zeros((n_out, n_in))
        for i in range(n_out):
            M[i, t["first"][i]:t["first"][i] + t["count"][i]] = t["weights"][i, :t["count"][i]]
        assert np.abs(M.sum(1) - 1.0).max() < 1e-15
        return M

    My, Mx = matrix(H, oh), matrix(W, ow)
    if (H, W) == (oh, ow):
        assert np.array_equal(My, np.eye(H)) and ops.resize_taps(H, oh, antialias)["max"] == 1
    x = torch.rand(2, 3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(H + W))
    want = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False, antialias=antialias).numpy()
    got = My @ x.numpy() @ Mx.T
    err = np.abs(got - want).max()
    print(f"{H} x {W} -> {oh} x {ow}, antialias {antialias}: {ops.resize_taps(H, oh, antialias)['max']} x "
          f"{ops.resize_taps(W, ow, antialias)['max']} taps, error {err:.3e}")
    assert err <= 1e-14


# ---- packing and the loader -------------------------------------------------------------------------------------------------------------
def test_packing_and_loader(tmp_path):
    sd = Q.random_state(TINY, 3, TINY_TECH)
    assert tuple(sd["aesthetic_backbone.downsample_layers.0.0.weight"].shape) == (32, 3, 2, 4, 4)
    assert tuple(sd["aesthetic_backbone.downsample_layers.2.1.weight"].shape) == (128, 64, 1, 2, 2)
    assert tuple(sd["aesthetic_backbone.stages.2.1.dwconv.weight"].shape) == (128, 1, 3, 7, 7)
    assert tuple(sd["aesthetic_head.fc_hid.weight"].shape) == (16, 256, 1, 1, 1)
    assert "technical_backbone.layers.0.blocks.1.attn.fragment_position_bias_table" in sd and "technical_head.fc_last.bias" in sd
    assert float(sd["aesthetic_backbone.stages.0.0.gamma"].min()) >= 0.5                       # every block changes the map
    torch.save({"state_dict": sd}, tmp_path / "w.pth")
    W = Q.DoverWeights.load(str(tmp_path / "w.pth"), TINY, TINY_TECH)
    P = W.params
    # the depthwise weight is tap-major
    dw = sd["aesthetic_backbone.stages.1.0.dwconv.weight"]
    assert tuple(P["stages.1.0.dwconv.weight"].shape) == (3, 7, 7, 64)
    assert torch.equal(P["stages.1.0.dwconv.weight"][2, 5, 1], dw[:, 0, 2, 5, 1])
    # the downsample weight's blocks follow swin3d_patch_merge: chunk j of a merged pixel is input pixel (j & 1, j >> 1)
    ds = sd["aesthetic_backbone.downsample_layers.1.1.weight"]
    packed = P["downsample_layers.1.1.weight"]
    assert tuple(packed.shape) == (1, 1, 128, 64)
    for j in range(4):
        assert torch.equal(packed[0, 0, 32 * j:32 * (j + 1)], ds[:, :, 0, j & 1, j >> 1].t())
    x = torch.randn(1, 1, 2, 2, 32, dtype=torch.float64)
    merged = torch.cat([x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]], -1)          # the merge's order
    want = F.conv3d(x.permute(0, 4, 1, 2, 3), ds.double(), stride=(1, 2, 2)).flatten()
    assert float((merged.flatten() @ packed[0, 0].double() - want).abs().max()) < 1e-12
    # gamma is folded into pwconv2
    g = sd["aesthetic_backbone.stages.2.1.gamma"]
    assert torch.equal(P["stages.2.1.pwconv2.weight"][0, 0], (sd["aesthetic_backbone.stages.2.1.pwconv2.weight"] * g[:, None]).t())
    assert torch.equal(P["stages.2.1.pwconv2.bias"], sd["aesthetic_backbone.stages.2.1.pwconv2.bias"] * g)
    assert "stages.2.1.gamma" not in P
    assert torch.equal(P["stages.0.0.pwconv1.weight"][0, 0], sd["aesthetic_backbone.stages.0.0.pwconv1.weight"].t())
    assert torch.equal(P["downsample_layers.0.0.weight"][0, 0], sd["aesthetic_backbone.downsample_layers.0.0.weight"].flatten(1).t())
    assert tuple(P["aesthetic_head.fc_hid.weight"].shape) == (16, 256) and tuple(P["aesthetic_head.fc_last.weight"].shape) == (16,)
    # the renamed technical keys reach VqaWeights
    tw = W.technical()
    assert isinstance(tw, Q.VqaWeights) and tw.cfg == TINY_TECH
    assert torch.equal(tw.params["layers.1.blocks.0.attn.qkv.weight"][0, 0], sd["technical_backbone.layers.1.blocks.0.attn.qkv.weight"].t())
    assert torch.equal(tw.params["vqa_head.fc_hid.weight"], sd["technical_head.fc_hid.weight"].flatten(1))
    # refusals, by name
    for name, pattern in (("aesthetic_backbone.stages.2.0.gamma", r"aesthetic_backbone\.stages\.2\.0\.gamma is missing"),
                          ("technical_head.fc_hid.weight", r"technical_head\.fc_hid\.weight is missing")):
        bad = dict(sd)
        del bad[name]
        with pytest.raises(ValueError, match=pattern):
            Q.DoverWeights.from_state_dict(bad, TINY, TINY_TECH)
    bad = dict(sd)
    bad["aesthetic_backbone.stages.3.0.dwconv.weight"] = torch.zeros(256, 1, 3, 3, 3)
    with pytest.raises(ValueError, match=r"stages\.3\.0\.dwconv\.weight has shape \(256, 1, 3, 3, 3\)"):
        Q.DoverWeights.from_state_dict(bad, TINY, TINY_TECH)
    with pytest.raises(ValueError, match="has shape"):                                          # a tiny file is no DOVER checkpoint
        Q.DoverWeights.from_state_dict(sd)


def test_configuration():
    assert (CFG.size, CFG.clip_len, CFG.frame_interval, CFG.t_frag, CFG.num_clips) == ((224, 224), 32, 2, 32, 1)
    assert (CFG.width, CFG.depths, CFG.head_hidden, CFG.resize, CFG.dims) == (96, (3, 3, 9, 3), 64, "antialias", (96, 192, 384, 768))
    t = Q.TECHNICAL
    assert (t.fragments, t.fsize, t.clip_len, t.frame_interval, t.t_groups, t.num_clips, t.window) == ((7, 7), (32, 32), 32, 2, 1, 3, (8, 7, 7))
    shapes = Q.param_shapes()
    assert shapes["aesthetic_backbone.stages.2.8.dwconv.weight"] == (384, 1, 3, 7, 7) and shapes["aesthetic_backbone.stages.3.2.gamma"] == (768,)
    assert shapes["aesthetic_backbone.downsample_layers.3.1.weight"] == (768, 384, 1, 2, 2)
    assert shapes["technical_backbone.layers.0.blocks.0.attn.relative_position_bias_table"] == (15 * 13 * 13, 3)
    assert shapes["technical_head.fc_hid.weight"] == (64, 768, 1, 1, 1) and shapes["aesthetic_head.fc_hid.weight"] == (64, 768, 1, 1, 1)
    with pytest.raises(ValueError, match="choose antialias or plain"):
        Q.DoverConfig(resize="bicubic")
    with pytest.raises(ValueError, match="halves evenly"):
        Q.DoverConfig(size=(224, 220))
    assert Q.group_size(CFG) >= 1 and Q.group_size(CFG, budget=1) == 1
    for fn in (lambda: Q.sample_plan(10, 223, 400), lambda: Q.sample_plan(10, 400, 200)):
        with pytest.raises(ValueError, match="smaller than the 224 x 224"):
            fn()
    with pytest.raises(ValueError, match="at least one frame"):
        Q.sample_plan(0, 400, 400)


# ---- the fusion -------------------------------------------------------------------------------------------------------------------------
def test_fusion_and_overrides():
    assert Q.RESCALE == ((0.1107, 0.07355), (-0.08285, 0.03774)) and Q.FUSION == (0.6104, 0.3896)
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))
    out = Q.fuse(0.2, -0.05)
    t, a = (0.2 - 0.1107) / 0.07355, (-0.05 + 0.08285) / 0.03774
    assert out == {"technical_raw": 0.2, "aesthetic_raw": -0.05, "technical": sig(t), "aesthetic": sig(a), "overall": sig(0.6104 * t + 0.3896 * a)}
    assert out == D.fuse(0.2, -0.05) and tuple(out) == Q.KEYS
    assert Q.fuse(0.1107, -0.08285) == {"technical_raw": 0.1107, "aesthetic_raw": -0.08285, "technical": 0.5, "aesthetic": 0.5, "overall": 0.5}
    over = Q.with_rescale(None, 0.5, 1.0, None)
    assert over == ((0.1107, 0.5), (1.0, 0.03774))
    assert Q.fuse(0.2, -0.05, over)["technical"] == sig((0.2 - 0.1107) / 0.5) and Q.fuse(0.2, -0.05, over)["aesthetic"] == sig(-1.05 / 0.03774)
    assert Q.fuse(0.3, 0.4, ((0.0, 1.0), (0.0, 1.0)))["overall"] == sig(0.6104 * 0.3 + 0.3896 * 0.4)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _pred(tmp_path):
    from PIL import Image
    pred = tmp_path / "pred"
    (pred / "a").mkdir(parents=True)
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (8, 10, 3), dtype=np.uint8)).save(pred / "a" / f"{i:03d}.png")
    np.save(pred / "b.npy", rng.integers(0, 256, (3, 8, 10, 3), dtype=np.uint8))
    (pred / "notes.txt").write_text("not a clip")
    return pred


def test_process_writes_the_json(tmp_path):
    pred = _pred(tmp_path)
    seen = []

    def stub(frames):
        seen.append(tuple(frames.shape))
        if frames.shape[0] == 3:
            return {"overall": 0.654321, "technical": 0.7, "aesthetic": 0.61239, "technical_raw": 0.12344, "aesthetic_raw": -0.05}
        return {"overall": 0.11111, "technical": 0.2, "aesthetic": 0.3, "technical_raw": -0.2, "aesthetic_raw": -0.15}

    out = E.main(["--pred", str(pred), "--model", "unused.pth", "--out", str(tmp_path / "o")], score_fn=stub)
    assert seen == [(2, 8, 10, 3), (3, 8, 10, 3)]
    assert out == {"per_sample": {"a": {"dover": 0.1111, "dover_technical": 0.2, "dover_aesthetic": 0.3, "dover_technical_raw": -0.2,
                                        "dover_aesthetic_raw": -0.15},
                                  "b": {"dover": 0.6543, "dover_technical": 0.7, "dover_aesthetic": 0.6124, "dover_technical_raw": 0.1234,
                                        "dover_aesthetic_raw": -0.05}},
                   "average": {"dover": 0.3827, "dover_technical": 0.45, "dover_aesthetic": 0.4562, "dover_technical_raw": -0.0383,
                               "dover_aesthetic_raw": -0.1},
                   "count": 2}
    with open(tmp_path / "o" / "metrics_dover.json") as f:
        assert json.load(f) == out


def test_flags_and_refusals(tmp_path, monkeypatch, capsys):
    args = E.build_parser().parse_args(["--pred", "x", "--model", "m"])
    assert (args.seed, args.resize, args.out, args.technical_mean, args.technical_std, args.aesthetic_mean, args.aesthetic_std) == \
        (42, "antialias", "", None, None, None, None)
    got = {}

    def fake_process(pred, out, model, seed, score_fn, resize, rescale):
        got.update(pred=pred, out=out, model=model, seed=seed, resize=resize, rescale=rescale)
        return {}

    monkeypatch.setattr(E, "process", fake_process)
    E.main(["--pred", "p", "--model", "m.pth", "--seed", "9", "--resize", "plain", "--technical_mean", "0.5", "--aesthetic_std", "2"])
    assert got == {"pred": "p", "out": "p", "model": "m.pth", "seed": 9, "resize": "plain", "rescale": ((0.5, 0.07355), (-0.08285, 2.0))}
    monkeypatch.undo()
    for argv, msg in ((["--pred", "x", "--model", "m", "--resize", "bicubic"], "choose antialias or plain"),
                      (["--pred", "x", "--model", "m", "--technical_std", "0"], "--technical_std must be positive"),
                      (["--pred", "x", "--model", "m", "--aesthetic_std", "-1"], "--aesthetic_std must be positive"),
                      (["--pred", "x"], "--model")):
        with pytest.raises(SystemExit):
            E.main(argv)
        assert msg in capsys.readouterr().err
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no HIP device is visible"):
        E.make_score_fn(str(tmp_path / "none.pth"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(FileNotFoundError, match="checkpoint is not shipped; pass your own file"):
        E.make_score_fn(str(tmp_path / "none.pth"))
    # a clip below the view is reported with the reason and leaves no entry
    pred = tmp_path / "pred"
    pred.mkdir()
    np.save(pred / "small.npy", np.zeros((2, 100, 300, 3), dtype=np.uint8))

    def plan_only(frames):
        Q.sample_plan(frames.shape[0], frames.shape[1], frames.shape[2])
        return Q.fuse(0.0, 0.0)

    out = E.process(str(pred), str(tmp_path / "o"), score_fn=plan_only)
    assert out["count"] == 0 and "smaller than the 224 x 224" in capsys.readouterr().out


# ---- the library ------------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ("dove_dwconv3d_f32", "dove_dwconv3d_tile", "dove_vqa_resized_view_f32")


def test_exports_and_argument_checks():
    """The header declares the new entry points, lib.py binds them, the library built for gfx950 exports them, and each refuses bad
    arguments before any HIP call."""
    import os

    import test_abi
    assert set(NEW_EXPORTS) <= set(test_abi.header_symbols())
    assert {"dove_dwconv3d_f32", "dove_vqa_resized_view_f32"} <= set(L.SIGNATURES) and "dove_dwconv3d_tile" in L.PLAIN
    with open(os.path.join(test_abi.ROOT, "dove_amd", "csrc", "build.sh")) as f:
        assert re.search(r'SRCS="[^"]*\bconvnext3d\b', f.read())
    if not os.path.exists(L.LIB_PATH):                                      # hipcc --offload-arch=gfx950 needs no GPU
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    assert lib.dove_abi_version() == 15
    assert lib.dove_dwconv3d_f32(None, 1, 1, 1, 1, 4, None, None, None, None) == -1 and b"dove_dwconv3d_f32" in lib.dove_last_error()
    assert lib.dove_vqa_resized_view_f32(None, 1, 8, 8, None, 2, None, None, 1, None, None, 1, 8, 8, None, None, 0, None, None) == -1
    assert b"dove_vqa_resized_view_f32" in lib.dove_last_error()
    # the tile is one function of the shape: at most 16 rows, balanced; 7 or 8 columns, whichever wastes fewer
    assert [ops.dwconv3d_tile(h, h) for h in (56, 28, 14, 7)] == [(14, 8), (14, 7), (14, 7), (7, 7)]
    assert ops.dwconv3d_tile(1, 1) == (1, 7) and ops.dwconv3d_tile(17, 15) == (9, 8) and ops.dwconv3d_tile(16, 8) == (16, 8)
