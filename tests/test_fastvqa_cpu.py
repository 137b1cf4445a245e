"""FasterVQA / FAST-VQA without a GPU (dove_amd/fastvqa.py, dove_amd/eval_fastvqa.py): the sampling plan and the host geometry against
the restatement (tests/fastvqa_ref.py), the loader, the command line's JSON and refusals, and the new exports."""
import dataclasses
import json
import re

import numpy as np
import pytest
import torch

import fastvqa_ref as R
from dove_amd import eval_fastvqa as E
from dove_amd import fastvqa as Q
from dove_amd import lib as L

FASTER, FAST = Q.preset("FasterVQA"), Q.preset("FAST-VQA")
# The tiny networks of the GPU tests: width 32, heads of 32.  A: an 8 x 32 x 32 canvas (2 x 2 fragments of 16 x 16, two temporal groups),
# window (2,2,2).  B: an 8 x 28 x 28 canvas (7 x 7 fragments of 4 x 4), window (2,4,4): the 7 x 7 map is padded to 8, merged from odd sizes,
# and the later stages clamp the window.
TINY = dict(width=32, depths=(2, 2, 2, 2), heads=(1, 2, 4, 8), clip_len=8, head_hidden=16)
TINY_A = Q.VqaConfig(name="tiny-A", fragments=(2, 2), fsize=(16, 16), t_groups=2, window=(2, 2, 2), **TINY)
TINY_B = Q.VqaConfig(name="tiny-B", fragments=(7, 7), fsize=(4, 4), t_groups=1, num_clips=2, frame_interval=1, window=(2, 4, 4), **TINY)


def as_dict(cfg):
    return dataclasses.asdict(cfg)


# ---- the sampling plan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [FASTER, FAST, TINY_A, TINY_B], ids=lambda c: c.name)
@pytest.mark.parametrize("num_frames", [1, 8, 33, 100])
def test_plan_is_seeded_in_range_and_equals_the_restatement(cfg, num_frames):
    Hc, Wc = cfg.canvas
    for H, W in ((Hc, Wc), (Hc + 1, Wc + 1), (720, 1280), (1280, 720)):
        idx, org = Q.sample_plan(num_frames, H, W, cfg, seed=7)
        again = Q.sample_plan(num_frames, H, W, cfg, seed=7)
        assert np.array_equal(idx, again[0]) and np.array_equal(org, again[1])
        assert idx.dtype == np.int32 and idx.shape == (cfg.num_clips, cfg.clip_len) and idx.min() >= 0 and idx.max() < num_frames
        assert org.dtype == np.int32 and org.shape == (cfg.num_clips,) + cfg.fragments + (cfg.t_groups, 2)
        assert org.min() >= 0 and (org[..., 0] + cfg.fsize[0]).max() <= H and (org[..., 1] + cfg.fsize[1]).max() <= W
        draws = Q.sample_draws(num_frames, H, W, cfg, 7)
        ridx, rorg = R.plan_from_draws(num_frames, H, W, as_dict(cfg), draws)
        assert np.array_equal(idx, ridx) and np.array_equal(org, rorg)
        fed = Q.sample_plan(num_frames, H, W, cfg, draws=draws)
        assert np.array_equal(fed[0], idx) and np.array_equal(fed[1], org)


def test_plan_draws_move_with_the_seed_and_wrap():
    a, b = Q.sample_plan(100, 720, 1280, FASTER, seed=1), Q.sample_plan(100, 720, 1280, FASTER, seed=2)
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    span = 720 // 7 - 32
    assert len(np.unique(a[1][..., 0] - np.minimum(720 // 7 * np.arange(7), 720 - 32)[None, :, None, None])) > span // 2   # the offsets spread
    idx, _ = Q.sample_plan(8, 720, 1280, FASTER, seed=1)                       # 8 frames: every group starts at its own frame and wraps
    assert idx[0].tolist() == [(g + 2 * k) % 8 for g in range(8) for k in range(4)]
    idx, _ = Q.sample_plan(200, 720, 1280, FAST, seed=1)                       # four evenly spaced clips of consecutive-interval-2 frames
    assert all((np.diff(row) == 2).all() for row in idx) and idx[:, 0].tolist() == [17, 51, 86, 120]


# ---- the host geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(4, 8, 8), (16, 7, 7), (2, 7, 5)], ids=str)
@pytest.mark.parametrize("window", [(4, 4, 4), (8, 7, 7), (2, 3, 3)], ids=str)
@pytest.mark.parametrize("shifted", [False, True])
def test_geometry_equals_the_restatement(dims, window, shifted):
    grid = (7, 7)
    geo = Q.geometry(dims, window, grid, shifted)
    ws, ss = R.get_window_size(dims, window, tuple(w // 2 for w in window) if shifted else (0, 0, 0))
    padded = R.padded_size(dims, ws)
    assert geo["window"] == ws and geo["shift"] == ss and geo["padded"] == padded
    N = ws[0] * ws[1] * ws[2]
    assert geo["length"] == N and geo["windows"] == padded[0] * padded[1] * padded[2] // N
    assert np.array_equal(geo["index"], R.relative_position_index(window)[:N, :N].numpy())
    assert geo["index"].max() < (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1) and geo["index"].min() >= 0
    assert np.array_equal(geo["frag"], R.fragment_ids(*padded, grid, ws, ss).numpy())
    if any(ss):
        want = R.compute_mask(*padded, ws, ss).numpy()                         # [nW,N,N]: 0 or -100
        reg = geo["region"]
        got = np.where(reg[:, None, :] != reg[:, :, None], R.MASK_VALUE, 0.0)
        assert np.array_equal(got, want)
    else:
        assert geo["region"] is None
    # the window gather's slot order is the restatement's partition of the padded, rolled map
    pos = torch.arange(padded[0] * padded[1] * padded[2]).view(1, *padded, 1)
    rolled = torch.roll(pos, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
    want = R.window_partition(rolled, ws).squeeze(-1).numpy()
    counts = [p // w for p, w in zip(padded, ws)]
    a, n = np.arange(geo["windows"])[:, None], np.arange(N)[None, :]
    p = [((a // (counts[1] * counts[2])) * ws[0] + n // (ws[1] * ws[2]) + ss[0]) % padded[0],
         (((a // counts[2]) % counts[1]) * ws[1] + (n // ws[2]) % ws[1] + ss[1]) % padded[1],
         ((a % counts[2]) * ws[2] + n % ws[2] + ss[2]) % padded[2]]
    assert np.array_equal((p[0] * padded[1] + p[1]) * padded[2] + p[2], want)


# ---- the loader -------------------------------------------------------------------------------------------------------------------------
def test_loader_maps_the_published_names(tmp_path):
    sd = Q.random_state(TINY_B, 3)
    assert "fragments_backbone.layers.0.blocks.1.attn.fragment_position_bias_table" in sd
    assert "fragments_backbone.layers.3.blocks.0.attn.fragment_position_bias_table" not in sd
    assert tuple(sd["vqa_head.fc_hid.weight"].shape) == (16, 256, 1, 1, 1) and tuple(sd["vqa_head.fc_last.weight"].shape) == (1, 16, 1, 1, 1)
    sd["fragments_backbone.layers.0.blocks.0.attn.relative_position_index"] = torch.zeros(32, 32, dtype=torch.long)     # a buffer: ignored
    torch.save({"state_dict": sd}, tmp_path / "w.pth")
    W = Q.VqaWeights.load(str(tmp_path / "w.pth"), TINY_B)
    P = W.params
    assert torch.equal(P["layers.1.blocks.0.attn.qkv.weight"][0, 0], sd["fragments_backbone.layers.1.blocks.0.attn.qkv.weight"].t())
    assert torch.equal(P["patch_embed.proj.weight"][0, 0], sd["fragments_backbone.patch_embed.proj.weight"].flatten(1).t())
    assert tuple(P["layers.0.downsample.reduction.weight"].shape) == (1, 1, 128, 64)
    assert torch.equal(P["layers.0.blocks.0.attn.fragment_position_bias_table"],
                       sd["fragments_backbone.layers.0.blocks.0.attn.fragment_position_bias_table"])
    assert tuple(P["vqa_head.fc_hid.weight"].shape) == (16, 256) and tuple(P["vqa_head.fc_last.weight"].shape) == (16,)
    bad = dict(sd)
    bad["fragments_backbone.layers.2.blocks.1.attn.fragment_position_bias_table"] = torch.zeros(5, 4)
    with pytest.raises(ValueError, match=r"layers\.2\.blocks\.1\.attn\.fragment_position_bias_table has shape \(5, 4\)"):
        Q.VqaWeights.from_state_dict(bad, TINY_B)
    del bad["fragments_backbone.layers.2.blocks.1.attn.fragment_position_bias_table"]
    with pytest.raises(ValueError, match="fragment_position_bias_table is missing"):
        Q.VqaWeights.from_state_dict(bad, TINY_B)
    with pytest.raises(ValueError, match="patch_embed.proj.weight has shape"):       # a tiny file is no FasterVQA checkpoint
        Q.VqaWeights.from_state_dict(sd, "FasterVQA")


def test_presets():
    assert FASTER.canvas == (224, 224) and FAST.canvas == (224, 224) and FASTER.dims == (96, 192, 384, 768)
    assert (FASTER.t_groups, FASTER.num_clips, FASTER.window) == (8, 1, (4, 4, 4)) and (FAST.t_groups, FAST.num_clips, FAST.window) == (1, 4, (8, 7, 7))
    assert FASTER.rescale == (0.14759505, 0.03613452) and FAST.rescale == (-0.110198185, 0.04178565)
    assert Q.with_rescale(FAST, None, 0.5) == (-0.110198185, 0.5)
    shapes = Q.param_shapes(FAST)
    assert shapes["fragments_backbone.layers.0.blocks.0.attn.relative_position_bias_table"] == (15 * 13 * 13, 3)
    assert shapes["vqa_head.fc_hid.weight"] == (64, 768, 1, 1, 1)
    with pytest.raises(ValueError, match="unknown variant"):
        Q.preset("DOVER")
    with pytest.raises(ValueError, match="32 wide"):
        Q.VqaConfig(width=64)
    assert Q.group_size(FASTER) >= 4 and Q.group_size(FASTER, budget=1) == 1


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_process_writes_the_json(tmp_path):
    from PIL import Image
    pred = tmp_path / "pred"
    (pred / "a").mkdir(parents=True)
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (8, 10, 3), dtype=np.uint8)).save(pred / "a" / f"{i:03d}.png")
    np.save(pred / "b.npy", rng.integers(0, 256, (3, 8, 10, 3), dtype=np.uint8))
    (pred / "notes.txt").write_text("not a clip")
    seen = []

    def stub(frames):
        seen.append(tuple(frames.shape))
        if frames.shape[0] == 3:
            return 0.12344, 0.654321
        return -0.2, 0.11111

    out = E.main(["--pred", str(pred), "--model", "unused.pth", "--out", str(tmp_path / "o")], score_fn=stub)
    assert seen == [(2, 8, 10, 3), (3, 8, 10, 3)]
    assert out == {"per_sample": {"a": {"fastervqa": 0.1111, "fastervqa_raw": -0.2}, "b": {"fastervqa": 0.6543, "fastervqa_raw": 0.1234}},
                   "average": {"fastervqa": 0.3827, "fastervqa_raw": -0.0383}, "count": 2}
    with open(tmp_path / "o" / "metrics_fastervqa.json") as f:
        assert json.load(f) == out


def test_refusals(tmp_path, monkeypatch, capsys):
    with pytest.raises(ValueError, match="smaller than the 224 x 224 fragment canvas; the original upsamples"):
        Q.sample_plan(10, 223, 400, FASTER)
    with pytest.raises(ValueError, match="smaller than the 224 x 224 fragment canvas"):
        Q.sample_plan(10, 400, 200, FAST)
    with pytest.raises(ValueError, match="at least one frame"):
        Q.sample_plan(0, 400, 400, FAST)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no HIP device is visible"):
        E.make_score_fn(str(tmp_path / "none.pth"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(FileNotFoundError, match="checkpoint is not shipped; pass your own file"):
        E.make_score_fn(str(tmp_path / "none.pth"))
    with pytest.raises(ValueError, match="unknown variant"):
        E.make_score_fn(str(tmp_path / "none.pth"), variant="MANIQA")
    for argv, msg in ((["--pred", "x", "--model", "m", "--variant", "DOVER"], "choose FasterVQA or FAST-VQA"),
                      (["--pred", "x", "--model", "m", "--rescale_std", "0"], "must be positive")):
        with pytest.raises(SystemExit):
            E.main(argv)
        assert msg in capsys.readouterr().err
    # a clip below the canvas is reported with the reason and leaves no entry
    pred = tmp_path / "pred"
    pred.mkdir()
    np.save(pred / "small.npy", np.zeros((2, 100, 300, 3), dtype=np.uint8))

    def plan_only(frames):
        Q.sample_plan(frames.shape[0], frames.shape[1], frames.shape[2], FASTER)
        return 0.0, 0.5

    out = E.process(str(pred), str(tmp_path / "o"), score_fn=plan_only)
    assert out["count"] == 0 and "smaller than the 224 x 224 fragment canvas" in capsys.readouterr().out


# ---- the library ------------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ("dove_vqa_fragments_f32", "dove_swin3d_window_gather_f32", "dove_swin3d_window_scatter_f32", "dove_swin3d_patch_merge_f32",
               "dove_swin3d_window_attention_f32", "dove_swin3d_attention_tiles", "dove_vqa_head_f64")


def test_exports_and_argument_checks():
    """The header declares the new entry points, the library built for gfx950 exports them, and each refuses bad arguments before any HIP call."""
    import os

    import test_abi
    from dove_amd import ops
    assert set(NEW_EXPORTS) <= set(test_abi.header_symbols())
    with open(os.path.join(test_abi.ROOT, "dove_amd", "csrc", "build.sh")) as f:
        assert re.search(r'SRCS="[^"]*\bswin3d\b', f.read())
    if not os.path.exists(L.LIB_PATH):                                      # hipcc --offload-arch=gfx950 needs no GPU
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    assert lib.dove_abi_version() == 15
    assert ops.swin3d_attention_tiles() == (32, 32, 392)
    assert lib.dove_swin3d_window_attention_f32(None, None, None, 96, 1, 64, 3, 1.0, None, None, 1, None, None, None, 1, None, 96, None) == -1
    assert b"dove_swin3d_window_attention_f32" in lib.dove_last_error()
    assert lib.dove_vqa_head_f64(None, 0, 1, 1, 1, None, None, 1, None, None, None, None) == -1 and b"vqa_head" in lib.dove_last_error()
    assert lib.dove_swin3d_patch_merge_f32(None, 1, 2, 2, 4, None, None) == -1 and b"patch_merge" in lib.dove_last_error()
    assert ops.swin3d_padded((4, 7, 7), (4, 4, 4)) == ((4, 8, 8), 4, 64)
