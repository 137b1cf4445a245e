"""The video-compression step on the device: csrc/vcodec.hip against tests/vcodec_ref.py, byte for byte - vectors, SADs, output frames,
chosen QPs and bit counts - and the step inside apply_recipe and the command-line tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vcodec_ref as R
from dove_amd import degrade as D
from dove_amd import ops
from test_vcodec_cpu import texture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "tests", "golden", "degradation_config.yaml")
S = R.SEARCH


# ---- motion search ----------------------------------------------------------------------------------------------------------------
def search_cases(h, w):
    """(cur, ref) planes of h x w: a flat frame (every cost ties: the answer is (0, 0)), a shift of exactly SEARCH, one of SEARCH + 2
    (outside the window), shifts that make the border macroblocks point outside the frame, noise, and two-level content full of ties."""
    T = texture(h + 40, w + 40, 7)[..., 0].astype(np.uint8)
    rng = np.random.default_rng(1)
    win = lambda dy, dx: T[20 + dy:20 + dy + h, 20 + dx:20 + dx + w]
    cases = [(np.full((h, w), 77, dtype=np.uint8), np.full((h, w), 77, dtype=np.uint8)),
             (win(0, 0), win(-S, -S)), (win(0, 0), win(S, -S)), (win(0, 0), win(-S - 2, -S - 2)),
             (win(0, 0), win(5, -6)), (win(0, 0), win(-3, 4)),
             (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)),
             (rng.integers(0, 2, (h, w), dtype=np.uint8) * 255, rng.integers(0, 2, (h, w), dtype=np.uint8) * 255),
             (rng.integers(100, 102, (h, w), dtype=np.uint8), rng.integers(100, 102, (h, w), dtype=np.uint8))]
    return np.stack([c for c, _ in cases]), np.stack([r for _, r in cases])


@pytest.mark.parametrize("size", [(48, 64), (33, 47)])
@pytest.mark.parametrize("search,lam", [(7, 4), (3, 0), (15, 9)])
def test_motion_search_equals_the_definition(size, search, lam):
    cur, ref = search_cases(*size)
    mv, sad = ops.motion_search_u8(torch.from_numpy(cur).cuda(), torch.from_numpy(ref).cuda(), search, lam)
    mv, sad = mv.cpu().numpy(), sad.cpu().numpy()
    assert mv.dtype == np.int32 and mv.shape == (len(cur), -(-size[0] // 16), -(-size[1] // 16), 2) and sad.shape == mv.shape[:3]
    for i in range(len(cur)):
        want_mv, want_sad = R.motion_search(cur[i], ref[i], search, lam)
        assert np.array_equal(mv[i], want_mv), (i, mv[i].tolist(), want_mv.tolist())
        assert np.array_equal(sad[i], want_sad), i
    assert not mv[0].any() and not sad[0].any()                                 # the flat frame
    if search == S and size == (48, 64):
        assert (mv[1][1:-1, 1:-1] == S).all() and not sad[1][1:-1, 1:-1].any()  # the shift of SEARCH is found where it is inside the frame
        assert (mv[4][0, :, 0] < 0).all() and (mv[4][:, -1, 1] > 0).all()       # top and right border macroblocks point outside the frame


# ---- the round trip ---------------------------------------------------------------------------------------------------------------
def moving_clip(n, h, w, seed):
    """A window sliding over a texture plus noise, on a float scale that leaves 0..255 on both sides and is not whole-numbered."""
    T = texture(h + 3 * n + 8, w + 3 * n + 8, seed)
    fr = np.stack([T[4 + t:4 + t + h, 4 + 2 * t:4 + 2 * t + w] for t in range(n)])
    fr = (fr - 128) * 1.6 + 128 + np.random.default_rng(seed).normal(0, 3, fr.shape)
    return np.ascontiguousarray(fr, dtype=np.float32)


ROUNDTRIPS = {  # name: (frames, height, width, gop, bitrate)
    "two groups and a short one": (11, 40, 56, 4, 9000),
    "odd sizes": (5, 33, 47, 8, 6000),
    "one frame": (1, 40, 56, 8, 20000),
    "QP 0": (4, 40, 56, 4, 10 ** 7),
    "mid QP": (4, 40, 56, 4, 3000),
    "QP 51": (4, 40, 56, 4, 0),
    "whole macroblocks": (3, 32, 48, 2, 12000),
}


@pytest.mark.parametrize("name", list(ROUNDTRIPS))
def test_roundtrip_equals_the_definition(name):
    n, h, w, gop, bitrate = ROUNDTRIPS[name]
    x = moving_clip(n, h, w, n * 100 + h)
    want, want_qp, want_bits = R.vcodec_roundtrip(x, bitrate, gop, want_stats=True)
    got, qp, bits = ops.vcodec_roundtrip(torch.from_numpy(x).cuda(), bitrate, gop, want_stats=True)
    print(name, "QP", want_qp.tolist(), "bits", want_bits.tolist())
    assert got.dtype == torch.uint8 and qp.dtype == torch.int32 and bits.dtype == torch.int64
    assert qp.cpu().tolist() == want_qp.tolist()
    assert bits.cpu().tolist() == want_bits.tolist()
    assert np.array_equal(got.cpu().numpy(), want)
    if name == "QP 0":
        assert want_qp.tolist() == [0]
    if name == "QP 51":
        assert want_qp.tolist() == [51]
    if name == "mid QP":
        assert 0 < want_qp[0] < 51
    if name == "two groups and a short one":
        assert len(want_qp) == 3 and torch.equal(ops.vcodec_roundtrip(torch.from_numpy(x).cuda(), bitrate, gop), got)


# ---- inside a recipe --------------------------------------------------------------------------------------------------------------
def test_split_into_groups_does_not_change_the_bytes():
    x = torch.from_numpy(np.clip(moving_clip(16, 40, 56, 3), 0, 255).astype(np.uint8))
    params = {"sigma_x": 1.2, "sigma_y": 0.7, "angle": 0.3, "beta_gaussian": 1.0, "beta_plateau": 1.0, "omega": 1.0}
    recipe = {"version": D.RECIPE_VERSION, "seed": 5, "scale": 1, "frames": 16, "input_size": [40, 56], "output_size": [24, 36],
              "steps": [{"op": "blur", "stage": "t", "family": "aniso", "size": 7, "params": [params]},
                        {"op": "resize", "stage": "t", "size": [24, 36], "mode": "bicubic"},
                        {"op": "vcodec", "stage": "t", "codec": "h264", "bitrate": 5000, "gop": 8},
                        {"op": "noise", "stage": "t", "kind": "gaussian", "gray": False, "level": [4.0] * 16, "stream_id": 0}]}
    whole = D.apply_recipe(x, recipe)
    assert tuple(whole.shape) == (16, 24, 36, 3) and whole.dtype == torch.uint8
    halves = torch.cat([D.apply_recipe(x[f0:f0 + 8], recipe, f0) for f0 in (0, 8)])
    assert torch.equal(whole, halves)
    # the step on its own is the definition's, and as the last step its frames come back unchanged
    last = dict(recipe, steps=recipe["steps"][:3])
    mid = ops.resize(ops.blur2d(x.cuda().float(), torch.from_numpy(D.kernel_from_params("aniso", 7, params).astype(np.float32)).cuda()), 24, 36, 1)
    want = R.vcodec_roundtrip(mid.cpu().numpy(), 5000, 8)
    assert np.array_equal(D.apply_recipe(x, last).cpu().numpy(), want)
    with pytest.raises(ValueError, match="--block"):
        D.apply_recipe(x[:4].cuda(), recipe, 0)


# ---- the tool ---------------------------------------------------------------------------------------------------------------------
def run_tool(*args):
    p = subprocess.run([sys.executable, "-m", "dove_amd.degrade", *args], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout


def test_tool_runs_and_replays_the_codec_steps(tmp_path):
    clip = np.clip(moving_clip(8, 48, 64, 9), 0, 255).astype(np.uint8)
    src, out1, out2, out3 = tmp_path / "in", tmp_path / "out1", tmp_path / "out2", tmp_path / "out3"
    os.makedirs(src)
    np.save(src / "c.npy", clip)
    common = ["--input_dir", str(src), "--config", CONFIG, "--scale", "4", "--seed", "21"]
    stdout = run_tool(*common, "--output_path", str(out1), "--video_codec", "sim", "--gop", "4", "--block", "4")
    recipe = json.load(open(out1 / "c.recipe.json"))
    codec = [s for s in recipe["steps"] if s["op"] == "vcodec" or s.get("type") == "RandomVideoCompression"]
    assert len(codec) == 2 and codec[0]["op"] == "vcodec" and all(s["op"] == "vcodec" or s["reason"] == "prob" for s in codec)
    assert all(s["gop"] == 4 for s in codec if s["op"] == "vcodec") and "vcodec" in stdout
    assert json.dumps(recipe) == json.dumps(D.Degrader(CONFIG, 4, 21, "sim", 4).recipe(8, 48, 64))
    got = np.load(out1 / "c.npy")
    assert got.shape == (8, 12, 16, 3)
    assert np.array_equal(got, D.apply_recipe(torch.from_numpy(clip), recipe).cpu().numpy())      # blocks of 4 in the tool, one of 8 here
    run_tool("--input_dir", str(src), "--output_path", str(out2), "--recipe_in", str(out1 / "c.recipe.json"), "--block", "8")
    assert np.array_equal(np.load(out2 / "c.npy"), got)                          # --recipe_in replays the vcodec steps
    run_tool(*common, "--output_path", str(out3), "--block", "3")                # without the flag: the codec steps are skipped, any --block
    plain = json.load(open(out3 / "c.recipe.json"))
    assert json.dumps(plain) == json.dumps(D.Degrader(CONFIG, 4, 21).recipe(8, 48, 64))
    assert [s["reason"] for s in plain["steps"] if s.get("type") == "RandomVideoCompression"] == ["no video codec in this build"] * 2
    assert np.array_equal(np.load(out3 / "c.npy"), D.apply_recipe(torch.from_numpy(clip), plain).cpu().numpy())
