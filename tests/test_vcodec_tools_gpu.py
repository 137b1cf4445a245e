"""The codec round trip's H.264 tool set on the device: csrc/vcodec.hip against tests/vcodec_tools_ref.py, byte for byte - output frames,
chosen QPs and bit counts - for every tool on its own and all together, and the tool set inside the command-line tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vcodec_tools_ref as T
from dove_amd import degrade as D
from dove_amd import ops
from test_vcodec_tools_cpu import BITRATES, SHAPES, TOOLSETS, clip_of, reference, tools_clip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "tests", "golden", "degradation_config.yaml")


def bitrate_of(shape, rate):
    return {"QP 51": 0, "mid": SHAPES[shape][4], "QP 0": 10 ** 7}[rate]


@pytest.mark.parametrize("tools", TOOLSETS)
@pytest.mark.parametrize("rate", BITRATES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_roundtrip_equals_the_definition(shape, rate, tools):
    gop = SHAPES[shape][3]
    want, want_qp, want_bits, _ = reference(shape, rate, tools)
    x = torch.from_numpy(clip_of(shape)).cuda()
    got, qp, bits = ops.vcodec_roundtrip(x, bitrate_of(shape, rate), gop, want_stats=True, tools=tools)
    print(shape, rate, tools, "QP", want_qp.tolist(), "bits", want_bits.tolist(), "got", qp.cpu().tolist(), bits.cpu().tolist())
    assert got.dtype == torch.uint8 and qp.dtype == torch.int32 and bits.dtype == torch.int64
    assert qp.cpu().tolist() == want_qp.tolist()
    assert bits.cpu().tolist() == want_bits.tolist()
    diff = got.cpu().numpy() != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:8].tolist())
    assert (rate == "QP 51" and set(want_qp) == {51}) or (rate == "QP 0" and set(want_qp) == {0}) or (rate == "mid" and all(16 <= q < 51 for q in want_qp))
    if tools == 0:                                                                # the plain operator, as it is without the argument
        plain = ops.vcodec_roundtrip(x, bitrate_of(shape, rate), gop, want_stats=True)
        assert all(torch.equal(a, b) for a, b in zip(plain, (got, qp, bits)))
    if tools == T.ALL_TOOLS:                                                      # names are the mask, and two calls are identical
        again = ops.vcodec_roundtrip(x, bitrate_of(shape, rate), gop, want_stats=True, tools=["intra16", "qpel", "deblock"])
        assert all(torch.equal(a, b) for a, b in zip(again, (got, qp, bits)))


def test_groups_do_not_depend_on_the_call():
    x = torch.from_numpy(tools_clip(6, 40, 56, 9)).cuda()
    for tools in (T.ALL_TOOLS, T.QPEL | T.DEBLOCK):
        whole, qp, bits = ops.vcodec_roundtrip(x, 4000, 3, want_stats=True, tools=tools)
        halves = [ops.vcodec_roundtrip(x[f0:f0 + 3], 4000, 3, want_stats=True, tools=tools) for f0 in (0, 3)]
        assert torch.equal(whole, torch.cat([h[0] for h in halves]))
        assert torch.equal(qp, torch.cat([h[1] for h in halves])) and torch.equal(bits, torch.cat([h[2] for h in halves]))


def run_tool(*args):
    p = subprocess.run([sys.executable, "-m", "dove_amd.degrade", *args], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout


def test_tool_runs_and_replays_sim_h264(tmp_path):
    clip = np.clip(tools_clip(8, 48, 64, 9), 0, 255).astype(np.uint8)
    src, out1, out2 = tmp_path / "in", tmp_path / "out1", tmp_path / "out2"
    os.makedirs(src)
    np.save(src / "c.npy", clip)
    run_tool("--input_dir", str(src), "--config", CONFIG, "--scale", "4", "--seed", "21", "--output_path", str(out1), "--video_codec", "sim-h264",
             "--gop", "4", "--block", "4")
    recipe = json.load(open(out1 / "c.recipe.json"))
    assert json.dumps(recipe) == json.dumps(D.Degrader(CONFIG, 4, 21, "sim-h264", 4).recipe(8, 48, 64))
    codec = [s for s in recipe["steps"] if s["op"] == "vcodec"]
    assert codec and all(s["tools"] == ["intra16", "qpel", "deblock"] and s["gop"] == 4 for s in codec)
    got = np.load(out1 / "c.npy")
    assert np.array_equal(got, D.apply_recipe(torch.from_numpy(clip), recipe).cpu().numpy())      # blocks of 4 in the tool, one of 8 here
    plain = dict(recipe, steps=[{k: v for k, v in s.items() if k != "tools"} for s in recipe["steps"]])
    assert not np.array_equal(got, D.apply_recipe(torch.from_numpy(clip), plain).cpu().numpy())   # the tools change the pixels
    run_tool("--input_dir", str(src), "--output_path", str(out2), "--recipe_in", str(out1 / "c.recipe.json"), "--block", "8")
    assert np.array_equal(np.load(out2 / "c.npy"), got)
