"""Optical flow and E*warp without a device: the C symbols, the weight loader and its BatchNorm folding, the padding and pair-grouping
arithmetic, the command line's flags and refusals, and the shape of the JSON it writes (from a stubbed per-clip function)."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from dove_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLOW_SYMBOLS = ["dove_conv2d_f32", "dove_instance_norm_f32", "dove_instance_norm_f32_workspace_bytes", "dove_corr_volume_f32",
                "dove_avgpool2_f32", "dove_corr_lookup_f32", "dove_gru_gate_f32", "dove_gru_update_f32", "dove_add_f32",
                "dove_convex_upsample_f32", "dove_flow_warp_error", "dove_flow_warp_error_workspace_bytes"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.fixture(scope="module")
def flow():
    from dove_amd import flow
    return flow


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_flow_symbols_declared_bound_and_exported(lib):
    with open(os.path.join(ROOT, "include", "dove_hip.h")) as f:
        src = f.read()
    declared = set(re.findall(r"\b(dove_[a-z0-9_]+)\s*\(", src))
    for s in FLOW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/dove_hip.h"
        assert s in L.SIGNATURES or s in L.PLAIN, f"{s} has no binding in dove_amd/lib.py"
        assert hasattr(lib, s), f"{s} is not exported by libdove_hip.so"
    with open(os.path.join(ROOT, "dove_amd", "csrc", "build.sh")) as f:
        assert re.search(r'SRCS="[^"]*\bflow\b', f.read())


def test_abi_version_is_still_15(lib):
    with open(os.path.join(ROOT, "include", "dove_hip.h")) as f:
        assert int(re.search(r"#define\s+DOVE_ABI_VERSION\s+(\d+)", f.read()).group(1)) == 15
    assert lib.dove_abi_version() == 15


def test_entry_points_validate_before_any_hip_call(lib):
    a = L.Conv2dF32Args()
    assert a.struct_size == C.sizeof(L.Conv2dF32Args) and C.sizeof(L.Conv2dF32Args) % 8 == 0
    a.x = a.w = a.out = 1
    a.n, a.h, a.w_in, a.cin, a.cout, a.kh, a.kw, a.stride, a.ldx, a.ldo, a.out_mul = 1, 4, 4, 8, 8, 3, 3, 1, 8, 8, 1.0
    for field, bad, word in (("kh", 4, b"kernel"), ("kw", 9, b"kernel"), ("stride", 3, b"stride"), ("act", 7, b"act"), ("ldo", 4, b"ldo"),
                             ("ldx", 2, b"ldx"), ("cin", 0, b"positive")):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert lib.dove_conv2d_f32(C.byref(a), None) == -1 and word in lib.dove_last_error(), field
        setattr(a, field, good)
    a.scale = 1                                                  # scale without shift
    assert lib.dove_conv2d_f32(C.byref(a), None) == -1 and b"scale and shift" in lib.dove_last_error()
    a.scale = None
    a.struct_size -= 8
    assert lib.dove_conv2d_f32(C.byref(a), None) == -1 and b"struct_size" in lib.dove_last_error()
    assert lib.dove_instance_norm_f32(None, 1, 2, 2, 4, None, 0, 1e-5, None, 0, None, None) == -1
    assert lib.dove_instance_norm_f32(1, 1, 2, 2, 4, None, 0, 1e-5, 1, 8, 1, None) == -1 and b"workspace" in lib.dove_last_error()
    assert lib.dove_corr_lookup_f32(1, 1, 1, 1, 1, 2, 0, 1, 7, 20, 1, None) == -1 and b"at least 8" in lib.dove_last_error()
    assert lib.dove_avgpool2_f32(1, 4, 1, 8, 1, None) == -1
    assert lib.dove_flow_warp_error(1, 1, L.BF16, 1, 1, 1, 8, 8, 1, 1 << 20, 1, None, None, None) == -1 and b"dtype" in lib.dove_last_error()
    assert lib.dove_flow_warp_error(1, 1, L.U8, 1, 1, 1, 8, 8, 1, 0, 1, None, None, None) == -1 and b"workspace" in lib.dove_last_error()
    assert int(lib.dove_flow_warp_error_workspace_bytes(2, 37, 53)) == 2 * math.ceil(37 * 53 / 256) * 16
    assert int(lib.dove_instance_norm_f32_workspace_bytes(2, 16, 20, 96)) == 2 * 96 * 2 * 16 + 2 * 96 * 8
    assert int(lib.dove_instance_norm_f32_workspace_bytes(0, 16, 20, 96)) == 0


# ---- weights --------------------------------------------------------------------------------------------------------------------------
def test_random_state_is_reproducible_and_matches_the_reference_shapes(flow, golden_dir):
    with open(os.path.join(golden_dir, "raft_state_shapes.json")) as f:
        want = {k: tuple(v) for k, v in json.load(f).items()}
    assert flow.raft_param_shapes() == want
    a, b, c = flow.random_raft_state(7), flow.random_raft_state(7), flow.random_raft_state(8)
    assert list(a) == list(want) or set(a) == set(want)
    for k, shape in want.items():
        assert tuple(a[k].shape) == shape and torch.equal(a[k], b[k]), k
    w = a["update_block.gru.convz1.weight"]
    assert not torch.equal(w, c["update_block.gru.convz1.weight"])
    assert abs(float(w.std()) / math.sqrt(2.0 / (384 * 5)) - 1) < 0.02
    assert float(a["fnet.conv1.bias"].abs().min()) > 0 and float(a["fnet.conv1.bias"].abs().max()) < 0.5
    for k in ("cnet.norm1.weight", "cnet.layer2.0.norm3.running_var"):
        assert 0.5 <= float(a[k].min()) and float(a[k].max()) <= 1.5
    assert a["cnet.norm1.num_batches_tracked"].dtype == torch.int64
    # norm3 is registered twice in the reference's module tree: both names carry the same values
    for leaf in ("weight", "bias", "running_mean", "running_var"):
        assert torch.equal(a[f"cnet.layer3.0.norm3.{leaf}"], a[f"cnet.layer3.0.downsample.1.{leaf}"])


def test_loader_strips_prefix_rejects_wrong_shape_and_small_model(flow, tmp_path):
    sd = flow.random_raft_state(3)
    path = tmp_path / "raft.pth"
    torch.save({"module." + k: v for k, v in sd.items()}, path)
    W = flow.RaftWeights.load(str(path))
    direct = flow.RaftWeights.from_state_dict(sd)
    assert set(W.convs) == set(direct.convs)
    for k in W.convs:
        assert torch.equal(W.convs[k].w, direct.convs[k].w) and torch.equal(W.convs[k].b, direct.convs[k].b)
    # the kernel's layout: [kh, kw, Cin, Cout]; z and r share one conv; cnet's last conv is split into its tanh and relu halves
    assert tuple(W.convs["gru.convzr1"].w.shape) == (1, 5, 384, 256) and tuple(W.convs["gru.convq2"].w.shape) == (5, 1, 384, 128)
    w = sd["update_block.gru.convr1.weight"]
    assert torch.equal(W.convs["gru.convzr1"].w[0, 3, 17, 128 + 5], w[5, 17, 0, 3])
    assert torch.equal(W.convs["cnet.conv2.inp"].w[0, 0, :, 2], sd["cnet.conv2.weight"][130, :, 0, 0])
    assert W.convs["fnet.conv1"].scale is None and W.convs["cnet.conv1"].scale is not None and W.convs["cnet.conv2.net"].scale is None
    bad = dict(sd)
    bad["update_block.encoder.convf1.weight"] = torch.zeros(128, 2, 5, 5)
    with pytest.raises(ValueError, match=r"update_block\.encoder\.convf1\.weight.*\(128, 2, 5, 5\).*\(128, 2, 7, 7\)"):
        flow.RaftWeights.from_state_dict(bad)
    missing = {k: v for k, v in sd.items() if k != "fnet.conv2.bias"}
    with pytest.raises(ValueError, match="fnet.conv2.bias is missing"):
        flow.RaftWeights.from_state_dict(missing)
    small = {"module.update_block.gru.convz.weight": torch.zeros(96, 242, 3, 3), "module.fnet.layer1.0.conv3.weight": torch.zeros(32, 8, 1, 1)}
    with pytest.raises(NotImplementedError, match="small"):
        flow.RaftWeights.from_state_dict(small)
    with pytest.raises(NotImplementedError, match="small"):
        flow.RaftWeights.load(str(path), small=True)


def test_batch_norm_folding_matches_torch_fp64(flow):
    g = torch.Generator().manual_seed(5)
    c = 96
    x = torch.randn(2, c, 5, 7, generator=g, dtype=torch.float64)
    w, b = torch.rand(c, generator=g) + 0.5, 0.1 * torch.randn(c, generator=g)
    mean, var = 0.1 * torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    want = torch.nn.functional.batch_norm(x, mean.double(), var.double(), w.double(), b.double(), training=False, eps=1e-5)
    scale, shift = flow.fold_batch_norm(w, b, mean, var)
    assert scale.dtype == torch.float32 and shift.dtype == torch.float32
    got = x * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    assert float((got - want).abs().max()) < 5e-7               # the two float32 roundings, on values of a few units
    sd = flow.random_raft_state(3)
    W = flow.RaftWeights.from_state_dict(sd)
    s2, t2 = flow.fold_batch_norm(*(sd[f"cnet.layer2.0.norm3.{leaf}"] for leaf in ("weight", "bias", "running_mean", "running_var")))
    assert torch.equal(W.convs["cnet.layer2.0.downsample.0"].scale, s2) and torch.equal(W.convs["cnet.layer2.0.downsample.0"].shift, t2)


# ---- padding and grouping ---------------------------------------------------------------------------------------------------------------
def test_input_padder_arithmetic(flow):
    assert flow.input_pad(131, 165) == (1, 2, 2, 3)              # (left, right, top, bottom): 165 -> 168, 131 -> 136, centred
    assert flow.input_pad(128, 160) == (0, 0, 0, 0) and flow.input_pad(720, 1280) == (0, 0, 0, 0)
    assert flow.input_pad(129, 167) == (0, 1, 3, 4)
    for h in range(120, 140):
        l, r, t, b = flow.input_pad(h, 200 - h)
        assert (h + t + b) % 8 == 0 and (200 - h + l + r) % 8 == 0 and 0 <= t + b < 8 and t == (t + b) // 2 and l == (l + r) // 2


def test_pair_grouping_planner(flow):
    one = flow.workspace_bytes(128, 160, 1)
    assert flow.workspace_bytes(128, 160, 3) == 3 * one
    corr = 4 * 320 * (320 + 80 + 20 + 4)                         # the 16 x 20 volume and its pools, floats
    assert one > corr and flow.workspace_bytes(256, 320, 1) > 15 * corr
    assert flow.plan_pair_groups(5, 128, 160, 2 * one + 1) == [(0, 2), (2, 4), (4, 5)]
    assert flow.plan_pair_groups(5, 128, 160, 100 * one) == [(0, 5)]
    assert flow.plan_pair_groups(1, 128, 160, one) == [(0, 1)]
    with pytest.raises(MemoryError, match="2880x5120"):
        flow.plan_pair_groups(2, 2880, 5120, 256 * 2**30)
    assert flow.workspace_bytes(2880, 5120, 1) > 280e9           # the all-pairs volume alone


# ---- the metric's bookkeeping and the command line ------------------------------------------------------------------------------------
def test_summarize_pairs(flow):
    r = flow.summarize_pairs([[3.0, 10.0], [0.0, 0.0], [6.0, 4.0]])
    assert r["pairs"] == 3 and r["pairs_without_valid_pixels"] == 1
    assert r["warping_error"] == pytest.approx(1000 * (3.0 / 30 + 6.0 / 12) / 2, rel=1e-15)
    assert math.isnan(r["per_pair"][1]) and r["per_pair"][0] == pytest.approx(0.1)
    r = flow.summarize_pairs(np.zeros((2, 2)))
    assert math.isnan(r["warping_error"]) and r["pairs_without_valid_pixels"] == 2


def _make_clips(root):
    rng = np.random.default_rng(0)
    for name, f in (("clipA", 3), ("clipB", 2), ("clipC", 4), ("single", 1)):
        np.save(os.path.join(root, name + ".npy"), rng.integers(0, 256, (f, 8, 8, 3), dtype=np.uint8))
    with open(os.path.join(root, "notes.txt"), "w") as f:
        f.write("not a clip")


def test_cli_json_shape_from_a_stubbed_flow(tmp_path, capsys):
    from dove_amd import eval_ewarp as E
    pred, out = tmp_path / "pred", tmp_path / "out"
    pred.mkdir()
    _make_clips(str(pred))
    values = {3: 1.23456789, 2: float("nan"), 4: 2.00004}

    def stub(frames):
        n = frames.shape[0]
        return {"warping_error": values[n], "pairs": n - 1, "pairs_without_valid_pixels": n - 1 if n == 2 else 0}

    res = E.main(["--pred", str(pred), "--out", str(out), "--mixed_precision", "--alternate_corr", "--iters", "5"], clip_error_fn=stub)
    text = capsys.readouterr().out
    assert "--mixed_precision changes nothing" in text and "--alternate_corr changes nothing" in text
    assert "clipB: 1 of 1 pairs have no valid pixel" in text and "Skipping single" in text
    with open(out / "metrics_ewarp.json") as f:
        got = json.load(f)
    assert set(got) == {"per_sample", "average", "count"} and got["count"] == 3
    assert got["per_sample"]["clipA"] == {"warping_error": 1.2346} and got["per_sample"]["clipC"] == {"warping_error": 2.0}
    assert math.isnan(got["per_sample"]["clipB"]["warping_error"])
    assert got["average"] == {"warping_error": round((1.2346 + 2.0) / 2, 4)}
    assert res["count"] == 3
    # every clip without a valid pixel: the average is NaN; no clip at all: empty average
    res = E.main(["--pred", str(pred)], clip_error_fn=lambda fr: {"warping_error": float("nan"), "pairs": 1, "pairs_without_valid_pixels": 1})
    assert math.isnan(res["average"]["warping_error"]) and os.path.exists(pred / "metrics_ewarp.json")      # --out defaults to --pred
    empty = tmp_path / "empty"
    empty.mkdir()
    assert E.main(["--pred", str(empty)], clip_error_fn=stub) == {"per_sample": {}, "average": {}, "count": 0}


def test_cli_refusals(tmp_path, capsys):
    from dove_amd import eval_ewarp as E
    for argv, word in ((["--pred", str(tmp_path), "--small"], "small"), (["--pred", str(tmp_path), "--metric", "dover"], "warping_error"),
                       (["--pred", str(tmp_path), "--iters", "0"], "iters"), ([], "--pred")):
        with pytest.raises(SystemExit) as e:
            E.main(argv, clip_error_fn=lambda fr: {})
        assert e.value.code == 2 and word in capsys.readouterr().err
    args = E.build_parser().parse_args(["--pred", "x"])
    assert args.metric == "warping_error" and args.iters == 20 and args.model.endswith("raft-things.pth") and args.out == ""
    assert not (args.small or args.mixed_precision or args.alternate_corr)
