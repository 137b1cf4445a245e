"""LPIPS and DISTS without a device: the C symbols and their refusals, the shape-only kernel selection of the trunk conv, the weight
loaders, self-checks of the torch restatement (tests/percep_ref.py) in fp64, the command lines' flags and refusals, and the JSON shape."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import percep_ref as R
from dove_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERCEP_SYMBOLS = ["dove_convnet_conv_f32", "dove_convnet_conv_f32_kernel_name", "dove_percep_prep_f32", "dove_maxpool_f32", "dove_l2pool_f32",
                  "dove_lpips_layer", "dove_lpips_layer_workspace_bytes", "dove_dists_layer", "dove_dists_layer_workspace_bytes"]
FAST, GENERAL = b"convnet3x3_f32_kernel", b"conv_f32_kernel"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.fixture(scope="module")
def percep():
    from dove_amd import percep
    return percep


def conv_args(cin=64, cout=128, k=3, stride=1, pad=1, h=8, w=8, n=1):
    a = L.ConvnetConvF32Args()
    a.x = a.w = a.out = 256
    a.n, a.h, a.w_in, a.cin, a.cout, a.kh, a.kw, a.stride, a.pad_h, a.pad_w, a.relu, a.ldx, a.ldo = n, h, w, cin, cout, k, k, stride, pad, pad, 1, \
        cin, cout
    return a


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_percep_symbols_declared_bound_and_exported(lib):
    with open(os.path.join(ROOT, "include", "dove_hip.h")) as f:
        declared = set(re.findall(r"\b(dove_[a-z0-9_]+)\s*\(", f.read()))
    for s in PERCEP_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/dove_hip.h"
        assert s in L.SIGNATURES or s in L.PLAIN, f"{s} has no binding in dove_amd/lib.py"
        assert hasattr(lib, s), f"{s} is not exported by libdove_hip.so"
    with open(os.path.join(ROOT, "dove_amd", "csrc", "build.sh")) as f:
        assert re.search(r'SRCS="[^"]*\bpercep\b', f.read())


def test_abi_version_is_still_15(lib):
    assert lib.dove_abi_version() == 15


def test_conv_refuses_bad_arguments_before_any_hip_call(lib):
    a = conv_args()
    assert a.struct_size == C.sizeof(L.ConvnetConvF32Args) and C.sizeof(L.ConvnetConvF32Args) % 8 == 0
    assert lib.dove_convnet_conv_f32_kernel_name(C.byref(a)) == FAST
    for field, bad, word in (("kh", 12, b"kernel"), ("kw", 0, b"kernel"), ("stride", 5, b"stride"), ("stride", 0, b"stride"),
                             ("pad_h", 3, b"pad"), ("pad_w", -1, b"pad"), ("ldo", 4, b"ldo"), ("ldx", 2, b"ldx"), ("cin", 0, b"positive"),
                             ("n", 0, b"positive"), ("x", None, b"null"), ("w", None, b"null"), ("out", None, b"null")):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert lib.dove_convnet_conv_f32(C.byref(a), None) == -1 and word in lib.dove_last_error(), field
        assert lib.dove_convnet_conv_f32_kernel_name(C.byref(a)) == b"", field
        setattr(a, field, good)
    b = conv_args(k=11, stride=4, pad=2, h=6, w=6, cin=3)          # 6 + 4 < 11: no output pixel
    assert lib.dove_convnet_conv_f32(C.byref(b), None) == -1 and b"smaller than the kernel" in lib.dove_last_error()
    a.struct_size -= 8
    assert lib.dove_convnet_conv_f32(C.byref(a), None) == -1 and b"struct_size" in lib.dove_last_error()
    assert lib.dove_convnet_conv_f32_kernel_name(C.byref(a)) == b""
    assert lib.dove_convnet_conv_f32(None, None) == -1


def test_other_entry_points_refuse_bad_arguments(lib):
    m3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    z3 = (C.c_float * 3)(0.5, 0.0, 0.5)
    v = L.ImageView()
    v.data, v.dtype = 256, L.U8
    for args, word in (((None, 1, 3, 4, 4, 1.0, 0.0, m3, m3, 1, None), b"null"), ((C.byref(v), 1, 2, 4, 4, 1.0, 0.0, m3, m3, 1, None), b"channels"),
                       ((C.byref(v), 1, 3, 0, 4, 1.0, 0.0, m3, m3, 1, None), b"positive"), ((C.byref(v), 1, 3, 4, 4, 1.0, 0.0, m3, z3, 1, None), b"std"),
                       ((C.byref(v), 1, 3, 4, 4, 1.0, 0.0, m3, m3, None, None), b"null")):
        assert lib.dove_percep_prep_f32(*args) == -1 and word in lib.dove_last_error(), word
    v.dtype = L.BF16
    assert lib.dove_percep_prep_f32(C.byref(v), 1, 3, 4, 4, 1.0, 0.0, m3, m3, 1, None) == -1 and b"dtype" in lib.dove_last_error()
    for args, word in (((None, 8, 1, 4, 4, 8, 2, 2, 1, 8, None), b"null"), ((1, 8, 1, 4, 4, 8, 5, 2, 1, 8, None), b"window"),
                       ((1, 8, 1, 4, 4, 8, 2, 0, 1, 8, None), b"stride"), ((1, 8, 1, 2, 4, 8, 3, 2, 1, 8, None), b"smaller"),
                       ((1, 4, 1, 4, 4, 8, 2, 2, 1, 8, None), b"ldx"), ((1, 8, 1, 4, 4, 8, 2, 2, 1, 4, None), b"ldo")):
        assert lib.dove_maxpool_f32(*args) == -1 and word in lib.dove_last_error(), word
    for args, word in (((1, 8, 1, 4, 4, 8, None, 8, None), b"null"), ((1, 8, 0, 4, 4, 8, 1, 8, None), b"positive"),
                       ((1, 4, 1, 4, 4, 8, 1, 8, None), b"ldx")):
        assert lib.dove_l2pool_f32(*args) == -1 and word in lib.dove_last_error(), word
    need = int(lib.dove_lpips_layer_workspace_bytes(2, 37, 53))
    assert need == 2 * math.ceil(37 * 53 / 128) * 8
    assert int(lib.dove_lpips_layer_workspace_bytes(0, 37, 53)) == 0
    for args, word in (((1, 1, 64, 1, 2, 37, 53, 64, None, need, 1, None), b"null"), ((1, 1, 64, 1, 2, 37, 53, 64, 1, need - 1, 1, None), b"workspace"),
                       ((1, 1, 32, 1, 2, 37, 53, 64, 1, need, 1, None), b"ld "), ((1, 1, 64, 1, 2, 37, 53, 0, 1, need, 1, None), b"positive")):
        assert lib.dove_lpips_layer(*args) == -1 and word in lib.dove_last_error(), word
    need = int(lib.dove_dists_layer_workspace_bytes(2, 37, 53, 64))
    assert need == 2 * 64 * math.ceil(37 * 53 / 1024) * 5 * 8
    assert int(lib.dove_dists_layer_workspace_bytes(0, 37, 53, 64)) == 0 and int(lib.dove_dists_layer_workspace_bytes(2, 37, 53, 0)) == 0
    for args, word in (((1, 1, 64, 1, None, 2, 37, 53, 64, 1, need, 1, None), b"null"), ((1, 1, 64, 1, 1, 2, 37, 53, 64, 1, need - 1, 1, None), b"workspace"),
                       ((1, 1, 32, 1, 1, 2, 37, 53, 64, 1, need, 1, None), b"ld "), ((1, 1, 64, 1, 1, 0, 37, 53, 64, 1, need, 1, None), b"positive")):
        assert lib.dove_dists_layer(*args) == -1 and word in lib.dove_last_error(), word


def test_kernel_name_is_a_function_of_the_shape(lib, percep):
    vgg3x3 = [(cout, cin) for stage in percep.VGG_STAGES for _, cout, cin in stage if cin >= 64]
    assert len(vgg3x3) == 12
    for cout, cin in vgg3x3:
        # 64 -> 64 is the one VGG16 shape on which the fast walk was measured to lose (its N tile is half empty): cout < 128 goes general
        want = FAST if cout >= 128 else GENERAL
        assert (want == GENERAL) == ((cout, cin) == (64, 64))
        for hw in ((1, 1), (45, 80), (720, 1280)):
            assert lib.dove_convnet_conv_f32_kernel_name(C.byref(conv_args(cin, cout, h=hw[0], w=hw[1], n=2))) == want, (cin, cout, hw)
    assert lib.dove_convnet_conv_f32_kernel_name(C.byref(conv_args(64, 64, h=720, w=1280, n=2))) == GENERAL
    for cout, want in ((64, GENERAL), (96, GENERAL), (124, GENERAL), (128, FAST), (132, FAST), (200, FAST)):
        assert lib.dove_convnet_conv_f32_kernel_name(C.byref(conv_args(64, cout))) == want, cout
    for kw in (dict(cin=3, cout=64), dict(cin=3, cout=64, k=11, stride=4, pad=2, h=31, w=31), dict(cin=64, cout=192, k=5, pad=2),
               dict(cin=64, cout=128, stride=2), dict(cin=48, cout=128), dict(cin=64, cout=128, pad=0), dict(cin=64, cout=130)):
        assert lib.dove_convnet_conv_f32_kernel_name(C.byref(conv_args(**kw))) == GENERAL, kw
    a = conv_args(64, 128)
    a.ldx = 66                                                      # rows that are not 16-byte aligned cannot take 16-byte loads
    assert lib.dove_convnet_conv_f32_kernel_name(C.byref(a)) == GENERAL
    from dove_amd import ops
    assert ops.convnet_conv_kernel_name((2, 45, 80, 256), (3, 3, 256, 512)) == FAST.decode()
    assert ops.convnet_conv_kernel_name((2, 31, 31, 3), (11, 11, 3, 64), stride=4, pad=(2, 2)) == GENERAL.decode()
    # AlexNet's 3 x 3 convs have cin 192, 384, 256: multiples of 32
    for _, cout, cin, k, _, _ in percep.ALEX_CONVS[2:]:
        assert lib.dove_convnet_conv_f32_kernel_name(C.byref(conv_args(cin, cout))) == FAST


def test_routing_is_as_recorded(lib):
    """tests/golden/conv_f32_routing.json (tools/make_conv_routing_golden.py) holds the kernel that dove_convnet_conv_f32 and
    dove_resnet_conv_f32 chose, '' for a refusal, over a grid that crosses every routing rule, recorded before the fp32 convs were given
    one dispatch.  Every row must still give that name."""
    with open(os.path.join(ROOT, "tests", "golden", "conv_f32_routing.json")) as f:
        rec = json.load(f)
    assert rec["fields"] == ["entry", "k", "stride", "pad", "cin", "cout", "ldx", "x", "pool", "h", "w", "name"] and len(rec["rows"]) > 5000
    assert set(rec["names"]) == {"", "conv_f32_kernel", "convnet3x3_f32_kernel", "convnet3x3_n64_f32_kernel", "pointwise_f32_kernel"}
    wrong = []
    for row in rec["rows"]:
        entry, k, stride, pad, cin, cout, ldx, x, pool, h, w, name = row
        a = (L.ConvnetConvF32Args, L.ResnetConvF32Args)[entry]()
        a.x, a.w, a.out = x, 256, 256
        a.n, a.h, a.w_in, a.cin, a.cout, a.stride, a.relu, a.ldx, a.ldo = 2, h, w, cin, cout, stride, 1, ldx, cout
        if entry == 0:
            a.kh, a.kw, a.pad_h, a.pad_w = k, k, pad, pad
        else:
            a.k, a.pool = k, pool
        got = getattr(lib, rec["entries"][entry] + "_kernel_name")(C.byref(a)).decode()
        if got != rec["names"][name]:
            wrong.append((row, got))
    assert not wrong, (len(wrong), wrong[:5])


# ---- weights --------------------------------------------------------------------------------------------------------------------------
def test_random_states_are_reproducible_with_healthy_magnitudes(percep):
    for net in ("alex", "vgg"):
        (a, la), (b, lb), (c, _) = percep.random_lpips_state(5, net), percep.random_lpips_state(5, net), percep.random_lpips_state(6, net)
        want = percep.backbone_param_shapes(net)
        assert set(a) == set(want)
        for k, shape in want.items():
            assert tuple(a[k].shape) == shape and torch.equal(a[k], b[k]), k
        k = "features.10.weight"
        assert not torch.equal(a[k], c[k])
        fan = a[k].shape[1] * a[k].shape[2] * a[k].shape[3]
        assert abs(float(a[k].std()) / math.sqrt(2.0 / fan) - 1) < 0.02
        assert float(a["features.0.bias"].abs().min()) > 0 and float(a["features.0.bias"].abs().max()) < 0.5
        assert [tuple(v.shape) for v in la.values()] == [(1, ch, 1, 1) for ch in percep.LPIPS_CHANNELS[net]]
        assert all(float(v.min()) > 0 for v in la.values()) and all(torch.equal(la[k], lb[k]) for k in la)
    sd, ab = percep.random_dists_state(5)
    assert set(sd) == set(percep.backbone_param_shapes("vgg"))
    assert tuple(ab["alpha"].shape) == tuple(ab["beta"].shape) == (1, 1475, 1, 1) and float(ab["alpha"].min()) > 0 and float(ab["beta"].min()) > 0
    assert sorted(n for n, *_ in percep.ALEX_CONVS) == [0, 3, 6, 8, 10]
    assert [n for stage in percep.VGG_STAGES for n, *_ in stage] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]


def test_loaders_key_maps_prefix_layout_and_errors(percep, tmp_path):
    sd, lin = percep.random_lpips_state(3, "alex")
    extra = dict(sd)
    extra["classifier.1.weight"] = torch.zeros(4, 4)                # classifier entries are ignored
    bp, lp = tmp_path / "alexnet-owt.pth", tmp_path / "LPIPS_v0.1_alex.pth"
    torch.save({"module." + k: v for k, v in extra.items()}, bp)
    torch.save(lin, lp)
    W = percep.LpipsWeights.load(str(bp), str(lp), "alex")
    assert sorted(W.convs) == [0, 3, 6, 8, 10] and W.net == "alex" and len(W.lins) == 5
    w, b = W.convs[3]
    assert tuple(w.shape) == (5, 5, 64, 192) and w.dtype == torch.float32 and w.is_contiguous()
    src = sd["features.3.weight"]
    for co, ci, ky, kx in ((0, 0, 0, 0), (191, 63, 4, 4), (17, 5, 1, 3), (100, 40, 2, 0)):
        assert float(w[ky, kx, ci, co]) == float(src[co, ci, ky, kx])
    assert torch.equal(b, sd["features.3.bias"]) and torch.equal(W.lins[1], lin["lin1.model.1.weight"].reshape(-1))
    bad = dict(sd)
    bad["features.6.weight"] = torch.zeros(384, 192, 5, 5)
    with pytest.raises(ValueError, match=r"features\.6\.weight has shape \(384, 192, 5, 5\), expected \(384, 192, 3, 3\)"):
        percep.LpipsWeights.from_state_dicts(bad, lin, "alex")
    miss = {k: v for k, v in sd.items() if k != "features.8.bias"}
    with pytest.raises(ValueError, match=r"features\.8\.bias is missing"):
        percep.LpipsWeights.from_state_dicts(miss, lin, "alex")
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight is missing"):
        percep.LpipsWeights.from_state_dicts(sd, {k: v for k, v in lin.items() if not k.startswith("lin4")}, "alex")
    with pytest.raises(ValueError, match=r"VGG16 checkpoint: features\.0\.weight has shape \(64, 3, 11, 11\), expected \(64, 3, 3, 3\)"):
        percep.LpipsWeights.from_state_dicts(sd, lin, "vgg")       # an AlexNet state is no VGG16

    vsd, ab = percep.random_dists_state(3)
    D = percep.DistsWeights.from_state_dicts({"module." + k: v for k, v in vsd.items()}, ab)
    assert len(D.convs) == 13 and [t.numel() for t in D.alpha] == list(percep.DISTS_CHANNELS) == [t.numel() for t in D.beta]
    total = sum(float(t.sum()) for t in D.alpha) + sum(float(t.sum()) for t in D.beta)
    assert abs(total - 1) < 1e-12 and D.alpha[0].dtype == torch.float64
    w_sum = ab["alpha"].double().sum() + ab["beta"].double().sum()
    assert float(D.beta[1][2]) == float(ab["beta"].double().reshape(-1)[3 + 2] / w_sum)
    with pytest.raises(ValueError, match=r"alpha has shape \(1, 1472, 1, 1\), expected \(1, 1475, 1, 1\)"):
        percep.DistsWeights.from_state_dicts(vsd, {"alpha": ab["alpha"][:, 3:], "beta": ab["beta"]})
    with pytest.raises(ValueError, match="beta is missing"):
        percep.DistsWeights.from_state_dicts(vsd, {"alpha": ab["alpha"]})


def test_weight_directory_lookup(percep, tmp_path):
    with pytest.raises(FileNotFoundError, match=r"alexnet\*\.pth.*" + re.escape(str(tmp_path))):
        percep.load_metric_weights(str(tmp_path), "lpips")
    sd, lin = percep.random_lpips_state(2, "alex")
    torch.save(sd, tmp_path / "alexnet-owt-7be5be79.pth")
    with pytest.raises(FileNotFoundError, match=r"LPIPS_v0\.1_alex\*\.pth"):
        percep.load_metric_weights(str(tmp_path), "lpips")
    torch.save(lin, tmp_path / "LPIPS_v0.1_alex-df73285e.pth")
    assert percep.load_metric_weights(str(tmp_path), "lpips").net == "alex"
    with pytest.raises(FileNotFoundError, match=r"vgg16\*\.pth"):
        percep.load_metric_weights(str(tmp_path), "dists")


def test_group_size_and_small_image_refusal(percep):
    assert percep.group_size("vgg", 720, 1280) == 4 and percep.group_size("vgg", 720, 1280, budget=1) == 1
    assert percep.group_size("vgg", 67, 91) > 100
    x = torch.zeros(1, 3, 15, 40)
    with pytest.raises(ValueError, match="minimum side is 16"):
        percep._inputs(x, x, "vgg", "lpips")
    with pytest.raises(ValueError, match="minimum side is 31"):
        percep._inputs(torch.zeros(1, 3, 40, 30), torch.zeros(1, 3, 40, 30), "alex", "lpips")
    with pytest.raises(ValueError, match="same"):
        percep._inputs(x, torch.zeros(1, 3, 16, 40), "vgg", "dists")


# ---- the restatement, in fp64 -----------------------------------------------------------------------------------------------------------
def test_ref_l2pool_is_the_grouped_conv():
    g = torch.Generator().manual_seed(0)
    a = torch.tensor([0.5, 1.0, 0.5], dtype=torch.float64)
    k = a[:, None] * a[None, :]
    k = k / k.sum()
    assert k.flatten().tolist() == [1 / 16, 1 / 8, 1 / 16, 1 / 8, 1 / 4, 1 / 8, 1 / 16, 1 / 8, 1 / 16]
    for h, w in ((5, 7), (16, 20), (17, 23), (1, 1)):
        x = torch.randn(2, 6, h, w, generator=g, dtype=torch.float64)
        want = torch.sqrt(F.conv2d(x ** 2, k[None, None].repeat(6, 1, 1, 1), stride=2, padding=1, groups=6) + 1e-12)
        got = R.l2pool_ref(x)
        assert got.shape == want.shape == (2, 6, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
        assert float((got - want).abs().max()) < 1e-14


def test_ref_identical_images_score_zero(percep):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 3, 33, 41, generator=g, dtype=torch.float64)
    for net in ("alex", "vgg"):
        sd, lin = percep.random_lpips_state(4, net)
        v = R.lpips_ref(sd, lin, net, x, x.clone())
        assert v.dtype == torch.float64 and v.tolist() == [0.0, 0.0]
        y = (x + 0.1 * torch.randn(x.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
        assert float(R.lpips_ref(sd, lin, net, x, y).min()) > 0
    sd, ab = percep.random_dists_state(4)
    assert float(R.dists_ref(sd, ab, x, x.clone()).abs().max()) < 1e-12
    y = (x + 0.1 * torch.randn(x.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    d = R.dists_ref(sd, ab, x, y)
    assert 0 < float(d.min()) and float(d.max()) < 1
    assert R.dists_ref(sd, ab, x.float(), y.float()).dtype == torch.float32
    # a one-channel image is the same as its three-fold repetition
    assert torch.equal(R.dists_ref(sd, ab, x[:, :1], y[:, :1]), R.dists_ref(sd, ab, x[:, :1].repeat(1, 3, 1, 1), y[:, :1].repeat(1, 3, 1, 1)))


# ---- surfaces ---------------------------------------------------------------------------------------------------------------------------
def test_surfaces_without_weights_refuse_as_before_and_with_wrong_weights(percep):
    from dove_amd import metrics as M
    for name in ("lpips", "lpips-vgg", "dists"):
        with pytest.raises(NotImplementedError, match="pyiqa"):
            M.create_metric(name)
    W = percep.LpipsWeights.from_state_dicts(*percep.random_lpips_state(1, "alex"), "alex")
    m = M.create_metric("lpips", weights=W)
    assert m.lower_better is True and m.metric_name == "lpips"
    with pytest.raises(TypeError, match="DistsWeights"):
        M.create_metric("dists", weights=W)
    with pytest.raises(TypeError, match="vgg"):
        M.create_metric("lpips-vgg", weights=W)
    with pytest.raises(NotImplementedError, match="weights belong to"):
        M.create_metric("psnr", weights=W)
    with pytest.raises(NotImplementedError, match="pyiqa"):
        M.clip_metrics(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), torch.zeros(1, 32, 32, 3, dtype=torch.uint8), ["psnr", "dists"],
                       weights={"lpips": W})
    y = M.rgb_to_y(torch.full((2, 4, 5, 3), 255, dtype=torch.uint8))
    assert tuple(y.shape) == (2, 1, 4, 5) and abs(float(y[0, 0, 0, 0]) - (0.257 + 0.504 + 0.098 + 0.0625)) < 1e-6


def test_command_lines_refuse_missing_weights(tmp_path, capsys):
    from dove_amd import cli, eval_metrics
    assert eval_metrics.load_weights(["psnr", "lpips"], "") == {}
    with pytest.raises(FileNotFoundError, match=r"alexnet\*\.pth"):
        eval_metrics.load_weights(["psnr", "lpips"], str(tmp_path))
    assert eval_metrics.load_weights(["psnr", "ssim"], str(tmp_path)) == {}
    # without --metric_weights the metrics fail to initialise, as before
    models = eval_metrics.init_models(["lpips", "clipiqa"])
    assert models == {} and "pyiqa" in capsys.readouterr().out
    with pytest.raises(NotImplementedError, match="psnr"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "psnr,lpips", "--gt_dir", str(tmp_path)])
    with pytest.raises(FileNotFoundError, match=r"DISTS_weights\*\.pth|vgg16\*\.pth"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "psnr,dists", "--gt_dir", str(tmp_path), "--metric_weights", str(tmp_path)])
    with pytest.raises(NotImplementedError):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "clipiqa", "--gt_dir", str(tmp_path), "--metric_weights", str(tmp_path)])


def test_json_shape_from_a_stubbed_clip_function(tmp_path, monkeypatch, percep):
    from dove_amd import eval_metrics
    from dove_amd import metrics as M
    gt, pred, wdir = tmp_path / "gt", tmp_path / "pred", tmp_path / "w"
    for d in (gt, pred, wdir):
        d.mkdir()
    for name in ("a", "b"):
        np.save(gt / f"{name}.npy", np.zeros((2, 32, 32, 3), np.uint8))
        np.save(pred / f"{name}.npy", np.zeros((2, 32, 32, 3), np.uint8))
    sd, lin = percep.random_lpips_state(1, "alex")
    vsd, ab = percep.random_dists_state(1)
    torch.save(sd, wdir / "alexnet-owt.pth")
    torch.save(lin, wdir / "LPIPS_v0.1_alex.pth")
    torch.save(vsd, wdir / "vgg16-397923af.pth")
    torch.save(ab, wdir / "DISTS_weights.pth")
    seen = []

    def stub(pred_u8, gt_u8, names, crop=0, test_y_channel=False, is_center=False, name=None, weights=None):
        seen.append((name, list(names), crop, test_y_channel, sorted(weights)))
        return {"psnr": 30.123456, "lpips": 0.25 if name == "a" else 0.35, "dists": 0.123449}

    monkeypatch.setattr(M, "clip_metrics", stub)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    out = eval_metrics.main(["--gt", str(gt), "--pred", str(pred), "--out", str(tmp_path), "--metrics", "psnr,lpips,dists", "--crop", "4",
                             "--test_y_channel", "--metric_weights", str(wdir)])
    assert seen == [("a", ["psnr", "lpips", "dists"], 4, True, ["dists", "lpips"]), ("b", ["psnr", "lpips", "dists"], 4, True, ["dists", "lpips"])]
    with open(tmp_path / "metrics_psnr_lpips_dists.json") as f:
        on_disk = json.load(f)
    assert on_disk == out == {"per_sample": {"a": {"psnr": 30.1235, "lpips": 0.25, "dists": 0.1234},
                                             "b": {"psnr": 30.1235, "lpips": 0.35, "dists": 0.1234}},
                              "average": {"psnr": 30.1235, "lpips": 0.3, "dists": 0.1234}, "count": 2}
