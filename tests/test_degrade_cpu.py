"""Degradation synthesis without a device: the blur-kernel families against goldens made by the reference's own constructors
(tools/make_degrade_goldens.py), tests/degrade_ref.py against independent implementations (scipy, torch float64, libjpeg through Pillow),
the Degrader's recipes, and the argument checks of the C entry points (they run before any HIP call)."""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest
import torch

import degrade_ref as R
from dove_amd import degrade as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "tests", "golden", "degradation_config.yaml")


# ---- blur-kernel families ---------------------------------------------------------------------------------------------------------
def test_kernel_families_match_the_goldens(golden_dir):
    g = np.load(os.path.join(golden_dir, "degrade_kernels_golden.npz"))
    fams = [str(f) for f in g["families"]]
    assert set(fams) == set(D.KERNEL_FAMILIES) and set(int(s) for s in g["sizes"]) == {7, 13, 21}
    for i, (fam, size, p) in enumerate(zip(fams, g["sizes"], g["params"])):
        want = g[f"k{i}"]
        got = D.blur_kernel(fam, int(size), *[float(v) for v in p])
        assert got.shape == want.shape == (size, size) and got.dtype == np.float64
        assert abs(got.sum() - 1) < 1e-12
        err = np.abs(got - want).max()
        assert err <= (1e-10 if fam == "sinc" else 1e-12), (fam, size, p, err)


def test_bessel_j1_known_values():
    # Abramowitz & Stegun table 9.1: J1(1), J1(2), J1(10); the first zero j_{1,1}
    x = np.array([0.0, 1.0, 2.0, 10.0, 3.8317059702075125])
    want = np.array([0.0, 0.4400505857449335, 0.5767248077568734, 0.04347274616886144, 0.0])
    assert np.abs(D.bessel_j1(x) - want).max() < 1e-14
    assert np.abs(D.bessel_j1(-x) + want).max() < 1e-14


# ---- the numpy definitions against independent implementations --------------------------------------------------------------------
def test_ref_blur_matches_scipy_correlate_mirror():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 255, (2, 12, 17, 3))
    for k in (3, 7, 21):
        kern = rng.normal(size=(2, k, k))                       # asymmetric: correlation and convolution differ
        want = np.stack([np.stack([ndimage.correlate(x[n, ..., c], kern[n], mode="mirror") for c in range(3)], -1) for n in range(2)])
        assert np.abs(R.blur2d(x, kern) - want).max() < 1e-10
    one = np.zeros((7, 7))
    one[1, 5] = 1.0                                             # tap (dy, dx) = (1, 5): out[y, x] = in[y - 2, x + 2]
    assert np.array_equal(R.blur2d(x, one)[:, 2:, :-2], x[:, :-2, 2:])


@pytest.mark.parametrize("size", [(5, 7), (20, 31), (3, 17), (1, 1), (12, 17)])
def test_ref_bilinear_bicubic_match_torch_float64(size):
    x = np.random.default_rng(1).uniform(0, 255, (2, 12, 17, 3))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    for mode, name in ((R.RESIZE_BILINEAR, "bilinear"), (R.RESIZE_BICUBIC, "bicubic")):
        want = torch.nn.functional.interpolate(xt, size=size, mode=name, align_corners=False, antialias=False).permute(0, 2, 3, 1).numpy()
        assert np.abs(R.resize(x, *size, mode) - want).max() < 1e-10, (size, name)


def test_ref_area_matches_torch_at_integer_factors():
    x = np.random.default_rng(2).uniform(0, 255, (1, 12, 16, 3))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    for size in ((3, 4), (4, 8), (6, 2), (12, 16), (24, 32), (36, 16)):
        want = torch.nn.functional.interpolate(xt, size=size, mode="area").permute(0, 2, 3, 1).numpy()
        assert np.abs(R.resize(x, *size, R.RESIZE_AREA) - want).max() < 1e-10, size
    M = R.axis_matrix(12, 5, R.RESIZE_AREA)                      # a non-integer factor: rows are coverage fractions of the span
    assert np.allclose(M.sum(1), 1) and np.allclose(M.sum(0), 5 / 12)
    assert np.allclose(M[0, :3], [5 / 12, 5 / 12, 2 / 12])


def test_ref_dct_matrix_and_quality_rule():
    Cm = R.dct_matrix()
    assert list(Cm[1, :4]) == [4017, 3406, 2276, 799] and Cm[0, 0] == 2896 and list(Cm[2, :2]) == [3784, 1567]
    # rows are unit vectors scaled by 8192 with every entry rounded by at most 1/2: <a + da, b + db> is off by at most 2 sqrt(8) / 2 / 8192
    assert np.abs(Cm @ Cm.T / 8192.0 ** 2 - np.eye(8)).max() < 2 * 8 ** 0.5 * 0.5 / 8192
    assert R.quant_table(R.JPEG_LUMA, 50).tolist() == R.JPEG_LUMA.tolist()
    assert R.quant_table(R.JPEG_LUMA, 100).max() == 1 and R.quant_table(R.JPEG_CHROMA, 1).min() == 255
    assert R.quant_table(R.JPEG_LUMA, 49)[0, 0] == (16 * 102 + 50) // 100 and R.quant_table(R.JPEG_LUMA, 75)[0, 0] == 8


def smooth_plus_noise(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 9 + yy / 13), 128 + 90 * np.cos(xx / 7 - yy / 11), 128 + 80 * np.sin(xx / 5) * np.cos(yy / 6)], -1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255)


@pytest.mark.parametrize("quality", [30, 50, 75, 95])
@pytest.mark.parametrize("size", [(16, 16), (33, 47), (50, 70), (64, 96)])
def test_ref_jpeg_is_close_to_libjpeg(size, quality):
    """The definition is not libjpeg's arithmetic bit for bit (another integer DCT), so it is held to libjpeg by the ratio of its distance
    from Pillow's round trip to the loss of that round trip itself: a wrong table, quality rule or chroma layout gives a ratio near or above 1."""
    Image = pytest.importorskip("PIL.Image")
    img = smooth_plus_noise(*size, size[0] * 100 + quality).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling=2)
    pil = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).astype(np.float64)
    mine = R.jpeg_frame(img.astype(np.float32), quality).astype(np.float64)
    dist, loss = np.abs(mine - pil).mean(), np.abs(pil - img).mean()
    print(f"jpeg {size} q{quality}: |ref - pillow| {dist:.3f}  |pillow - input| {loss:.3f}  ratio {dist / loss:.3f}")
    assert dist / loss <= 0.25


# ---- Degrader ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def degrader():
    return D.Degrader(CONFIG, scale=4, seed=42)


def test_yaml_fixture_loads_and_both_stages_parse(degrader):
    assert [name for name, _, _ in degrader.stages] == ["degradation_1", "degradation_2"]
    s1, s2 = degrader.stages
    assert [t for t, _ in s1[1]] == ["RandomBlur", "RandomResize", "RandomNoise", "RandomJPEGCompression", "RandomVideoCompression"]
    assert [t for t, _ in s2[1]] == ["RandomBlur", "RandomResize", "RandomNoise", "RandomJPEGCompression"]
    assert s1[2] is None and len(s2[2]["entries"]) == 2 and isinstance(s2[2]["entries"][1], list)
    assert s1[1][3][1]["quality_step"] == 3


def test_same_seed_same_recipe_and_json_round_trip(degrader):
    a, b = degrader.recipe(7, 256, 320), D.Degrader(CONFIG, 4, 42).recipe(7, 256, 320)
    assert json.dumps(a) == json.dumps(b)
    assert json.loads(json.dumps(a)) == a
    assert json.dumps(degrader.recipe(7, 256, 320, seed=43)) != json.dumps(a)
    assert a["frames"] == 7 and a["input_size"] == [256, 320] and a["seed"] == 42 and a["version"] == D.RECIPE_VERSION


@pytest.mark.parametrize("scale", [2, 3, 4])
def test_target_size_follows_scale(scale):
    d = D.Degrader(CONFIG, scale=scale, seed=5)
    for seed in range(20):
        r = d.recipe(2, 250, 333, seed=seed)
        want = [int(250 / scale), int(333 / scale)]
        targets = [s for s in r["steps"] if s["op"] == "resize" and s["how"] == "target"]
        assert len(targets) == 1 and targets[0]["size"] == want and r["output_size"] == want
        assert [s for s in r["steps"] if s["op"] == "resize"][-1] is targets[0]


def test_is_size_even_and_size_bookkeeping(degrader):
    seen = set()
    for seed in range(300):
        h, w = 250, 333
        for s in degrader.recipe(1, 250, 333, seed=seed)["steps"]:
            if s["op"] == "resize":
                if s["how"] != "target":
                    assert s["size"][0] % 2 == 0 and s["size"][1] % 2 == 0 and min(s["size"]) >= 2, s
                    seen.add(s["how"])
                h, w = s["size"]
            if s["op"] == "blur":
                assert s["size"] // 2 < min(h, w)                      # only kernel sizes one reflection can serve are drawn
    assert seen == {"up", "down", "keep"}


def test_shuffle_keeps_the_group_adjacent(degrader):
    orders = set()
    for seed in range(64):
        tail = [s for s in degrader.recipe(1, 256, 256, seed=seed)["steps"] if s["stage"] == "degradation_2.shuffle"]
        kinds = [s["type"] if s["op"] == "skipped" else s["op"] for s in tail]
        assert len(kinds) == 3
        i = kinds.index("resize")
        assert kinds[i + 1] in ("blur", "RandomBlur")                  # the sinc blur (or its skip by prob) directly after the resize
        if kinds[i + 1] == "blur":
            assert tail[i + 1]["family"] == "sinc"
        orders.add(kinds.index("RandomVideoCompression"))
    assert orders == {0, 2}                                            # both orders occur, never the codec step inside the group


def test_codec_steps_are_recorded_as_skipped(degrader):
    r = degrader.recipe(3, 128, 128)
    codec = [s for s in r["steps"] if s["op"] == "skipped" and s["type"] == "RandomVideoCompression"]
    assert [s["stage"] for s in codec] == ["degradation_1", "degradation_2.shuffle"]
    assert all("codec" in s["reason"] for s in codec)


def _config(**resize_params):
    cfg = D.load_config(CONFIG)
    cfg = json.loads(json.dumps(cfg))
    cfg["degradation_1"]["random_resize"]["params"].update(resize_params)
    return cfg


def test_refusals():
    with pytest.raises(NotImplementedError, match="resize_step"):
        D.Degrader(_config(resize_step=0.1))
    with pytest.raises(NotImplementedError, match="lanczos"):
        D.Degrader(_config(resize_opt=["bilinear", "lanczos"], resize_prob=[0.5, 0.5]))
    cfg = _config()
    cfg["degradation_2"]["degradation_with_shuffle"]["degradations"][0] = {"type": "RandomSharpen", "params": {}}
    with pytest.raises(NotImplementedError, match="RandomSharpen"):
        D.Degrader(cfg)
    cfg = _config()
    cfg["degradation_1"]["random_sharpen"] = {"params": {}}
    with pytest.raises(ValueError, match="random_sharpen"):
        D.Degrader(cfg)
    cfg = _config()
    cfg["degradation_1"]["random_blur"]["params"]["kernel_list"][0] = "skew"
    with pytest.raises(NotImplementedError, match="skew"):
        D.Degrader(cfg)
    with pytest.raises(ValueError, match="version"):
        D.apply_recipe(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), {"version": 0, "steps": []})


def test_draw_frequencies(degrader):
    """20 000 recipes: the stage-1 draws of kernel family, resize direction and noise kind are within 5 binomial sigma of the config's
    probabilities (stage 1 has no ``prob``, so every recipe draws each once)."""
    n = 20000
    counts = {"family": {}, "how": {}, "kind": {}}
    for seed in range(n):
        for s in degrader.recipe(1, 256, 256, seed=seed)["steps"]:
            if s["stage"] != "degradation_1" or s["op"] == "skipped":
                continue
            for key, op in (("family", "blur"), ("how", "resize"), ("kind", "noise")):
                if s["op"] == op:
                    counts[key][s[key]] = counts[key].get(s[key], 0) + 1
    p1 = D.load_config(CONFIG)["degradation_1"]
    want = {"family": dict(zip(p1["random_blur"]["params"]["kernel_list"], p1["random_blur"]["params"]["kernel_prob"])),
            "how": dict(zip(("up", "down", "keep"), p1["random_resize"]["params"]["resize_mode_prob"])),
            "kind": dict(zip(p1["random_noise"]["params"]["noise_type"], p1["random_noise"]["params"]["noise_prob"]))}
    for key, probs in want.items():
        assert sum(counts[key].values()) == n
        for name, p in probs.items():
            got, sigma = counts[key].get(name, 0), (n * p * (1 - p)) ** 0.5
            assert abs(got - n * p) <= 5 * sigma, (key, name, got, n * p, sigma)


def test_jpeg_qualities_follow_the_step_rule(degrader):
    for seed in range(20):
        for s in degrader.recipe(24, 128, 128, seed=seed)["steps"]:
            if s["op"] == "jpeg":
                q = s["quality"]
                assert len(q) == 24 and all(isinstance(v, int) and 30 <= v <= 95 for v in q)
                assert max(abs(a - b) for a, b in zip(q, q[1:])) <= 3 and len(set(q)) > 1
            if s["op"] == "noise":
                assert len(s["level"]) == 24 and len(set(s["level"])) == 1          # the shipped config has no noise walk
            if s["op"] == "blur":
                assert len(s["params"]) == 1                                       # ... and no kernel walk: one kernel for all frames


def test_walks_clip_to_the_range():
    cfg = _config()
    cfg["degradation_1"]["random_noise"]["params"].update(gaussian_sigma_step=20, poisson_scale_step=2)
    cfg["degradation_1"]["random_blur"]["params"].update(sigma_x_step=2, rotate_angle_step=1)
    r = D.Degrader(cfg, seed=3).recipe(40, 128, 128)
    noise = next(s for s in r["steps"] if s["op"] == "noise" and s["stage"] == "degradation_1")
    lo, hi = (1, 30) if noise["kind"] == "gaussian" else (0.05, 3)
    assert len(set(noise["level"])) > 10 and lo <= min(noise["level"]) and max(noise["level"]) <= hi
    assert lo in noise["level"] or hi in noise["level"]                            # steps this large hit a bound within 40 frames
    blur = next(s for s in r["steps"] if s["op"] == "blur" and s["stage"] == "degradation_1")
    sx = [p["sigma_x"] for p in blur["params"]]
    assert len(sx) == 40 and 0.2 <= min(sx) and max(sx) <= 3 and len({p["sigma_y"] for p in blur["params"]}) == 1


def test_bicubic_preset_recipe():
    r = D.bicubic_recipe(5, 90, 130, 4)
    assert r["steps"] == [{"op": "resize", "stage": "preset", "size": [22, 32], "mode": "bicubic"}] and r["output_size"] == [22, 32]


# ---- the C entry points refuse bad arguments before any HIP call ------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    from dove_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    one = C.c_void_p(8)                                                            # never dereferenced: the checks come first

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.dove_last_error(), (rc, lib.dove_last_error())
    refused(lib.dove_blur2d_f32(one, 1, 10, 32, one, 21, 0, one, None), "too small")        # h <= k / 2
    refused(lib.dove_blur2d_f32(one, 1, 32, 10, one, 21, 0, one, None), "too small")
    refused(lib.dove_blur2d_f32(one, 1, 32, 32, one, 8, 0, one, None), "odd")
    refused(lib.dove_blur2d_f32(one, 1, 32, 32, one, 23, 0, one, None), "odd in 3..21")
    refused(lib.dove_blur2d_f32(one, 0, 32, 32, one, 7, 0, one, None), "bad shape")
    refused(lib.dove_blur2d_f32(None, 1, 32, 32, one, 7, 0, one, None), "null")
    refused(lib.dove_resize_f32(one, 1, 8, 8, 4, 4, 3, one, None), "bad mode")
    refused(lib.dove_resize_f32(one, 1, 8, 8, 0, 4, 0, one, None), "bad shape")
    sig = (C.c_float * 1)(1.0)
    refused(lib.dove_add_gaussian_noise_f32(one, 1, 8, 8, sig, 0, 1, 0, -1, one, None), "frame0")
    refused(lib.dove_add_poisson_noise_f32(one, 1, 8, 8, sig, 0, 1, 1 << 32, 0, one, 1024, one, None), "stream_id")
    refused(lib.dove_add_poisson_noise_f32(one, 1, 8, 8, sig, 0, 1, 0, 0, one, 1023, one, None), "workspace")
    assert lib.dove_poisson_noise_workspace_bytes(3) == 3 * 1024
    assert lib.dove_jpeg_roundtrip_workspace_bytes(2, 17, 33) == 2 * 32 * 48 * 3 // 2
    ws = lib.dove_jpeg_roundtrip_workspace_bytes(1, 8, 8)
    refused(lib.dove_jpeg_roundtrip(one, 1, 8, 8, (C.c_int * 1)(0), one, ws, one, None), "quality")
    refused(lib.dove_jpeg_roundtrip(one, 1, 8, 8, (C.c_int * 1)(101), one, ws, one, None), "quality")
    refused(lib.dove_jpeg_roundtrip(one, 1, 8, 8, (C.c_int * 1)(50), one, ws - 1, one, None), "workspace")
