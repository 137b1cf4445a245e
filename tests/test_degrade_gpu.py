"""The degradation operators on the device (csrc/degrade.hip) against tests/degrade_ref.py, the recipe runner against the hand composition
of the operators, and the command-line tool.  Shapes are the smallest that reach every branch: borders that reflect their full width,
widths that are no tile multiple, more than one block, one MCU and several, sizes that need padding."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import degrade_ref as R
from dove_amd import degrade as D
from dove_amd import lib as L
from dove_amd import ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "tests", "golden", "degradation_config.yaml")


def frames(n, h, w, seed):
    return np.random.default_rng(seed).uniform(0, 255, (n, h, w, 3)).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- blur -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_kernels(golden_dir):
    g = np.load(os.path.join(golden_dir, "degrade_kernels_golden.npz"))
    out = {}
    for i, (fam, size) in enumerate(zip(g["families"], g["sizes"])):
        out.setdefault(int(size), []).append((str(fam), g[f"k{i}"]))
    return out


@pytest.mark.parametrize("k", [7, 13, 21])
@pytest.mark.parametrize("shape", [(1, 11, 11), (2, 12, 37), (1, 40, 70), (2, 64, 96)])
def test_blur_matches_float64(shape, k, golden_kernels):
    """Tolerance 2 k^2 2^-24 sum|w| 255: k^2 FMAs, each rounding a partial sum bounded by sum|w| * 255, doubled; against the float64
    correlation with the fp32-rounded weights."""
    x = frames(*shape, seed=k)
    xd = dev(x)
    fams = golden_kernels[k]
    picks = [kern for fam, kern in fams[shape[1] % 3::3]]                      # one parameter set of each of the seven families
    assert len(picks) == 7
    picks.append(np.random.default_rng(k).normal(size=(k, k)))                 # asymmetric, signed
    for kern in picks:
        k32 = kern.astype(np.float32)
        got = ops.blur2d(xd, dev(k32)).cpu().numpy()
        err = np.abs(got - R.blur2d(x, k32)).max()
        assert err <= R.blur_tolerance(k32), (shape, k, err, R.blur_tolerance(k32))
    per = np.stack([fams[(3 * n + 1) % len(fams)][1] for n in range(shape[0])]).astype(np.float32)      # one kernel per frame
    got = ops.blur2d(xd, dev(per)).cpu().numpy()
    assert np.abs(got - R.blur2d(x, per)).max() <= R.blur_tolerance(per)


def test_blur_one_hot_kernels_are_exact_shifts():
    """A one-hot kernel at tap (dy, dx) must give the reflect-101 padded frame shifted by that tap, bit for bit: all 49 taps of k = 7,
    the corners and the centre of k = 21 (convolution for correlation, a dropped tap or a wrong border cannot hide in a tolerance)."""
    x = frames(1, 12, 13, seed=3)[0]
    for k, taps in ((7, [(dy, dx) for dy in range(7) for dx in range(7)]), (21, [(0, 0), (0, 20), (20, 0), (20, 20), (10, 10)])):
        r = k // 2
        xp = np.pad(x, ((r, r), (r, r), (0, 0)), mode="reflect")
        kern = np.zeros((len(taps), k, k), dtype=np.float32)
        for n, (dy, dx) in enumerate(taps):
            kern[n, dy, dx] = 1.0
        want = np.stack([xp[dy:dy + 12, dx:dx + 13] for dy, dx in taps])
        got = ops.blur2d(dev(np.broadcast_to(x, (len(taps), 12, 13, 3))), dev(kern)).cpu().numpy()
        assert np.array_equal(got, want), k


def test_blur_does_not_depend_on_the_split(golden_kernels):
    x = dev(frames(3, 40, 70, seed=9))
    per = dev(np.stack([golden_kernels[13][i][1] for i in (0, 7, 20)]).astype(np.float32))
    whole = ops.blur2d(x, per)
    parts = torch.cat([ops.blur2d(x[:1], per[:1]), ops.blur2d(x[1:], per[1:])])
    assert torch.equal(whole, parts)
    assert torch.equal(ops.blur2d(x[2:], per[2]), whole[2:])                  # a shared [k,k] kernel is the same arithmetic


# ---- resize -----------------------------------------------------------------------------------------------------------------------
RESIZE_CASES = [((11, 13), (5, 7)), ((12, 16), (3, 4)), ((9, 10), (13, 15)), ((1, 1), (3, 3)), ((64, 96), (16, 24))]


@pytest.mark.parametrize("mode", [L.RESIZE_BILINEAR, L.RESIZE_BICUBIC, L.RESIZE_AREA])
@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_resize_matches_float64(src, dst, mode):
    x = frames(2, *src, seed=src[0])
    got = ops.resize(dev(x), *dst, mode).cpu().numpy()
    assert got.shape == (2, *dst, 3)
    err = np.abs(got - R.resize(x, *dst, mode)).max()
    assert err <= R.resize_tolerance(*src, *dst, mode), (src, dst, mode, err)


def test_resize_to_the_even_size_of_a_recipe():
    """is_size_even: a drawn factor that asks for an odd number of rows and columns gives the even size below it."""
    d = D.Degrader(CONFIG, seed=1)
    for seed in range(200):
        step = next(s for s in d.recipe(1, 30, 26, seed=seed)["steps"] if s["op"] == "resize")
        if step["how"] == "down" and int(30 * step["factor"]) % 2 == 1 and int(26 * step["factor"]) % 2 == 1:
            break
    else:
        raise AssertionError("no seed below 200 asks for an odd size")
    oh, ow = step["size"]
    assert [oh, ow] == [int(30 * step["factor"]) - 1, int(26 * step["factor"]) - 1]
    x = frames(1, 30, 26, seed=4)
    for mode in (L.RESIZE_BILINEAR, L.RESIZE_BICUBIC, L.RESIZE_AREA):
        got = ops.resize(dev(x), oh, ow, mode).cpu().numpy()
        assert np.abs(got - R.resize(x, oh, ow, mode)).max() <= R.resize_tolerance(30, 26, oh, ow, mode)


def test_resize_same_size_is_an_exact_copy():
    x = dev(frames(2, 9, 10, seed=5))
    for mode in (L.RESIZE_BILINEAR, L.RESIZE_BICUBIC, L.RESIZE_AREA):
        assert torch.equal(ops.resize(x, 9, 10, mode), x)


# ---- Gaussian noise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", [False, True])
def test_gaussian_noise_is_sigma_times_randn_at_the_stated_indices(gray):
    n, h, w, seed, stream, frame0 = 2, 9, 11, 1234, 5, 3                       # 297 elements per frame: Philox blocks straddle frames
    sigma = [2.5, 7.0]
    per = h * w * (1 if gray else 3)
    z = ops.randn((n, h, w, 1) if gray else (n, h, w, 3), seed, stream, offset=frame0 * per)
    prod = z * torch.tensor(sigma, device="cuda").view(n, 1, 1, 1)
    noise = ops.add_gaussian_noise(torch.zeros(n, h, w, 3, device="cuda"), sigma, gray, seed, stream, frame0)
    ulp = prod.abs() * 2.0 ** -23
    assert bool(((noise - prod).abs() <= ulp).all())                           # x = 0: out - x is the rounded product itself
    if gray:
        assert torch.equal(noise[..., 0], noise[..., 1]) and torch.equal(noise[..., 0], noise[..., 2])
    want = R.gaussian_z(n, h, w, gray, seed, stream, frame0) * np.array(sigma).reshape(n, 1, 1, 1)      # the numpy definition of the stream
    # tests/test_randn_gpu.py gates the fp32 normals at 4 * 1.017e-6 of their float64 evaluation; the product adds one rounding
    assert bool((np.abs(noise.cpu().numpy() - want) <= max(sigma) * 4 * 1.017e-6 + np.abs(want) * 2.0 ** -23).all())
    x = dev(frames(n, h, w, seed=6))
    out = ops.add_gaussian_noise(x, sigma, gray, seed, stream, frame0)
    exact = x.double() + prod.double()
    assert bool(((out.double() - exact).abs() <= (out.abs() + prod.abs()).double() * 2.0 ** -23).all())


@pytest.mark.parametrize("gray", [False, True])
def test_gaussian_noise_blocks_equal_one_call(gray):
    x = dev(frames(5, 9, 11, seed=7))
    sigma = [1.0, 30.0, 4.5, 0.0, 12.0]
    whole = ops.add_gaussian_noise(x, sigma, gray, 99, 2, 3)
    parts = torch.cat([ops.add_gaussian_noise(x[:2], sigma[:2], gray, 99, 2, 3), ops.add_gaussian_noise(x[2:], sigma[2:], gray, 99, 2, 5)])
    assert torch.equal(whole, parts)
    assert torch.equal(whole[3], x[3])                                         # sigma 0


# ---- Poisson noise ----------------------------------------------------------------------------------------------------------------
REGION = 512                                                                   # the constant region: 512 x 512 = 2^18 pixels
POISSON_V = (0, 1, 7, 128, 255)


def poisson_frame(v, distinct):
    """[520,512,3]: rows 0..511 hold v, the 8-row strip below cycles through ``distinct`` values that include v."""
    f = np.full((REGION + 8, REGION), float(v), dtype=np.float32)
    pool = np.array(sorted({v} | set(range(256))), dtype=np.float32)
    pool = np.concatenate([[v], pool[pool != v]])[:distinct]
    f[REGION:] = pool[np.arange(8 * REGION) % distinct].reshape(8, REGION)
    return np.repeat(f[..., None], 3, axis=2)


def poisson_cdf(k, rate):
    return torch.special.gammaincc(k.double() + 1.0, torch.full_like(k, rate, dtype=torch.float64))


def check_poisson_sample(kk, v, U, what):
    """kk: the draws K / U of one region (a flat device tensor).  Mean, variance and Kolmogorov distance against Poisson(v U) / U."""
    n, lam = kk.numel(), v * U
    K = kk.double() * U
    assert torch.equal(K, K.round()), what                                     # integers over U
    mean, var = float(kk.double().mean()), float(kk.double().var(unbiased=False))
    ks = 0.0
    if lam > 0:
        vals, counts = torch.unique(K.cpu(), return_counts=True)
        grid = torch.arange(int(vals[0]) - 1, int(vals[-1]) + 1, dtype=torch.float64)
        emp = torch.zeros_like(grid)
        emp[(vals - grid[0]).long()] = counts.double() / n
        ks = float((emp.cumsum(0) - poisson_cdf(grid.clamp(min=0), float(lam)) * (grid >= 0)).abs().max())
    print(f"poisson {what}: rate {lam} n {n} mean {mean:.5f} (want {v}) var {var:.5f} (want {v / U:.5f}) KS {ks:.2e} (bound {1.95 / math.sqrt(n):.2e})")
    assert abs(mean - v) <= 6 * math.sqrt(v / (U * n)), what
    assert abs(var - v / U) <= 6 * math.sqrt((lam + 2 * lam * lam) / n) / U ** 2, what
    assert ks <= 1.95 / math.sqrt(n), what


@pytest.fixture(scope="module")
def poisson_colour():
    """Ten frames in one call: every v with 1 distinct value (U = 1, rate v: inversion below 10, PTRS above) and with 200 (U = 256, rates
    up to 65 280)."""
    cases = [(v, d) for d in (1, 200) for v in POISSON_V]
    x = dev(np.stack([poisson_frame(v, d) for v, d in cases]))
    return cases, x, ops.add_poisson_noise(x, 1.0, False, 2024, 3, 0)


@pytest.mark.parametrize("i", range(10))
def test_poisson_colour_statistics(poisson_colour, i):
    cases, x, out = poisson_colour
    v, distinct = cases[i]
    U = 1 if distinct == 1 else 256
    assert R.poisson_U(R.poisson_values(x[i].cpu().numpy(), False)) == U
    kk = (out[i, :REGION] - x[i, :REGION]).flatten() + v                        # scale 1 and integer x: exact
    if v == 0:
        assert torch.equal(out[i, :REGION], x[i, :REGION])                      # rate 0 gives exactly 0
    check_poisson_sample(kk, v, U, f"colour v={v} U={U}")


def test_poisson_gray_uses_the_luma():
    """One draw per pixel from the luma's value, added to R, G and B alike: v = 7 with U = 1, v = 128 with U = 256, and a frame whose channels
    differ (200, 50, 10 -> luma 90.29 -> 90)."""
    rgb = np.empty((REGION, REGION, 3), dtype=np.float32)
    rgb[...] = (200.0, 50.0, 10.0)
    x = dev(np.stack([poisson_frame(7, 1)[:REGION], poisson_frame(128, 1)[:REGION], rgb]))
    x[1, 0, :200, :] = torch.arange(200, device="cuda", dtype=torch.float32)[:, None]       # 200 distinct lumas in frame 1
    out = ops.add_poisson_noise(x, 1.0, True, 77, 1, 0)
    d = out - x
    assert torch.equal(d[..., 0], d[..., 1]) and torch.equal(d[..., 0], d[..., 2])
    vals = R.poisson_values(x.cpu().numpy(), True)
    assert int(vals[2, 5, 5, 0]) == 90 and [R.poisson_U(vals[i]) for i in range(3)] == [1, 256, 1]
    check_poisson_sample(d[0, ..., 0].flatten() + 7, 7, 1, "gray v=7")
    check_poisson_sample(d[1, 1:, :, 0].flatten() + 128, 128, 256, "gray v=128 U=256")
    check_poisson_sample(d[2, ..., 0].flatten() + 90, 90, 1, "gray luma 90")


@pytest.mark.parametrize("gray", [False, True])
def test_poisson_U_follows_the_distinct_count(gray):
    """K / U has a resolution of 1 / U: all draws are multiples of it, and not all of 2 / U."""
    for distinct, U in ((1, 1), (2, 2), (3, 4), (128, 128), (129, 256), (256, 256)):
        f = (np.arange(32 * 32) % distinct + (256 - distinct)).astype(np.float32).reshape(1, 32, 32, 1)
        x = dev(np.repeat(f, 3, axis=3))
        assert R.poisson_U(R.poisson_values(x.cpu().numpy(), gray)[0]) == U
        d = (ops.add_poisson_noise(x, 1.0, gray, 5, 0, 0) - x).double()
        assert torch.equal(d * U, (d * U).round()), (distinct, U)
        if U > 1:
            assert not torch.equal(d * (U // 2), (d * (U // 2)).round()), (distinct, U)


@pytest.mark.parametrize("gray", [False, True])
def test_poisson_blocks_equal_one_call(gray):
    x = dev(frames(3, 17, 23, seed=8))                                         # every frame has its own distinct count
    x[1] = (x[1] / 16).round() * 16
    scale = [0.5, 1.0, 2.5]
    whole = ops.add_poisson_noise(x, scale, gray, 31, 4, 6)
    parts = torch.cat([ops.add_poisson_noise(x[:1], scale[:1], gray, 31, 4, 6), ops.add_poisson_noise(x[1:], scale[1:], gray, 31, 4, 7)])
    assert torch.equal(whole, parts)
    assert not torch.equal(whole, ops.add_poisson_noise(x, scale, gray, 31, 5, 6))          # another stream, other draws


# ---- JPEG -------------------------------------------------------------------------------------------------------------------------
QUALITIES = [30, 49, 50, 75, 95, 100]


def jpeg_input(kind, n, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "smooth":
        rng = np.random.default_rng(h * 1000 + w)
        base = np.stack([128 + 100 * np.sin(xx / 9 + yy / 13), 128 + 90 * np.cos(xx / 7 - yy / 11), 128 + 80 * np.sin(xx / 5) * np.cos(yy / 6)], -1)
        return np.clip(base[None] + rng.normal(0, 6, (n, h, w, 3)), 0, 255).astype(np.float32)
    if kind in ("zeros", "full"):
        return np.full((n, h, w, 3), 0.0 if kind == "zeros" else 255.0, dtype=np.float32)
    if kind == "checker":                                                      # the IDCT overshoots 0..255 and is clamped
        return np.broadcast_to((((yy + xx) & 1) * 255.0)[None, ..., None], (n, h, w, 3)).astype(np.float32).copy()
    return np.random.default_rng(h + w).uniform(-40, 300, (n, h, w, 3)).astype(np.float32)      # "wild": clip and truncation


@pytest.mark.parametrize("kind", ["smooth", "zeros", "full", "checker", "wild"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 8, 8), (1, 16, 16), (2, 17, 23), (1, 33, 47), (2, 64, 96)])
def test_jpeg_is_bit_identical_to_the_definition(shape, kind):
    """Every quality in one call: frame j gets QUALITIES[j % 6], so the per-frame array differs across frames."""
    n, h, w = shape
    x = np.concatenate([jpeg_input(kind, n, h, w)] * len(QUALITIES))
    q = [QUALITIES[j // n] for j in range(len(x))]
    got = ops.jpeg_roundtrip(dev(x), q).cpu().numpy()
    want = R.jpeg_roundtrip(x, q)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (shape, kind, np.abs(got.astype(int) - want.astype(int)).max())
    if kind == "smooth" and h >= 16:
        assert not np.array_equal(want[0], want[-1])                           # the qualities do differ in effect
    assert np.array_equal(ops.jpeg_roundtrip(dev(x[:1]), 30).cpu().numpy(), want[:1])       # a scalar quality


# ---- recipes and the tool ---------------------------------------------------------------------------------------------------------
def compose_by_hand(clip_u8, recipe, frame0=0):
    x = clip_u8.cuda().float()
    n = x.shape[0]
    for s in recipe["steps"]:
        if s["op"] == "blur":
            plist = s["params"] if len(s["params"]) == 1 else s["params"][frame0:frame0 + n]
            k = np.stack([D.kernel_from_params(s["family"], s["size"], p) for p in plist]).astype(np.float32)
            x = ops.blur2d(x, dev(k[0] if len(k) == 1 else k))
        elif s["op"] == "resize":
            x = ops.resize(x, s["size"][0], s["size"][1], {"bilinear": L.RESIZE_BILINEAR, "bicubic": L.RESIZE_BICUBIC, "area": L.RESIZE_AREA}[s["mode"]])
        elif s["op"] == "noise":
            fn = ops.add_gaussian_noise if s["kind"] == "gaussian" else ops.add_poisson_noise
            x = fn(x, s["level"][frame0:frame0 + n], s["gray"], recipe["seed"], s["stream_id"], frame0)
        elif s["op"] == "jpeg":
            x = ops.jpeg_roundtrip(x, s["quality"][frame0:frame0 + n]).float()
    return x.clamp(0, 255).to(torch.uint8)


@pytest.fixture(scope="module")
def clip():
    yy, xx = np.mgrid[0:48, 0:64]
    base = np.stack([128 + 100 * np.sin(xx / 9 + yy / 13), 128 + 90 * np.cos(xx / 7 - yy / 11), 128 + 80 * np.sin(xx / 5) * np.cos(yy / 6)], -1)
    fr = np.stack([np.roll(base, 2 * t, axis=1) for t in range(5)]) + np.random.default_rng(0).normal(0, 4, (5, 48, 64, 3))
    return torch.from_numpy(np.clip(fr, 0, 255).astype(np.uint8))


def full_recipe(min_ops=("blur", "resize", "noise", "jpeg")):
    d = D.Degrader(CONFIG, scale=4, seed=0)
    for seed in range(200):
        r = d.recipe(5, 48, 64, seed=seed)
        ops_run = [s["op"] for s in r["steps"]]
        kinds = {s["kind"] for s in r["steps"] if s["op"] == "noise"}
        if all(o in ops_run for o in min_ops) and kinds == {"gaussian", "poisson"}:
            return r
    raise AssertionError("no seed below 200 runs every operator")


def test_apply_recipe_equals_the_hand_composition(clip):
    r = full_recipe()
    got = D.apply_recipe(clip, r)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, 12, 16, 3) and r["output_size"] == [12, 16]
    assert torch.equal(got, compose_by_hand(clip, r))
    blocks = torch.cat([D.apply_recipe(clip[f0:f0 + 2], r, f0) for f0 in (0, 2, 4)])       # --block 2
    assert torch.equal(got, blocks)
    assert len({bytes(f.cpu().numpy().tobytes()) for f in got}) == 5


def run_tool(*args):
    p = subprocess.run([sys.executable, "-m", "dove_amd.degrade", *args], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout


def test_tool_on_png_folder_and_y4m(clip, tmp_path):
    from PIL import Image

    from dove_amd import prepost, y4m, yuv
    src, out1, out2 = tmp_path / "in", tmp_path / "out1", tmp_path / "out2"
    prepost.save_frames_as_png(clip, str(src / "a"))
    fmt = yuv.YuvFormat("444", "bt601", "limited")
    with y4m.Y4MWriter(str(src / "b.y4m"), 64, 48, 16, "444") as wr:
        wr.write(yuv.rgb_to_yuv(clip.cuda(), fmt).cpu())
    run_tool("--input_dir", str(src), "--output_path", str(out1), "--config", CONFIG, "--scale", "4", "--seed", "11", "--block", "2",
             "--png_save")
    for name in ("a", "b"):
        files = sorted(os.listdir(out1 / name))
        assert files == [f"{i:03d}.png" for i in range(5)]
        assert Image.open(out1 / name / "000.png").size == (16, 12)
        recipe = json.load(open(out1 / f"{name}.recipe.json"))
        assert recipe["frames"] == 5 and recipe["input_size"] == [48, 64] and recipe["output_size"] == [12, 16] and recipe["seed"] == 11
    got_a = prepost.load_frames(str(out1 / "a"))
    recipe = json.load(open(out1 / "a.recipe.json"))
    assert torch.equal(got_a, D.apply_recipe(clip, recipe).cpu())              # blocks of 2 in the tool, one block here
    run_tool("--input_dir", str(src), "--output_path", str(out2), "--recipe_in", str(out1 / "a.recipe.json"), "--block", "16")
    assert np.array_equal(np.load(out2 / "a.npy"), got_a.numpy())              # --recipe_in reproduces the bytes
    b_rgb = prepost.load_frames(str(src / "b.y4m"))
    assert np.array_equal(np.load(out2 / "b.npy"), D.apply_recipe(b_rgb, recipe).cpu().numpy())


def test_tool_preset_bicubic_is_the_resize_alone(clip, tmp_path):
    src, out = tmp_path / "in", tmp_path / "out"
    os.makedirs(src)
    np.save(src / "c.npy", clip.numpy())
    run_tool("--input_dir", str(src), "--output_path", str(out), "--preset", "bicubic", "--scale", "4", "--block", "3")
    want = ops.resize(clip.cuda().float(), 12, 16, L.RESIZE_BICUBIC).clamp(0, 255).to(torch.uint8)
    assert np.array_equal(np.load(out / "c.npy"), want.cpu().numpy())
    assert json.load(open(out / "c.recipe.json"))["steps"] == [{"op": "resize", "stage": "preset", "size": [12, 16], "mode": "bicubic"}]
