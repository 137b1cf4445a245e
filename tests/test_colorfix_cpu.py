"""CPU side of the GPU colour fix: the float64 restatement (tests/colorfix_ref.py) pinned to the reference's recorded fp32 outputs
(tests/golden/colorfix_golden.npz, tools/make_colorfix_goldens.py), its algebra, the new header symbols, the refusals of the C call, of
the CLI and of the standalone tool."""
import os

import numpy as np
import pytest
import torch

import colorfix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"a": (2, 3, 45, 37), "b": (1, 3, 9, 12), "c": (1, 3, 72, 104)}
MODES = ("wavelet", "adain")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "colorfix_golden.npz"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_reference_fp32(golden, case, mode):
    """e_ref = max |reference fp32 - restatement f64|: the reference's own distance from float64, and what pins the restatement to it."""
    c, s, ref32 = golden[f"{case}_content"], golden[f"{case}_style"], golden[f"{case}_{mode}"]
    assert c.shape == CASES[case] and c.dtype == s.dtype == ref32.dtype == np.float32
    assert np.array_equal(R.bf16_round(c), c) and np.array_equal(R.bf16_round(s), s)      # inputs are exact in bfloat16
    want = R.fix(c, s, mode)
    e_ref = float(np.abs(ref32.astype(np.float64) - want).max())
    print(f"[colorfix] case {case} {mode}: e_ref = {e_ref:.3e}")
    assert 0.0 < e_ref < 1e-6
    # the reference's own fp32 result, truncated to uint8, stays inside the uint8 gate of the GPU test
    worst, share = R.u8_gate(R.to_u8(ref32.astype(np.float64)), R.to_u8(want))
    assert worst <= 1 and share <= 1e-3


@pytest.mark.parametrize("shape", [(1, 3, 45, 37), (2, 3, 9, 12), (1, 3, 70, 90), (1, 3, 1, 1), (1, 3, 1, 40), (1, 3, 33, 1)])
def test_wavelet_forms_agree_in_float64(shape):
    rng = np.random.default_rng(sum(shape))
    c, s = rng.random(shape), rng.random(shape)
    np.testing.assert_allclose(R.wavelet(c, s), R.wavelet_two_pyramids(c, s), rtol=0, atol=1e-14)


def test_blur_is_replicate_padded_dilated_conv():
    """B_r against torch's own replicate pad + dilated depthwise conv2d in float64 (what the definition says, from a second source)."""
    rng = np.random.default_rng(5)
    x = rng.random((2, 3, 19, 23))
    k = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
    k2 = (k[:, None] * k[None, :] / 16.0)[None, None].repeat(3, 1, 1, 1)
    for r in R.RADII:                                           # radius 16 and 8 exceed half the image: every tap pattern occurs
        t = torch.nn.functional.pad(torch.from_numpy(x), (r, r, r, r), mode="replicate")
        want = torch.nn.functional.conv2d(t, k2, groups=3, dilation=r).numpy()
        np.testing.assert_allclose(R.blur(x, r), want, rtol=0, atol=1e-15)


def test_identity_and_constant_offset():
    rng = np.random.default_rng(6)
    c = 0.2 + 0.5 * rng.random((2, 3, 40, 52))
    for mode in MODES:
        np.testing.assert_allclose(R.fix(c, c, mode), c, rtol=0, atol=1e-14)          # identical content and style: content
        np.testing.assert_allclose(R.fix(c, c + 0.125, mode), c + 0.125, rtol=0, atol=1e-14)   # style = content + c, away from the clamp
    one = rng.random((1, 3, 1, 1))
    two = rng.random((1, 3, 1, 1))
    np.testing.assert_allclose(R.wavelet(one, two), one + (two - one), rtol=0, atol=0)
    assert np.array_equal(R.to_u8(np.array([-0.1, 0.0, 0.999, 1.0, 1.2, 127.5 / 255])), np.array([0, 0, 254, 255, 255, 127], np.uint8))


def test_adain_statistics_are_unbiased():
    rng = np.random.default_rng(7)
    c, s = rng.random((2, 3, 11, 13)), rng.random((2, 3, 11, 13))
    out = R.adain(c, s)
    flat = out.reshape(2, 3, -1)
    np.testing.assert_allclose(flat.mean(2), s.reshape(2, 3, -1).mean(2), atol=1e-13)
    want_std = np.sqrt(s.reshape(2, 3, -1).var(2, ddof=1) + 1e-5)
    got_std = flat.std(2, ddof=1) * np.sqrt(c.reshape(2, 3, -1).var(2, ddof=1) + 1e-5) / c.reshape(2, 3, -1).std(2, ddof=1)
    np.testing.assert_allclose(got_std, want_std, rtol=1e-12)


def test_header_symbols_exported_and_abi_refusals():
    import ctypes as C

    from dove_amd import lib as L
    with open(os.path.join(ROOT, "include", "dove_hip.h")) as f:
        src = f.read()
    for sym in ("dove_color_fix", "dove_color_fix_workspace_bytes", "DOVE_COLORFIX_WAVELET", "DOVE_COLORFIX_ADAIN", "DOVE_COLORFIX_CLAMP"):
        assert sym in src
    assert "#define DOVE_ABI_VERSION 15" in src
    assert "dove_color_fix" in L.SIGNATURES and "dove_color_fix_workspace_bytes" in L.PLAIN
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    assert lib.dove_abi_version() == 15
    W, A = L.COLORFIX_WAVELET, L.COLORFIX_ADAIN
    assert lib.dove_color_fix_workspace_bytes(W, 2, 720, 1280) == 2 * 2 * 3 * 720 * 1280 * 4
    assert 0 < lib.dove_color_fix_workspace_bytes(A, 2, 720, 1280) <= 2 * 128 * 12 * 8
    assert lib.dove_color_fix_workspace_bytes(W, 0, 720, 1280) == 0 and lib.dove_color_fix_workspace_bytes(7, 1, 8, 8) == 0
    v, o = L.ImageView(), L.ImageView()                          # data and ws stay NULL: no call here can reach a launch
    for x in (v, o):
        x.dtype, x.sn, x.sc, x.sh, x.sw = L.F32, 3 * 64 * 64, 64 * 64, 64, 1
    need = lib.dove_color_fix_workspace_bytes(W, 1, 64, 64)

    def call(mode=W, flags=1, n=1, h=64, w=64, nbytes=need, content=v, style=v, out=o, ws=None):
        ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
        return lib.dove_color_fix(ref(content), 1.0, 0.0, ref(style), 1.0, 0.0, n, h, w, mode, flags, ref(out), ws, nbytes, None)

    bad = L.ImageView()
    bad.dtype = 3
    for kw, msg in ((dict(mode=0), b"bad mode"), (dict(mode=3), b"bad mode"), (dict(flags=2), b"bad flags"), (dict(h=0), b"bad shape"),
                    (dict(n=-1), b"bad shape"), (dict(mode=A, h=1, w=1, nbytes=1 << 20), b"at least 2 pixels"),
                    (dict(content=bad), b"bad dtype"), (dict(out=bad), b"bad dtype"), (dict(nbytes=need - 1), b"too small"),
                    (dict(content=None), b"null view"), (dict(out=None), b"null view")):
        assert call(**kw) == -1 and msg in lib.dove_last_error(), (kw, lib.dove_last_error())
    assert call() == -1 and b"null pointer" in lib.dove_last_error()       # valid arguments: the pointers are checked last
    # garbage (non-null) data pointers with a null workspace still stop at the pointer check
    v.data = o.data = 0x1000
    assert call() == -1 and b"null pointer" in lib.dove_last_error()
    assert call(mode=A, h=1, w=2, nbytes=1 << 20) == -1 and b"null pointer" in lib.dove_last_error()     # 2 pixels are enough for adain


def test_python_refusals_without_gpu():
    from dove_amd import colorfix
    z = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="mode must be one of"):
        colorfix.color_fix(z, z, "bogus")
    assert set(colorfix.MODES) == {"wavelet", "adain"}
    for fn in ("wavelet_reconstruction", "adaptive_instance_normalization", "color_fix", "main"):
        assert callable(getattr(colorfix, fn))
    from dove_amd import prepost
    with pytest.raises(ValueError, match="needs source"):
        prepost.postprocess_frames(torch.zeros(1, 3, 5, 8, 8), 0, 0, 0, color_fix="wavelet")


def test_cli_refuses_unknown_color_fix(tmp_path, capsys):
    from dove_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--input_dir", str(tmp_path), "--color_fix", "bogus"])
    assert e.value.code == 2
    assert "--color_fix" in capsys.readouterr().err


def test_tool_pairing_factor_and_mp4_refusal(tmp_path, capsys):
    from dove_amd import colorfix
    pred, src, out = tmp_path / "pred", tmp_path / "src", tmp_path / "out"
    pred.mkdir()
    src.mkdir()
    for f in ("x.npy", "y", "w.npy"):
        (pred / f).touch()
    for f in ("x.npy", "y.npy", "z.png"):
        (src / f).touch()
    s_files, p_files = colorfix.pair_files(str(src), str(pred))
    assert sorted(p_files) == ["w", "x", "y"] and sorted(s_files) == ["x", "y", "z"]
    assert s_files["y"].endswith("y.npy") and p_files["y"].endswith(os.sep + "y")
    with pytest.raises(ValueError, match="not a folder"):
        colorfix.pair_files(str(tmp_path / "nope"), str(pred))
    assert colorfix.upscale_factor((5, 64, 96, 3), (5, 64, 96, 3)) == 1
    assert colorfix.upscale_factor((5, 64, 96, 3), (5, 16, 24, 3)) == 4
    assert colorfix.upscale_factor((5, 64, 96, 3), (5, 16, 32, 3)) is None
    assert colorfix.upscale_factor((5, 64, 96, 3), (5, 60, 96, 3)) is None
    assert colorfix.upscale_factor((5, 16, 24, 3), (5, 64, 96, 3)) is None
    # mp4 is refused with the wording of prepost.load_frames
    p2, s2 = tmp_path / "p2", tmp_path / "s2"
    p2.mkdir()
    s2.mkdir()
    (p2 / "clip.mp4").touch()
    (s2 / "clip.mp4").touch()
    with pytest.raises(ValueError, match="H.264 decoding"):
        colorfix.main(["--pred", str(p2), "--source", str(s2), "--out", str(out), "--mode", "wavelet"])
    with pytest.raises(SystemExit):
        colorfix.main(["--pred", str(p2), "--source", str(s2), "--out", str(out), "--mode", "bogus"])
    capsys.readouterr()
    # a prediction without a source is skipped with a message, before anything is loaded
    (s2 / "clip.mp4").unlink()
    assert colorfix.main(["--pred", str(p2), "--source", str(s2), "--out", str(out)]) == []
    assert "Skipping clip: no matching source file." in capsys.readouterr().out
