"""CPU side of the GPU PSNR / SSIM feature: the restated window, the eval tool's pairing / crop / JSON logic, the refusals (mp4,
network metrics, bad arguments through the C ABI) and the new header symbols."""
import json
import os

import numpy as np
import pytest
import torch

import fr_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_equals_fspecial():
    g = R.window_1d()
    np.testing.assert_allclose(np.outer(g, g), R.fspecial(11, 1.5), rtol=0, atol=1e-17)
    assert abs(g.sum() - 1.0) < 1e-15 and np.allclose(g, g[::-1])


def test_restatement_basics():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (2, 3, 20, 24), dtype=np.uint8)
    p, s = R.metrics(a, a)
    assert np.all(p == 80.0) and np.all(s == 1.0)
    base, noisy = R.structured_pair(rng, 1, 40, 50)
    p, s = R.metrics(noisy.transpose(0, 3, 1, 2), base.transpose(0, 3, 1, 2))
    assert 0.05 < s[0] < 0.99 and 15 < p[0] < 40


def test_pairing_output_name_and_summary(tmp_path):
    from dove_amd import eval_metrics as E
    (tmp_path / "gt").mkdir()
    (tmp_path / "pred").mkdir()
    for f in ("x.npy", "y", "z.png"):
        (tmp_path / "gt" / f).touch()
    for f in ("x.npy", "y.npy", "w.npy"):
        (tmp_path / "pred" / f).touch()
    gt, pred = E.pair_files(str(tmp_path / "gt"), str(tmp_path / "pred"))
    assert sorted(gt) == ["x", "y", "z"] and sorted(pred) == ["w", "x", "y"]
    assert pred["y"].endswith("y.npy") and gt["y"].endswith(os.sep + "y")
    assert E.pair_files("", str(tmp_path / "pred"))[0] is None
    assert E.output_name(["psnr", "ssim"]) == "metrics_psnr_ssim.json" and E.output_name(["ssim"]) == "metrics_ssim.json"
    res = {"a": {"psnr": 30.12345, "ssim": 0.5}, "b": {"psnr": 20.0, "ssim": 0.25}}
    out = E.summarize(res, ["psnr", "ssim", "lpips"])
    assert out["count"] == 2 and out["per_sample"] is res
    assert out["average"] == {"psnr": round((30.12345 + 20.0) / 2, 4), "ssim": 0.375}
    assert E.summarize({}, ["psnr"]) == {"per_sample": {}, "average": {}, "count": 0}
    json.dumps(out)


def test_match_resolution_and_crop_are_views():
    from dove_amd import metrics as M
    gt = torch.arange(4 * 9 * 12 * 3, dtype=torch.int32).reshape(4, 9, 12, 3).to(torch.uint8)
    pred = torch.zeros(3, 7, 13, 3, dtype=torch.uint8)
    for center, (top, left) in ((False, (0, 0)), (True, (1, 0))):
        g, p = M.match_resolution(gt, pred, is_center=center)
        assert g.shape == p.shape == (3, 7, 12, 3)
        assert g.data_ptr() == gt[0, top, left].data_ptr() and torch.equal(g, gt[:3, top:top + 7, left:left + 12])
    c = M.crop_border(gt, 2)
    assert c.shape == (4, 5, 8, 3) and c.data_ptr() == gt[0, 2, 2].data_ptr()
    assert M.crop_border(gt, 0) is gt


def test_refusals_without_gpu(tmp_path):
    from dove_amd import cli
    from dove_amd import eval_metrics as E
    from dove_amd import metrics as M
    with pytest.raises(ValueError, match="H.264 decoding"):
        E.load_sequence(str(tmp_path / "clip.mp4"))
    for name in ("lpips", "clipiqa", "dists", "niqe", "psnry"):
        with pytest.raises(NotImplementedError, match="pyiqa"):
            M.create_metric(name)
    with pytest.raises(NotImplementedError, match="pyiqa"):
        M.clip_metrics(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 16, 16, 3, dtype=torch.uint8), "psnr,musiq")
    assert isinstance(M.create_metric("SSIM"), M.FRMetric) and M.create_metric("psnr").to("cpu").eval().metric_name == "psnr"
    with pytest.raises(NotImplementedError, match="pyiqa"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "psnr,lpips", "--gt_dir", str(tmp_path)])
    with pytest.raises(ValueError, match="needs --gt_dir"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "ssim"])
    # init_models reports a metric that cannot be created and keeps the others, as the reference does with pyiqa
    models = E.init_models(["psnr", "clipiqa"], "cpu")
    assert list(models) == ["psnr"]


def _header():
    with open(os.path.join(ROOT, "include", "dove_hip.h")) as f:
        return f.read()


def test_header_symbols_exported_and_abi_refusals():
    import ctypes as C

    from dove_amd import lib as L
    src = _header()
    for sym in ("dove_fr_metrics", "dove_fr_metrics_workspace_bytes", "dove_image_view"):
        assert sym in src
    assert "dove_fr_metrics" in L.SIGNATURES and "dove_fr_metrics_workspace_bytes" in L.PLAIN
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    assert lib.dove_abi_version() == 15
    assert lib.dove_fr_metrics_workspace_bytes(2, 720, 1280) == 2 * 23 * 20 * 16
    assert lib.dove_fr_metrics_workspace_bytes(0, 720, 1280) == 0
    v = L.ImageView()                                            # data, ws and out stay NULL: no call here can reach a launch
    v.dtype, v.sn, v.sc, v.sh, v.sw = L.U8, 3 * 64 * 64, 1, 64 * 3, 3
    need = lib.dove_fr_metrics_workspace_bytes(1, 64, 64)

    def call(ch=3, h=64, w=64, flags=3, nbytes=need):
        return lib.dove_fr_metrics(C.byref(v), C.byref(v), 1, ch, h, w, flags, None, nbytes, None, None)

    for kw, msg in ((dict(ch=2), b"channels must be 1 or 3"), (dict(h=10), b"SSIM needs H and W >= 11"),
                    (dict(w=8), b"SSIM needs H and W >= 11"), (dict(ch=1, flags=7), b"rgb_to_y needs 3-channel"),
                    (dict(nbytes=need - 1), b"too small"), (dict(flags=4), b"flags"), (dict(flags=9), b"flags")):
        assert call(**kw) == -1 and msg in lib.dove_last_error(), (kw, lib.dove_last_error())
    assert call() == -1 and b"null pointer" in lib.dove_last_error()     # valid arguments: the pointers are checked last
    assert C.sizeof(L.ImageView) == 48
