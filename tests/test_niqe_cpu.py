"""NIQE without a GPU: the restatement's own footing (tests/niqe_ref.py), the C ABI's refusals with NULL data pointers, the host-side
dove_niqe_distance against numpy.linalg.pinv, the model loader and the refusals of the command lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import niqe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib():
    from dove_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_general_imresize_at_half_is_the_eight_tap_filter():
    """The kernel's fixed taps [-3 -9 29 111 111 29 -9 -3] / 256 at source 2i-3 .. 2i+4 with symmetric reflection are what MATLAB's general
    antialiased bicubic weights reduce to at exactly 0.5.  All weights are dyadic, so on an integer image the two agree bit for bit."""
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (12, 20)).astype(np.float64)
    out = R.imresize(a, 0.5)
    assert out.shape == (6, 10) and np.array_equal(out, R.half_eight_taps(a))
    w, idx = R.imresize_weights(12, 0.5)
    nz = np.abs(w).sum(axis=0) > 0                                # the general computation carries two all-zero columns
    assert np.array_equal(w[:, nz], np.tile(R.EIGHT_TAPS, (6, 1)))
    assert idx[0, nz].tolist() == [2, 1, 0, 0, 1, 2, 3, 4] and idx[5, nz].tolist() == [7, 8, 9, 10, 11, 11, 10, 9]
    b = rng.random((12, 20))                                      # non-integer values: equal up to the order of the sums
    assert np.abs(R.imresize(b, 0.5) - R.half_eight_taps(b)).max() <= 8 * EPS


def test_r_of_gamma_is_strictly_increasing():
    """The solve kernel finds alpha by a binary search over r(gam); that equals the first-index argmin only because r is strictly
    increasing over the whole grid, with steps far above the rounding of the table."""
    d = np.diff(R.R_GAM)
    assert R.GAM.shape == (9801,) and abs(R.GAM[0] - 0.2) < 1e-15 and abs(R.GAM[-1] - 10.0) < 1e-12
    assert (d > 0).all() and d.min() > 1e-7 > 1e6 * EPS


def test_header_symbols_bound_and_abi_refusals(lib):
    from dove_amd import lib as L
    with open(os.path.join(ROOT, "include", "dove_hip.h")) as f:
        src = f.read()
    for sym in ("dove_niqe_features", "dove_niqe_stats", "dove_niqe_distance"):
        assert re.search(rf"\b{sym}\(", src) and sym in L.SIGNATURES
    assert "dove_niqe_workspace_bytes(" in src and "dove_niqe_workspace_bytes" in L.PLAIN
    assert lib.dove_abi_version() == 15
    assert lib.dove_niqe_workspace_bytes(0, 720, 1280) == 0 and lib.dove_niqe_workspace_bytes(1, 95, 1280) == 0
    # per image and block: 2 x 31 moments and the 48 x 48 tile of the half-scale image, fp64
    assert lib.dove_niqe_workspace_bytes(2, 720, 1280) == 2 * 7 * 13 * (62 + 48 * 48) * 8
    v = L.ImageView()                                            # data, ws and the outputs stay NULL: no call here can reach a launch
    v.dtype, v.sn, v.sc, v.sh, v.sw = L.U8, 3 * 96 * 96, 1, 96 * 3, 3
    need = lib.dove_niqe_workspace_bytes(1, 96, 96)

    def call(ch=3, h=96, w=96, nbytes=need):
        return lib.dove_niqe_features(C.byref(v), 1, ch, h, w, None, nbytes, None, None, None)

    for kw, msg in ((dict(ch=2), b"channels must be 1 or 3"), (dict(ch=4), b"channels must be 1 or 3"), (dict(h=95), b"H and W >= 96"),
                    (dict(w=64), b"H and W >= 96"), (dict(nbytes=need - 1), b"too small")):
        assert call(**kw) == -1 and msg in lib.dove_last_error(), (kw, lib.dove_last_error())
    assert call() == -1 and b"null pointer" in lib.dove_last_error()     # valid arguments: the pointers are checked last
    assert lib.dove_niqe_stats(None, 1, 4, None, None, None, None) == -1 and b"null pointer" in lib.dove_last_error()
    assert lib.dove_niqe_stats(None, 1, 0, None, None, None, None) == -1 and b"bad shape" in lib.dove_last_error()
    assert lib.dove_niqe_distance(None, None, None, None, None) == -1 and b"null pointer" in lib.dove_last_error()


def _spd(rng, rank=36, scale=1.0):
    a = rng.standard_normal((36, rank))
    return scale * (a @ a.T) / rank


def test_distance_against_numpy_pinv(lib):
    """dove_niqe_distance (host code: Jacobi eigen-solve, pinv cut at 36 eps sigma_max) against numpy.linalg.pinv with the same cut, at
    1e-10 relative: both sides are fp64 on the host and the eigen-solve is backward stable."""
    from dove_amd import ops
    rng = np.random.default_rng(3)
    mu_a, mu_b = rng.standard_normal(36), rng.standard_normal(36)
    # a well-conditioned pair
    ca, cb = _spd(rng) + 0.1 * np.eye(36), _spd(rng, scale=3.0) + 0.1 * np.eye(36)
    want = R.distance(mu_a, ca, mu_b, cb)
    got = ops.niqe_distance(mu_a, ca, mu_b, cb)
    print(f"well-conditioned: {got!r} vs {want!r}, rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-10 * want
    # a pooled covariance of rank 30 of 36: six singular values are rounding noise and must be cut, or the score explodes
    basis = np.linalg.qr(rng.standard_normal((36, 36)))[0]
    lam = np.concatenate([np.linspace(0.5, 4.0, 30), np.zeros(6)])
    pooled = (basis * lam) @ basis.T
    ca = 0.4 * pooled
    cb = 2.0 * pooled - ca                                        # (ca + cb) / 2 = pooled up to rounding
    sv = np.linalg.svd((ca + cb) / 2, compute_uv=False)
    assert sv[29] > 0.4 and sv[30] < 36 * EPS * sv[0]
    want = R.distance(mu_a, ca, mu_b, cb)
    got = ops.niqe_distance(mu_a, ca, mu_b, cb)
    print(f"rank 30: {got!r} vs {want!r}, rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-10 * want
    # identical models
    assert ops.niqe_distance(mu_a, ca, mu_a, ca) == 0.0
    # a NaN anywhere is a NaN score, not an error (an image with fewer than two NaN-free blocks)
    bad = cb.copy()
    bad[3, 4] = np.nan
    assert np.isnan(ops.niqe_distance(mu_a, ca, mu_b, bad)) and np.isnan(ops.niqe_distance(np.full(36, np.nan), ca, mu_b, cb))
    with pytest.raises(ValueError, match="shapes"):
        ops.niqe_distance(mu_a[:35], ca, mu_b, cb)


def test_model_load_round_trips_and_names_bad_keys(tmp_path):
    from dove_amd import niqe
    rng = np.random.default_rng(5)
    mu, cov = rng.standard_normal(36), _spd(rng)
    niqe.NiqeModel(mu, cov).save(str(tmp_path / "niqe_fit.npz"))
    m = niqe.NiqeModel.load(str(tmp_path / "niqe_fit.npz"))
    assert np.array_equal(m.mu, mu) and np.array_equal(m.cov, cov) and m.to("cpu") is m
    np.savez(tmp_path / "short.npz", mu=mu[:30], cov=cov)
    with pytest.raises(ValueError, match=r"'mu' has shape \(30,\)"):
        niqe.NiqeModel.load(str(tmp_path / "short.npz"))
    np.savez(tmp_path / "flat.npz", mu=mu, cov=cov.reshape(-1))
    with pytest.raises(ValueError, match=r"'cov' has shape \(1296,\)"):
        niqe.NiqeModel.load(str(tmp_path / "flat.npz"))
    np.savez(tmp_path / "nocov.npz", mu=mu)
    with pytest.raises(KeyError, match="'cov' is missing"):
        niqe.NiqeModel.load(str(tmp_path / "nocov.npz"))
    with pytest.raises(ValueError, match="cov must be"):
        niqe.NiqeModel(mu, cov[:35])
    # the directory search: the .mat of pyiqa first, then a fitted .npz; nothing is a FileNotFoundError naming both patterns
    assert niqe.find_model_file(str(tmp_path)).endswith("niqe_fit.npz")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match=r"niqe_modelparameters\*\.mat or niqe\*\.npz in .*empty"):
        niqe.load_model(str(empty))


def test_model_load_mat(tmp_path):
    sio = pytest.importorskip("scipy.io")
    from dove_amd import niqe
    rng = np.random.default_rng(6)
    mu, cov = rng.standard_normal((1, 36)), _spd(rng)
    sio.savemat(str(tmp_path / "niqe_modelparameters.mat"), {"mu_prisparam": mu, "cov_prisparam": cov})
    np.savez(tmp_path / "niqe_fit.npz", mu=mu[0] + 1, cov=cov)
    m = niqe.load_model(str(tmp_path))                            # the .mat wins over the .npz
    assert m.mu.shape == (36,) and np.array_equal(m.mu, mu[0]) and np.array_equal(m.cov, cov)
    sio.savemat(str(tmp_path / "bad.mat"), {"mu_prisparam": mu, "cov_prisparam": cov[:, :20]})
    with pytest.raises(ValueError, match=r"'cov_prisparam' has shape \(36, 20\)"):
        niqe.NiqeModel.load(str(tmp_path / "bad.mat"))
    sio.savemat(str(tmp_path / "nomu.mat"), {"cov_prisparam": cov})
    with pytest.raises(KeyError, match="'mu_prisparam' is missing"):
        niqe.NiqeModel.load(str(tmp_path / "nomu.mat"))


def test_create_metric_and_python_refusals():
    from dove_amd import metrics as M
    from dove_amd import niqe
    with pytest.raises(NotImplementedError, match="pyiqa"):
        M.create_metric("niqe")                                   # no model: as before
    rng = np.random.default_rng(7)
    model = niqe.NiqeModel(rng.standard_normal(36), _spd(rng))
    m = M.create_metric("NIQE", weights=model)
    assert isinstance(m, niqe.NiqeMetric) and m.lower_better is True and m.metric_name == "niqe"
    with pytest.raises(TypeError, match="NiqeModel"):
        M.create_metric("niqe", weights=object())
    with pytest.raises(NotImplementedError, match="default options"):
        M.create_metric("niqe", weights=model, crop_border=4)
    with pytest.raises(NotImplementedError, match="weights belong to"):
        M.create_metric("ssim", weights=model)
    with pytest.raises(ValueError, match="at least 96"):
        niqe.features(torch.zeros(1, 3, 95, 200, dtype=torch.uint8))
    with pytest.raises(ValueError, match="1 or 3 channels"):
        niqe.features(torch.zeros(1, 2, 96, 96))
    with pytest.raises(TypeError, match="NiqeModel"):
        niqe.niqe(None, torch.zeros(1, 3, 96, 96))
    with pytest.raises(NotImplementedError, match="pyiqa"):
        M.nr_clip_metrics(torch.zeros(1, 96, 96, 3, dtype=torch.uint8), ["niqe"], {})


def test_command_lines_refuse_and_skip(tmp_path, capsys, monkeypatch):
    from dove_amd import cli, eval_metrics
    wdir, pred = tmp_path / "w", tmp_path / "pred"
    wdir.mkdir()
    pred.mkdir()
    # a requested metric whose file is absent: FileNotFoundError naming the patterns and the directory
    with pytest.raises(FileNotFoundError, match=r"niqe_modelparameters\*\.mat or niqe\*\.npz in .*w"):
        eval_metrics.load_weights(["psnr", "niqe"], str(wdir))
    assert eval_metrics.load_weights(["psnr", "niqe"], "") == {}
    with pytest.raises(FileNotFoundError, match=r"niqe\*\.npz"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "niqe", "--metric_weights", str(wdir)])
    # niqe without --metric_weights stays outside the path; a full-reference metric keeps needing --gt_dir, alone or beside niqe
    with pytest.raises(NotImplementedError, match="niqe"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "niqe"])
    with pytest.raises(ValueError, match="needs --gt_dir"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "psnr,niqe", "--metric_weights", str(wdir)])
    with pytest.raises(ValueError, match="needs --gt_dir"):
        cli.main(["--input_dir", str(tmp_path), "--eval_metrics", "ssim"])
    # without a model niqe fails to initialise with a message, as a pyiqa metric that cannot be created does in the reference
    assert eval_metrics.init_models(["niqe"]) == {} and "pyiqa" in capsys.readouterr().out
    # no --gt and only full-reference metrics: every clip is skipped with the reference's message
    np.save(pred / "a.npy", np.zeros((1, 96, 96, 3), np.uint8))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    out = eval_metrics.main(["--pred", str(pred), "--out", str(tmp_path), "--metrics", "psnr,ssim"])
    assert out["count"] == 0 and "Skipping a: GT is not provided and no NR-IQA metrics found." in capsys.readouterr().out


def test_gt_free_json_from_a_stubbed_metric(tmp_path, monkeypatch):
    """The ground-truth-free path of the evaluation tool, with the device work stubbed out: niqe alone is computed on the predictions and
    written to the same JSON; with --gt the clip function receives niqe beside the full-reference metrics."""
    import json

    from dove_amd import eval_metrics
    from dove_amd import metrics as M
    gt, pred, wdir = tmp_path / "gt", tmp_path / "pred", tmp_path / "w"
    for d in (gt, pred, wdir):
        d.mkdir()
    for name in ("a", "b"):
        np.save(gt / f"{name}.npy", np.zeros((2, 96, 96, 3), np.uint8))
        np.save(pred / f"{name}.npy", np.zeros((2, 96, 96, 3), np.uint8))
    rng = np.random.default_rng(8)
    np.savez(wdir / "niqe_model.npz", mu=rng.standard_normal(36), cov=_spd(rng))
    seen = []

    def nr_stub(pred_u8, names, weights):
        seen.append(("nr", tuple(pred_u8.shape), list(names), sorted(weights)))
        return {"niqe": 5.123449}

    def clip_stub(pred_u8, gt_u8, names, crop=0, test_y_channel=False, is_center=False, name=None, weights=None):
        seen.append(("fr", name, list(names), crop, sorted(weights)))
        return {"psnr": 30.5, "niqe": 4.25}

    monkeypatch.setattr(M, "nr_clip_metrics", nr_stub)
    monkeypatch.setattr(M, "clip_metrics", clip_stub)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    out = eval_metrics.main(["--pred", str(pred), "--out", str(tmp_path), "--metrics", "niqe", "--metric_weights", str(wdir), "--crop", "4"])
    assert seen == [("nr", (2, 96, 96, 3), ["niqe"], ["niqe"])] * 2
    with open(tmp_path / "metrics_niqe.json") as f:
        assert json.load(f) == out == {"per_sample": {"a": {"niqe": 5.1234}, "b": {"niqe": 5.1234}}, "average": {"niqe": 5.1234}, "count": 2}
    del seen[:]
    out = eval_metrics.main(["--gt", str(gt), "--pred", str(pred), "--out", str(tmp_path), "--metrics", "psnr,niqe", "--metric_weights",
                             str(wdir), "--crop", "4"])
    assert seen == [("fr", "a", ["psnr", "niqe"], 4, ["niqe"]), ("fr", "b", ["psnr", "niqe"], 4, ["niqe"])]
    assert out["per_sample"]["a"] == {"psnr": 30.5, "niqe": 4.25} and out["count"] == 2
