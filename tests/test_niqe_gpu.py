"""GPU NIQE (csrc/niqe.hip via dove_amd.niqe) against the fp64 restatement in tests/niqe_ref.py: the features per block (alpha as a grid
index), NaN semantics, every input form, the score, the fit, determinism, and the two command lines without ground truth.

The inputs are niqe_ref.make_image(seed, h, w): a ramp plus region-wise Gaussian / uniform / Laplacian noise, so that alpha spans about
0.8 .. 3.4.  For every (shape, seed) used here the restatement against itself with its MSCN fields perturbed by 1e-13 relative (three
seeded draws) shows no alpha moving to a neighbouring grid point, so a flip in a comparison below is an arithmetic error, not a
coin toss."""
import json
import os

import numpy as np
import pytest
import torch

import niqe_ref as R

pytestmark = pytest.mark.gpu

ALPHA_COLS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]               # the alpha of each (scale, product) in the 36-vector
RTOL = 1e-9                                                       # sums of at most 9216 fp64 terms: n eps ~ 2e-12, with margin for I - mu


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_blocks():
    """These tests allocate large odd-sized tensors (a 720 x 1280 frame, the 55 MB scratch of a clip).  Freed, they stay in torch's
    caching allocator, where a later request that almost fits takes a whole block; tests that compare peak allocated bytes (the streaming
    tool's bounded-memory test) then see this module's leftovers.  Hand the blocks back when the module is done."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def seed_of(h, n):
    return 1000 + 10 * h + n


def clip_u8(h, w, n=2):
    return np.stack([R.make_image(seed_of(h, i), h, w) for i in range(n)])


_REF = {}


def reference(h, w, n=2):
    """The restatement's (features [n,B,36], sharpness [n,B], alpha indices [n,B,10]) of clip_u8(h, w, n): computed once, shared, read-only."""
    if (h, w, n) not in _REF:
        out = [R.features(f) for f in clip_u8(h, w, n)]
        arrs = tuple(np.stack([o[k] for o in out]) for k in range(3))
        for a in arrs:
            a.setflags(write=False)
        _REF[(h, w, n)] = arrs
    return _REF[(h, w, n)]


def alpha_index(alpha):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(alpha), -1, np.rint((alpha - 0.2) / 0.001)).astype(np.int64)


def check_features(got_f, got_s, want_f, want_s, want_idx):
    """alpha as a grid index: at most 1 entry in 1000 may differ, by one step; everything else at RTOL, NaN exactly where the oracle's is."""
    assert got_f.shape == want_f.shape and got_s.shape == want_s.shape
    assert np.array_equal(np.isnan(got_f), np.isnan(want_f))
    idx = alpha_index(got_f[..., ALPHA_COLS])
    diff = np.abs(idx - want_idx)
    allowed = want_idx.size // 1000
    print(f"alpha entries {want_idx.size}, differing {int((diff > 0).sum())} (allowed {allowed}), largest step {int(diff.max())}")
    assert int((diff > 0).sum()) <= allowed and diff.max() <= 1
    # the features of a product whose alpha moved by a step follow the other grid point: they are compared where alpha agrees
    same = np.ones(want_f.shape, dtype=bool)
    groups = [(0, 2)] + [(2 + 4 * k, 6 + 4 * k) for k in range(4)]
    for s in range(2):
        for p, (a, b) in enumerate(groups):
            same[..., 18 * s + a:18 * s + b] = (diff[..., 5 * s + p] == 0)[..., None]
    ok = same & ~np.isnan(want_f)
    rel = np.abs(got_f[ok] - want_f[ok]) / np.abs(want_f[ok])
    rel_s = np.abs(got_s - want_s) / np.abs(want_s)
    print(f"features: largest relative difference {rel.max():.3e}; sharpness {rel_s.max():.3e}")
    assert rel.max() <= RTOL and rel_s.max() <= RTOL


def pristine_model(F):
    """A seeded synthetic pristine model for a clip with features F [n,B,36]: mu_p near the clip's own mu_d, cov_p SPD."""
    rng = np.random.default_rng(11)
    mu_d = np.nanmean(F.reshape(-1, 36), axis=0)
    a = rng.standard_normal((36, 36))
    return mu_d * (1.0 + 0.05 * rng.standard_normal(36)), 0.01 * (a @ a.T / 36 + 0.1 * np.eye(36))


@pytest.mark.parametrize("h,w", [(96, 96), (192, 288), (200, 300)])
def test_features_vs_oracle_u8_frames(h, w):
    """96x96: one block, every border is a pad.  192x288: interior block edges (a roll that leaks into the next block shows).  200x300:
    cropping after filtering instead of before shows."""
    from dove_amd import niqe
    f, s = niqe.features(torch.from_numpy(clip_u8(h, w)).cuda())
    assert f.dtype == torch.float64 and tuple(f.shape) == (2, (h // 96) * (w // 96), 36)
    check_features(f.cpu().numpy(), s.cpu().numpy(), *reference(h, w))


def test_production_shape_once():
    """One 720x1280 frame (7 x 13 blocks): the launch geometry at the real size, under the same criteria."""
    from dove_amd import niqe
    f, s = niqe.features(torch.from_numpy(clip_u8(720, 1280, 1)).cuda())
    assert tuple(f.shape) == (1, 91, 36)
    check_features(f.cpu().numpy(), s.cpu().numpy(), *reference(720, 1280, 1))


def test_nan_semantics():
    """A flat region covering block (0,0) and its 3-pixel filter margin: that block's scale-1 features are all NaN, and NaN sits exactly
    where the oracle has it; nanmean, the NaN-free covariance and both counts follow.  An all-constant frame scores NaN without raising."""
    from dove_amd import niqe, ops
    img = R.make_image(7, 192, 192)
    img[:99, :99] = 120
    wf, ws, _ = R.features(img)
    # grey level 120 is one of those for which the restatement's plain sum g_k c is exact, so its flat region is exactly flat (for about
    # half of the levels the rounding leaves 1 ulp, and a flat region is then all-negative or all-positive; the kernel's moments of
    # I - c are exact for every level)
    assert ws[0] == 0.0
    assert np.isnan(wf[0, :18]).all() and not np.isnan(wf[1:]).any() and not np.isnan(wf[0, 18:]).all()
    f, s = niqe.features(torch.from_numpy(img)[None].cuda())
    gf = f.cpu().numpy()[0]
    assert np.array_equal(np.isnan(gf), np.isnan(wf))
    ok = ~np.isnan(wf)
    assert (np.abs(gf[ok] - wf[ok]) <= RTOL * np.abs(wf[ok])).all()
    assert (np.abs(s.cpu().numpy()[0] - ws) <= RTOL * np.abs(ws) + 1e-300).all()
    mu, cov, counts = ops.niqe_stats(f)
    wmu, wcov, wcounts = R.stats(wf)
    assert tuple(counts.cpu().numpy()[0]) == wcounts == (3, 4)
    assert np.allclose(mu.cpu().numpy()[0], wmu, rtol=RTOL, atol=0)
    scale = np.sqrt(np.outer(np.diag(wcov), np.diag(wcov)))       # covariances cancel: compared against the size of the variances
    assert (np.abs(cov.cpu().numpy()[0] - wcov) <= RTOL * scale).all()
    model = niqe.NiqeModel(*pristine_model(wf[None]))
    flat = torch.full((1, 192, 192, 3), 77, dtype=torch.uint8).cuda()
    ff, _ = niqe.features(flat)
    assert torch.isnan(ff).all()
    _, _, c = ops.niqe_stats(ff)
    assert c.cpu().tolist() == [[0, 0]]
    score = niqe.niqe(model, flat)
    assert tuple(score.shape) == (1,) and torch.isnan(score).all()
    one = niqe.niqe(model, torch.from_numpy(img[:96, 96:])[None].cuda())   # one NaN-free block: no covariance, NaN as well
    assert torch.isnan(one).all()


def test_input_forms():
    """float32 NCHW one-channel input against the oracle; a crop of a larger tensor and a permuted tensor bit-equal to their dense copies;
    host frames handed to the create_metric module, as the reference's loop does."""
    from dove_amd import metrics as M
    from dove_amd import niqe
    g = torch.Generator().manual_seed(3)
    base = torch.from_numpy(R.make_image(21, 192, 200, channels=1)).permute(2, 0, 1).float() / 255.0        # [1,H,W]
    x = (base + 0.001 * torch.rand(base.shape, generator=g)).clamp(0, 1)[None]                              # not on the u8 lattice
    f, s = niqe.features(x.cuda())
    wf, ws, widx = R.features(x[0].numpy())
    check_features(f.cpu().numpy(), s.cpu().numpy(), wf[None], ws[None], widx[None])
    big = torch.rand(2, 3, 230, 260, generator=g).cuda()
    crop = big[:, :, 5:5 + 200, 7:7 + 196]
    assert not crop.is_contiguous()
    fa, sa = niqe.features(crop)
    fb, sb = niqe.features(crop.contiguous())
    assert torch.equal(fa, fb) and torch.equal(sa, sb)
    nhwc = torch.rand(2, 200, 196, 3, generator=g).cuda()
    perm = nhwc.permute(0, 3, 1, 2)
    assert torch.equal(niqe.features(perm)[0], niqe.features(perm.contiguous())[0])
    u8 = torch.from_numpy(clip_u8(192, 288)).cuda()
    assert torch.equal(niqe.features(u8)[0], niqe.features(u8.permute(0, 3, 1, 2).contiguous())[0])         # frames = their NCHW copy
    wf = reference(192, 288)[0]
    model = niqe.NiqeModel(*pristine_model(wf))
    metric = M.create_metric("niqe", weights=model).to("cuda").eval()
    host = torch.from_numpy(clip_u8(192, 288)).permute(0, 3, 1, 2).float() / 255.0                          # host [N,3,H,W] in [0,1]
    got = metric(host)
    assert got.is_cuda and got.dtype == torch.float64 and torch.equal(got, niqe.niqe(model, host.cuda()))
    # (float32 u / 255 is not the double u / 255: a luma that sits on a .5 tie rounds the other way, so the uint8 frames score 5.2015, 5.2713
    # and their float32 copies 5.1968, 5.2696; the uint8 frames, host or device, are one input)
    assert torch.equal(metric(torch.from_numpy(clip_u8(192, 288)).permute(0, 3, 1, 2)), niqe.niqe(model, u8))
    assert torch.equal(metric(host[0]), got[:1])                                                            # a single [C,H,W] image


def test_score_vs_oracle():
    """The score at 192x288 against the oracle's, with a seeded synthetic pristine model.

    Tolerance, measured on the CPU and not guessed: the oracle's features of these two frames were perturbed by 1e-9 relative (RTOL, what
    the feature comparison admits) in 20 seeded draws, F * (1 + 1e-9 N(0,1)), numpy default_rng(100 + draw); the largest relative change
    of the oracle's score was 8.1e-9 (frame 0) and 1.06e-8 (frame 1); times 10 that is 1.06e-7, above the 1e-9 floor (six blocks per
    frame make a covariance of rank 5, whose small pooled directions magnify a feature's change).  The figure is kept
    in MEASURED below and recomputed here, so a change of inputs cannot leave it stale."""
    from dove_amd import niqe
    wf = reference(192, 288)[0]
    mu_p, cov_p = pristine_model(wf)
    want = np.array([R.score(mu_p, cov_p, F) for F in wf])
    worst = 0.0
    for d in range(20):
        rng = np.random.default_rng(100 + d)
        for i, F in enumerate(wf):
            worst = max(worst, abs(R.score(mu_p, cov_p, F * (1.0 + 1e-9 * rng.standard_normal(F.shape))) - want[i]) / want[i])
    tol = max(10 * worst, 1e-9)
    print(f"oracle scores {want}, largest relative change under 1e-9 feature noise {worst:.3e}, tolerance {tol:.3e}")
    assert MEASURED_SCORE_TOL / 2 <= tol <= MEASURED_SCORE_TOL * 2   # the recorded figure still describes these inputs
    got = niqe.niqe(niqe.NiqeModel(mu_p, cov_p), torch.from_numpy(clip_u8(192, 288)).cuda()).cpu().numpy()
    rel = np.abs(got - want) / want
    print(f"device scores {got}, relative difference {rel}")
    assert (rel <= MEASURED_SCORE_TOL).all()


MEASURED_SCORE_TOL = 1.06e-7


def fit_images():
    """Three seeded 192x192 images whose top-left block is much calmer than the rest, so the sharpness rule has something to drop."""
    out = []
    for i in range(3):
        img = R.make_image(40 + i, 192, 192).astype(np.float64)
        yy, xx = np.mgrid[0:96, 0:96]
        by, bx = (i % 2) * 96, (i // 2) * 96
        calm = 100.0 + (0.3 * xx + 0.2 * yy)[..., None] + 0.25 * (img[by:by + 96, bx:bx + 96] - 128.0)
        img[by:by + 96, bx:bx + 96] = calm
        out.append(np.clip(np.round(img), 0, 255).astype(np.uint8))
    return out


def test_fit_vs_oracle_and_direction():
    from dove_amd import niqe
    imgs = fit_images()
    wmu, wcov, wkept = R.fit(imgs, 0.75)
    assert [k.tolist() for k in wkept] == [[1, 2, 3], [0, 1, 3], [0, 2, 3]]     # the calm block of each image is dropped
    model = niqe.fit([torch.from_numpy(i)[None] for i in imgs], sharpness=0.75)
    for i, img in enumerate(imgs):                                # the same kept-block set: from the device's own sharpness
        s = niqe.features(torch.from_numpy(img)[None])[1].cpu().numpy()[0]
        assert np.nonzero(s > 0.75 * s.max())[0].tolist() == wkept[i].tolist()
    assert np.allclose(model.mu, wmu, rtol=RTOL, atol=0)
    scale = np.sqrt(np.outer(np.diag(wcov), np.diag(wcov)))       # covariances cancel: compared against the size of the variances
    assert (np.abs(model.cov - wcov) <= RTOL * scale).all()
    # direction only: a model fitted on a clip scores the clip lower than the clip after a strong Gaussian blur
    clip = torch.from_numpy(clip_u8(192, 288)).cuda()
    own = niqe.fit([clip], sharpness=0.0)
    x = clip.permute(0, 3, 1, 2).float()
    k = torch.exp(-torch.arange(-6, 7, dtype=torch.float32) ** 2 / (2 * 3.0 ** 2)).cuda()
    k = (k / k.sum())
    x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (6, 6, 0, 0), mode="replicate"), k.view(1, 1, 1, 13).repeat(3, 1, 1, 1), groups=3)
    x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (0, 0, 6, 6), mode="replicate"), k.view(1, 1, 13, 1).repeat(3, 1, 1, 1), groups=3)
    blurred = x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    a, b = niqe.niqe(own, clip), niqe.niqe(own, blurred)
    print(f"own clip {a.tolist()}, blurred {b.tolist()}")
    assert (a < b).all()


def test_determinism_and_batch_independence():
    from dove_amd import niqe
    frames = torch.from_numpy(clip_u8(200, 300, 3)).cuda()
    f1, s1 = niqe.features(frames)
    f2, s2 = niqe.features(frames)
    assert f1.cpu().numpy().tobytes() == f2.cpu().numpy().tobytes() and torch.equal(s1, s2)
    model = niqe.NiqeModel(*pristine_model(f1.cpu().numpy()))
    a, b = niqe.niqe(model, frames), niqe.niqe(model, frames)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for i in range(3):                                           # N = 1 and N = 3 give the same bits for the shared frame
        fi, si = niqe.features(frames[i:i + 1])
        assert fi.cpu().numpy().tobytes() == f1[i:i + 1].cpu().numpy().tobytes() and torch.equal(si, s1[i:i + 1])
        assert niqe.niqe(model, frames[i:i + 1]).cpu().numpy().tobytes() == a[i:i + 1].cpu().numpy().tobytes()


def test_eval_tool_without_and_with_gt(tmp_path):
    from dove_amd import eval_metrics, niqe
    pred, gt, wdir = tmp_path / "pred", tmp_path / "gt", tmp_path / "w"
    for d in (pred, gt, wdir):
        d.mkdir()
    clips = {"a": clip_u8(192, 288), "b": clip_u8(200, 300)}
    for name, c in clips.items():
        np.save(pred / f"{name}.npy", c)
        np.save(gt / f"{name}.npy", np.clip(c.astype(np.int16) + 3, 0, 255).astype(np.uint8))
    mu_p, cov_p = pristine_model(reference(192, 288)[0])
    niqe.NiqeModel(mu_p, cov_p).save(str(wdir / "niqe_synthetic.npz"))
    model = niqe.load_model(str(wdir))
    want = {n: round(float(niqe.niqe(model, torch.from_numpy(c)).mean()), 4) for n, c in clips.items()}
    out = eval_metrics.main(["--pred", str(pred), "--metrics", "niqe", "--metric_weights", str(wdir), "--crop", "4", "--test_y_channel"])
    with open(pred / "metrics_niqe.json") as f:
        js = json.load(f)
    assert js == out and js["count"] == 2 and js["per_sample"] == {n: {"niqe": v} for n, v in want.items()}
    out = eval_metrics.main(["--gt", str(gt), "--pred", str(pred), "--out", str(tmp_path), "--metrics", "psnr,niqe", "--metric_weights",
                             str(wdir), "--crop", "4"])
    assert os.path.exists(tmp_path / "metrics_psnr_niqe.json")
    for n in clips:                                              # --crop does not reach niqe: the same value as without ground truth
        assert out["per_sample"][n]["niqe"] == want[n] and 30.0 < out["per_sample"][n]["psnr"] < 45.0


def test_cli_eval_metrics_niqe_without_gt_dir(golden_dir, tmp_path, capsys):
    """The inference command line scores its own output without ground truth.  The clip is 5 x 48 x 48: the smallest whose x4 output
    (192 x 192) holds the two blocks a finite score needs (the 16 x 16 clip of the other command-line tests gives 64 x 64, below one block)."""
    from dove_amd import cli, niqe
    inp, out, wdir = tmp_path / "in", tmp_path / "out", tmp_path / "w"
    inp.mkdir()
    wdir.mkdir()
    np.save(inp / "clip0.npy", np.random.default_rng(5).integers(0, 256, size=(5, 48, 48, 3), dtype=np.uint8))
    mu_p, cov_p = pristine_model(reference(192, 288)[0])
    niqe.NiqeModel(mu_p, cov_p).save(str(wdir / "niqe_synthetic.npz"))
    emb = os.path.join(golden_dir, "empty_prompt_embedding.safetensors")
    cli.main(["--input_dir", str(inp), "--random_init", "--num_layers", "1", "--prompt_embedding", emb, "--output_path", str(out),
              "--eval_metrics", "niqe", "--metric_weights", str(wdir)])
    res = np.load(out / "clip0.npy")
    assert res.shape == (5, 192, 192, 3)
    with open(out / "metrics_niqe.json") as f:
        js = json.load(f)
    assert js["count"] == 1 and set(js["per_sample"]) == {"niqe"}
    want = float(niqe.niqe(niqe.load_model(str(wdir)), torch.from_numpy(res)).mean())
    assert np.isfinite(want) and js["per_sample"]["niqe"] == [want] and js["average"]["niqe"] == want
    assert "[clip0.npy] NIQE=" in capsys.readouterr().out
