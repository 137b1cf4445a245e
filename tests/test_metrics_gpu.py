"""GPU PSNR / SSIM (csrc/metrics.hip via dove_amd.metrics) against the float64 restatement in tests/fr_metrics_ref.py, plus the CLI's
--eval_metrics and python -m dove_amd.eval_metrics end to end."""
import json
import os
import time

import numpy as np
import pytest
import torch

import fr_metrics_ref as R

pytestmark = pytest.mark.gpu


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(pred_u8, gt_u8, crop=0, rgb_y=False):
    """[F,H,W,3] uint8 pair through clip-style views on the device -> per-frame values vs the restatement."""
    from dove_amd import metrics as M
    p, g = _gpu(pred_u8), _gpu(gt_u8)
    if crop:
        p, g = p[:, crop:-crop, crop:-crop], g[:, crop:-crop, crop:-crop]
        pred_u8, gt_u8 = pred_u8[:, crop:-crop, crop:-crop], gt_u8[:, crop:-crop, crop:-crop]
    ps, ss = M.fr_metrics(p, g, rgb_to_y=rgb_y)
    rp, rs = R.metrics(pred_u8.transpose(0, 3, 1, 2), gt_u8.transpose(0, 3, 1, 2), rgb_y)
    assert ps.dtype == torch.float64 and ps.shape == (len(pred_u8),)
    np.testing.assert_allclose(ps.cpu().numpy(), rp, rtol=0, atol=1e-6)
    np.testing.assert_allclose(ss.cpu().numpy(), rs, rtol=0, atol=1e-5)
    return ss.cpu().numpy()


@pytest.mark.parametrize("h,w", [(11, 11), (37, 53), (64, 96)])
@pytest.mark.parametrize("rgb_y", [False, True])
def test_u8_frames_vs_restatement(h, w, rgb_y):
    rng = np.random.default_rng(h * w + rgb_y)
    a = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    _check(a, b, rgb_y=rgb_y)
    base, noisy = R.structured_pair(rng, 2, h, w)
    _check(noisy, base, rgb_y=rgb_y)
    if h > 11:
        _check(noisy, base, crop=4, rgb_y=rgb_y)


def test_structured_ssim_range_and_full_hd_frame():
    rng = np.random.default_rng(3)
    lo = [R.structured_pair(rng, 1, 64, 96, noise=n) for n in (2, 60)]
    s = [_check(nz, base)[0] for base, nz in lo]
    assert s[0] > 0.9 and s[1] < 0.5, s                         # SSIM spans a wide range on these pairs
    base, noisy = R.structured_pair(rng, 1, 720, 1280, noise=8)
    _check(noisy, base)
    _check(noisy, base, crop=4, rgb_y=True)


def test_identical_inputs_exact():
    from dove_amd import metrics as M
    rng = np.random.default_rng(1)
    a = _gpu(rng.integers(0, 256, (3, 40, 70, 3), dtype=np.uint8))
    for rgb_y in (False, True):
        ps, ss = M.fr_metrics(a, a.clone(), rgb_to_y=rgb_y)
        assert torch.all(ss == 1.0), ss
        assert torch.all((ps - 80.0).abs() <= 1e-9), ps


def test_float_inputs_and_strided_views():
    from dove_amd import metrics as M
    rng = np.random.default_rng(2)
    F, H, W = 3, 45, 70
    u = rng.integers(0, 256, (2, 3, F, H, W), dtype=np.uint8)
    v32 = torch.from_numpy(u).cuda().float() / 255              # [2,3,F,H,W] like the decoder's clip
    pred, ref = v32[0:1], v32[1:2]
    pv, rv = pred[0].permute(1, 0, 2, 3), ref[0].permute(1, 0, 2, 3)   # [F,3,H,W] non-contiguous views
    assert not pv.is_contiguous()
    for dt in (torch.float32, torch.bfloat16):
        p, r = pv.to(dt), rv.to(dt)
        ps, ss = M.fr_metrics(p, r)
        rp, rs = R.metrics(p.float().cpu().numpy(), r.float().cpu().numpy())
        np.testing.assert_allclose(ps.cpu().numpy(), rp, rtol=0, atol=1e-6)
        np.testing.assert_allclose(ss.cpu().numpy(), rs, rtol=0, atol=1e-5)
        yp, _ = M.fr_metrics(p, r, ssim=False, rgb_to_y=True)
        np.testing.assert_allclose(yp.cpu().numpy(), R.metrics(p.float().cpu().numpy(), r.float().cpu().numpy(), True)[0], atol=1e-6)
    # the uint8 path ([F,H,W,3] frames) agrees with the float path on u/255 inputs
    fu = [torch.from_numpy(np.ascontiguousarray(u[i].transpose(1, 2, 3, 0))).cuda() for i in (0, 1)]
    pu, su = M.fr_metrics(fu[0], fu[1])
    pf, sf = M.fr_metrics(pv, rv)
    assert float((pu - pf).abs().max()) <= 1e-4 and float((su - sf).abs().max()) <= 1e-4
    # pyiqa's surface: create_metric(name).to(device).eval()(pred, ref) -> [N]
    for name, want in (("psnr", pf), ("ssim", sf)):
        m = M.create_metric(name).to("cuda").eval()
        got = m(pv, rv)
        assert got.shape == (F,) and torch.equal(got, want)


def test_one_channel_and_mixed_dtypes():
    """[N,1,H,W] uint8 (the one-channel luma and PSNR branches) and a uint8 prediction against a float32 / bfloat16 reference."""
    from dove_amd import metrics as M
    rng = np.random.default_rng(7)
    base, noisy = R.structured_pair(rng, 2, 37, 53)
    g1, p1 = base[..., :1].transpose(0, 3, 1, 2), noisy[..., 1:2].transpose(0, 3, 1, 2)      # [2,1,37,53] uint8 (non-contiguous)
    for crop in (0, 4):
        gc, pc = (g1, p1) if not crop else (g1[:, :, crop:-crop, crop:-crop], p1[:, :, crop:-crop, crop:-crop])
        ps, ss = M.fr_metrics(_gpu(pc), _gpu(gc))
        rp, rs = R.metrics(pc, gc)
        np.testing.assert_allclose(ps.cpu().numpy(), rp, rtol=0, atol=1e-6)
        np.testing.assert_allclose(ss.cpu().numpy(), rs, rtol=0, atol=1e-5)
    ps, ss = M.fr_metrics(torch.from_numpy(p1).cuda()[:, :, :, ::2], torch.from_numpy(g1).cuda()[:, :, :, ::2])   # strided W
    rp, rs = R.metrics(p1[:, :, :, ::2], g1[:, :, :, ::2])
    np.testing.assert_allclose(ps.cpu().numpy(), rp, atol=1e-6)
    np.testing.assert_allclose(ss.cpu().numpy(), rs, atol=1e-5)
    ref32 = torch.from_numpy(base.transpose(0, 3, 1, 2).copy()).cuda().float() / 255          # [2,3,H,W] float32
    for ref in (ref32, ref32.to(torch.bfloat16)):
        for rgb_y in (False, True):
            ps, ss = M.fr_metrics(_gpu(noisy), ref, rgb_to_y=rgb_y)                              # [F,H,W,3] uint8 vs [N,3,H,W] float
            rp, rs = R.metrics(noisy.transpose(0, 3, 1, 2), ref.float().cpu().numpy(), rgb_y)
            np.testing.assert_allclose(ps.cpu().numpy(), rp, rtol=0, atol=1e-6)
            np.testing.assert_allclose(ss.cpu().numpy(), rs, rtol=0, atol=1e-5)


def test_create_metric_takes_host_frames_like_the_reference():
    """inference_script.py compute_metrics (:91-107) calls model(pred, gt) with HOST [1,3,H,W] float32 frames after
    create_metric(name).to(device).eval(); pyiqa moves them to the metric's device.  Same here, also for a metric never moved."""
    import dove_amd.metrics as pyiqa
    rng = np.random.default_rng(8)
    base, noisy = R.structured_pair(rng, 3, 40, 56)
    pred = torch.from_numpy(noisy.transpose(0, 3, 1, 2).copy()).float() / 255                  # [F,3,H,W] on the host
    gt = torch.from_numpy(base.transpose(0, 3, 1, 2).copy()).float() / 255
    rp, rs = R.metrics(pred.numpy(), gt.numpy())
    models = {name: pyiqa.create_metric(name).to(torch.device("cuda")).eval() for name in ("psnr", "ssim")}
    for name, model in models.items():
        scores = [model(pred[i].unsqueeze(0), gt[i].unsqueeze(0)).item() for i in range(pred.shape[0])]
        want = rp if name == "psnr" else rs
        np.testing.assert_allclose(scores, want, rtol=0, atol=1e-6 if name == "psnr" else 1e-5)
    assert models["ssim"].device.type == "cuda"
    unmoved = pyiqa.create_metric("ssim")
    assert abs(unmoved(pred[:1], gt[:1]).item() - rs[0]) <= 1e-5


def test_deterministic_and_refusals():
    from dove_amd import metrics as M
    rng = np.random.default_rng(4)
    a = torch.from_numpy(rng.random((4, 3, 130, 200), dtype=np.float32)).cuda()
    b = (a + 0.05 * torch.randn_like(a)).clamp(0, 1)
    r1, r2 = M.fr_metrics(a, b), M.fr_metrics(a, b)
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))
    with pytest.raises(RuntimeError, match="SSIM needs H and W >= 11"):
        M.fr_metrics(a[:, :, :10], b[:, :, :10])
    ps, _ = M.fr_metrics(a[:, :, :10], b[:, :, :10], ssim=False)       # PSNR alone has no size limit
    assert ps.shape == (4,)
    with pytest.raises(ValueError, match="differ in shape"):
        M.fr_metrics(a, b[:, :, 1:])
    with pytest.raises(RuntimeError, match="channels must be 1 or 3"):
        M.fr_metrics(a[:, :2], b[:, :2])
    with pytest.raises(RuntimeError, match="rgb_to_y needs 3-channel"):
        M.fr_metrics(a[:, :1], b[:, :1], rgb_to_y=True)
    with pytest.raises(NotImplementedError, match="pyiqa"):
        M.clip_metrics(a, b, ["psnr", "lpips"])


def test_speed_33x720x1280_pair():
    """PSNR + SSIM of two 33x720x1280 uint8 clips: median of 10 calls after warm-up, bracketed by synchronisations."""
    from dove_amd import metrics as M
    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.randint(0, 256, (33, 720, 1280, 3), dtype=torch.uint8, device="cuda", generator=g)
    b = (a.int() + torch.randint(-8, 9, a.shape, device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
    for _ in range(3):
        M.fr_metrics(a, b)
    times = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M.fr_metrics(a, b)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    ms = float(np.median(times)) * 1e3
    ceiling_ms = 2 * a.numel() / 6.29e12 * 1e3                   # both clips read once at the measured copy rate
    print(f"[fr_metrics] PSNR+SSIM 33x720x1280 uint8 pair: {ms:.3f} ms per call (median of 10); copy-ceiling {ceiling_ms:.3f} ms "
          f"= {ceiling_ms / ms:.2f} of it")
    assert ms <= 2.0, ms


def test_cli_eval_metrics_psnr_ssim(golden_dir, tmp_path, capsys):
    from dove_amd import cli
    from dove_amd import metrics as M
    inp, out, gtd = tmp_path / "in", tmp_path / "out", tmp_path / "gt"
    inp.mkdir()
    gtd.mkdir()
    rng = np.random.default_rng(5)
    np.save(inp / "clip0.npy", rng.integers(0, 256, size=(5, 16, 16, 3), dtype=np.uint8))
    gt = rng.integers(0, 256, size=(5, 64, 64, 3), dtype=np.uint8)
    np.save(gtd / "clip0.npy", gt)
    emb = os.path.join(golden_dir, "empty_prompt_embedding.safetensors")
    cli.main(["--input_dir", str(inp), "--random_init", "--num_layers", "1", "--prompt_embedding", emb, "--output_path", str(out),
              "--gt_dir", str(gtd), "--eval_metrics", "psnr,ssim"])
    printed = capsys.readouterr().out
    res = np.load(out / "clip0.npy")
    with open(out / "metrics_psnr_ssim.json") as f:
        js = json.load(f)
    assert set(js) == {"per_sample", "average", "count"} and js["count"] == 1
    want = M.clip_metrics(torch.from_numpy(res), torch.from_numpy(gt), ["psnr", "ssim"])
    for m in ("psnr", "ssim"):
        assert js["per_sample"][m] == [want[m]] and js["average"][m] == want[m]
    # the former CPU formula (10 log10(1 / (mse + 1e-8)) per frame, mean over frames)
    mse = ((res.astype(np.float64) / 255 - gt.astype(np.float64) / 255) ** 2).reshape(len(res), -1).mean(1)
    cpu = float((10 * np.log10(1.0 / (mse + 1e-8))).mean())
    line = [ln for ln in printed.splitlines() if ln.startswith("[clip0.npy] PSNR=")][0]
    assert abs(float(line.split("=")[1]) - cpu) <= 1e-4
    assert f"=== Overall Average SSIM: {want['ssim']:.4f} ===" in printed and "=== Overall Average PSNR: " in printed
    # the former combination: --eval_metrics psnr with --eval_psnr_dir and no --gt_dir keeps its CPU PSNR, printed once
    out2 = tmp_path / "out2"
    cli.main(["--input_dir", str(inp), "--random_init", "--num_layers", "1", "--prompt_embedding", emb, "--output_path", str(out2),
              "--eval_psnr_dir", str(gtd), "--eval_metrics", "psnr"])
    printed = capsys.readouterr().out
    assert printed.count("=== Overall Average PSNR: ") == 1 and printed.count("[clip0.npy] PSNR=") == 1
    res2 = np.load(out2 / "clip0.npy")
    mse2 = ((res2.astype(np.float64) / 255 - gt.astype(np.float64) / 255) ** 2).reshape(len(res2), -1).mean(1)
    with open(out2 / "metrics_psnr.json") as f:
        js2 = json.load(f)
    assert abs(js2["per_sample"]["psnr"][0] - float((10 * np.log10(1.0 / (mse2 + 1e-8))).mean())) <= 1e-4


def test_eval_metrics_tool_mismatch_crop_y_center(tmp_path):
    from PIL import Image

    from dove_amd import eval_metrics
    gtd, prd, outd = tmp_path / "gt", tmp_path / "pred", tmp_path / "res"
    gtd.mkdir()
    prd.mkdir()
    rng = np.random.default_rng(6)
    base, noisy = R.structured_pair(rng, 4, 48, 60)
    clips = {"a": (base, noisy[:3, 3:45, 1:58])}                 # pred has fewer frames and a smaller H x W
    g2, p2 = R.structured_pair(rng, 2, 30, 40, noise=40)
    clips["b"] = (g2, p2)
    np.save(gtd / "a.npy", clips["a"][0])
    np.save(prd / "a.npy", np.ascontiguousarray(clips["a"][1]))
    for d, arr in ((gtd / "b", g2), (prd / "b", p2)):                # PNG folders
        d.mkdir()
        for i, fr in enumerate(arr):
            Image.fromarray(fr).save(d / f"{i:03d}.png")
    np.save(prd / "c.npy", p2)                                       # no GT: skipped
    out = eval_metrics.main(["--gt", str(gtd), "--pred", str(prd), "--out", str(outd), "--crop", "2", "--test_y_channel",
                             "--is_center"])
    with open(outd / "metrics_psnr_ssim.json") as f:
        js = json.load(f)
    assert js == json.loads(json.dumps(out)) and js["count"] == 2 and set(js["per_sample"]) == {"a", "b"}
    for name, (g, p) in clips.items():
        want = R.clip_values(p, g, crop=2, test_y_channel=True, is_center=True)
        for m in ("psnr", "ssim"):
            assert abs(js["per_sample"][name][m] - round(want[m], 4)) <= 1e-4 + 1e-12, (name, m)
    for m in ("psnr", "ssim"):
        assert js["average"][m] == round(float(np.mean([js["per_sample"][n][m] for n in ("a", "b")])), 4)
