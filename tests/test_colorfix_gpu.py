"""GPU colour fix (csrc/colorfix.hip via dove_amd.colorfix) against the float64 restatement in tests/colorfix_ref.py and the reference's
recorded fp32 outputs (tests/golden/colorfix_golden.npz), plus prepost.postprocess_frames, the CLI's --color_fix, the standalone tool
and the bare C call.

Bounds.  Float gate on the golden cases: max |kernel - restatement| <= 2 * e_ref, e_ref = the reference's own fp32 distance from the
restatement on that case and mode (taken from the fixture here); the factor 2 allows for another summation order.  For sizes without a
recorded reference output the bound is 2 * the SMALLEST e_ref of that mode over the golden cases.  uint8 gate: no pixel off by more than
one level against trunc(clamp(restatement) * 255) and at most 1e-3 of the pixels off at all (truncation ties only)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import colorfix_ref as R

pytestmark = pytest.mark.gpu

CASES = ("a", "b", "c")
MODES = ("wavelet", "adain")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "colorfix_golden.npz"))


def _e_ref(golden, case, mode):
    want = R.fix(golden[f"{case}_content"], golden[f"{case}_style"], mode)
    return float(np.abs(golden[f"{case}_{mode}"].astype(np.float64) - want).max()), want


def _bound(golden, mode):
    return 2.0 * min(_e_ref(golden, k, mode)[0] for k in CASES)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f32(content, style, mode, **kw):
    from dove_amd import colorfix
    return colorfix.color_fix(content, style, mode, out_dtype=torch.float32, clamp=False, **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_float_gate_against_reference_error(golden, case, mode):
    from dove_amd import colorfix
    c, s = golden[f"{case}_content"], golden[f"{case}_style"]
    e_ref, want = _e_ref(golden, case, mode)
    fn = colorfix.wavelet_reconstruction if mode == "wavelet" else colorfix.adaptive_instance_normalization
    got = fn(torch.from_numpy(c), torch.from_numpy(s))           # host tensors, the reference's call
    assert got.dtype == torch.float32 and got.shape == c.shape and got.device.type == "cpu"
    err = float(np.abs(got.numpy().astype(np.float64) - want).max())
    print(f"[colorfix] case {case} {tuple(c.shape)} {mode}: kernel error {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}")
    assert err <= 2.0 * e_ref, (err, e_ref)
    # the same values handed over as bfloat16 (they are exact in it): the same bits
    got16 = _f32(_gpu(c).bfloat16(), _gpu(s).bfloat16(), mode)
    assert torch.equal(got16.cpu(), got)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_uint8_gate(golden, case, mode):
    from dove_amd import colorfix
    c, s = golden[f"{case}_content"], golden[f"{case}_style"]
    frames = colorfix.color_fix(_gpu(c), _gpu(s), mode, out_dtype=torch.uint8)
    assert frames.shape == (c.shape[0], c.shape[2], c.shape[3], 3) and frames.dtype == torch.uint8
    worst, share = R.u8_gate(frames.permute(0, 3, 1, 2).cpu().numpy(), R.to_u8(R.fix(c, s, mode)))
    print(f"[colorfix] case {case} {mode} uint8: worst {worst} level(s), share off {share:.2e}")
    assert worst <= 1 and share <= 1e-3
    # uint8 out is the truncation of the clamped fp32 out, and the clamped out is the clamp of the unclamped one
    f = colorfix.color_fix(_gpu(c), _gpu(s), mode, out_dtype=torch.float32, clamp=True)
    assert torch.equal(f, _f32(_gpu(c), _gpu(s), mode).clamp(0, 1))
    assert torch.equal((f * 255.0).to(torch.uint8), frames.permute(0, 3, 1, 2))
    b = colorfix.color_fix(_gpu(c), _gpu(s), mode, out_dtype=torch.bfloat16, clamp=True)
    assert torch.equal(b, f.bfloat16())


@pytest.mark.parametrize("mode", MODES)
def test_views_give_identical_bits(golden, mode):
    c, s = _gpu(golden["a_content"]), _gpu(golden["a_style"])     # [2,3,45,37] float32, exact in bf16
    plain = _f32(c, s, mode)
    assert torch.equal(plain, _f32(c, s, mode))                    # two calls: identical bits
    # [3,F,H,W] bf16 clips through permute
    c3, s3 = c.permute(1, 0, 2, 3).contiguous().bfloat16(), s.permute(1, 0, 2, 3).contiguous().bfloat16()
    cv, sv = c3.permute(1, 0, 2, 3), s3.permute(1, 0, 2, 3)
    assert not cv.is_contiguous()
    assert torch.equal(_f32(cv, sv, mode), plain)
    # crops of larger padded tensors (other strides, a pointer offset)
    g = torch.Generator(device="cuda").manual_seed(1)
    big_c = torch.rand(2, 3, 45 + 7, 37 + 9, device="cuda", generator=g)
    big_s = torch.rand(2, 3, 45 + 11, 37 + 6, device="cuda", generator=g).bfloat16()
    big_c[:, :, 3:48, 5:42] = c
    big_s[:, :, 8:53, 1:38] = s.bfloat16()
    assert torch.equal(_f32(big_c[:, :, 3:48, 5:42], big_s[:, :, 8:53, 1:38], mode), plain)
    # style in [-1,1] read as 0.5 x + 0.5: x = 2 s - 1 and s' = 0.5 x + 0.5, both in fp32 on the host
    x = (2.0 * s.cpu() - 1.0)
    s_back = (0.5 * x + 0.5)
    assert torch.equal(_f32(c, x.cuda(), mode, style_affine=(0.5, 0.5)), _f32(c, s_back.cuda(), mode))
    # [F,H,W,3] uint8 frames: read as u / 255 in fp32
    cu = (c * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    su = (s * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    cf, sf = (cu.cpu().float() / 255.0).permute(0, 3, 1, 2).contiguous().cuda(), (su.cpu().float() / 255.0).permute(0, 3, 1, 2).contiguous().cuda()
    from_u8 = _f32(cu, su, mode).float()
    assert torch.equal(from_u8, _f32(cf, sf, mode))
    assert torch.equal(_f32(cu.permute(0, 3, 1, 2).contiguous(), su.permute(0, 3, 1, 2), mode).float(), from_u8)
    # mixed: uint8 content frames against a float style
    assert torch.equal(_f32(cu, sf, mode).float(), from_u8)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 50), (17, 16), (64, 64), (65, 129), (2, 1), (130, 3)])
def test_sizes_against_restatement(golden, h, w):
    from dove_amd import colorfix
    rng = np.random.default_rng(h * 1000 + w)
    c, s = R.make_pair(rng, 2, h, w)
    got = _f32(_gpu(c), _gpu(s), "wavelet").cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - R.wavelet(c, s)).max())
    print(f"[colorfix] {h}x{w} wavelet: error {err:.3e} (bound {_bound(golden, 'wavelet'):.3e})")
    assert err <= _bound(golden, "wavelet")
    if h * w == 1:
        assert np.array_equal(got, c + (s - c))                   # every tap is the pixel itself: content + (style - content) in fp32
        with pytest.raises(RuntimeError, match="at least 2 pixels"):
            colorfix.adaptive_instance_normalization(_gpu(c), _gpu(s))
        return
    got = _f32(_gpu(c), _gpu(s), "adain").cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - R.adain(c, s)).max())
    print(f"[colorfix] {h}x{w} adain: error {err:.3e} (bound {_bound(golden, 'adain'):.3e})")
    assert err <= _bound(golden, "adain")


def test_full_frame_720x1280(golden):
    from dove_amd import colorfix
    rng = np.random.default_rng(9)
    c, s = R.make_pair(rng, 1, 720, 1280)
    cg, sg = _gpu(c).bfloat16(), _gpu(s).bfloat16()
    for mode in MODES:
        want = R.fix(c, s, mode)
        got = _f32(cg, sg, mode)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print(f"[colorfix] 720x1280 {mode}: error {err:.3e} (bound {_bound(golden, mode):.3e})")
        assert err <= _bound(golden, mode)
        assert torch.equal(got, _f32(cg, sg, mode))
        frames = colorfix.color_fix(cg, sg, mode, out_dtype=torch.uint8)
        worst, share = R.u8_gate(frames.permute(0, 3, 1, 2).cpu().numpy(), R.to_u8(want))
        print(f"[colorfix] 720x1280 {mode} uint8: worst {worst}, share off {share:.2e}")
        assert worst <= 1 and share <= 1e-3


def test_identity_offset_and_refusals():
    from dove_amd import colorfix
    rng = np.random.default_rng(11)
    c, _ = R.make_pair(rng, 1, 40, 52)
    c = 0.2 + 0.5 * c
    cg = _gpu(c.astype(np.float32))
    for mode in MODES:
        same = _f32(cg, cg.clone(), mode)
        assert float((same - cg).abs().max()) <= (0.0 if mode == "wavelet" else 1.2e-7)      # wavelet: low5(0) = 0 exactly
        off = _f32(cg, cg + 0.125, mode)
        assert float((off - (cg + 0.125)).abs().max()) <= 2.4e-7
    with pytest.raises(ValueError, match="differ in shape"):
        colorfix.color_fix(cg, cg[:, :, 1:], "wavelet")
    with pytest.raises(ValueError, match=r"must be \[N,3,H,W\]"):
        colorfix.color_fix(cg[:, :2], cg[:, :2], "wavelet")
    with pytest.raises(TypeError, match="float32 / bfloat16 / uint8"):
        colorfix.color_fix(cg.half(), cg.half(), "adain")


def test_postprocess_frames_color_fix():
    from dove_amd import colorfix, prepost
    g = torch.Generator(device="cuda").manual_seed(3)
    video = torch.rand(1, 3, 6, 40, 56, device="cuda", generator=g).bfloat16()
    source = (torch.rand(1, 3, 6, 40, 56, device="cuda", generator=g) * 2 - 1).bfloat16()
    pad_f, pad_h, pad_w = 1, 1, 2
    base = prepost.postprocess_frames(video, pad_f, pad_h, pad_w)
    assert torch.equal(prepost.postprocess_frames(video, pad_f, pad_h, pad_w, color_fix=None), base)
    assert torch.equal(prepost.postprocess_frames(video, pad_f, pad_h, pad_w, color_fix=None, source=source), base)
    assert base.shape == (5, 36, 48, 3)
    for mode in MODES:
        got = prepost.postprocess_frames(video, pad_f, pad_h, pad_w, color_fix=mode, source=source)
        # by hand: crop, copy, map the source to [0,1], fix, clamp, truncate
        c = video[0, :, :5, :36, :48].permute(1, 0, 2, 3).contiguous().float()
        s = (0.5 * source[0, :, :5, :36, :48].permute(1, 0, 2, 3).contiguous().float() + 0.5)
        fixed = colorfix.color_fix(c, s, mode, out_dtype=torch.float32, clamp=True)
        want = (fixed * 255.0).to(torch.uint8).permute(0, 2, 3, 1)
        assert got.shape == base.shape and got.dtype == torch.uint8 and got.is_contiguous()
        assert torch.equal(got, want)
        assert not torch.equal(got, base)


def test_c_call_from_ctypes_alone(golden):
    """dove_color_fix with views built by hand: [3,F,H,W] bf16 content, a [-1,1] fp32 style crop, [F,H,W,3] uint8 out."""
    from dove_amd import colorfix
    from dove_amd import lib as L
    lib = L.load()
    c, s = _gpu(golden["c_content"]), _gpu(golden["c_style"])     # [1,3,72,104]
    N, _, H, W = c.shape
    clip = c.permute(1, 0, 2, 3).contiguous().bfloat16()          # [3,N,H,W]
    pad = torch.zeros(N, 3, H + 4, W + 8, device="cuda")
    pad[:, :, 2:2 + H, 3:3 + W] = 2.0 * s - 1.0
    for mode, code in (("wavelet", L.COLORFIX_WAVELET), ("adain", L.COLORFIX_ADAIN)):
        out = torch.zeros(N, H, W, 3, dtype=torch.uint8, device="cuda")
        cv, sv, ov = L.ImageView(), L.ImageView(), L.ImageView()
        cv.data, cv.dtype, cv.sn, cv.sc, cv.sh, cv.sw = clip.data_ptr(), L.BF16, H * W, N * H * W, W, 1
        sv.data, sv.dtype = pad.data_ptr() + 4 * (2 * (W + 8) + 3), L.F32
        sv.sn, sv.sc, sv.sh, sv.sw = 3 * (H + 4) * (W + 8), (H + 4) * (W + 8), W + 8, 1
        ov.data, ov.dtype, ov.sn, ov.sc, ov.sh, ov.sw = out.data_ptr(), L.U8, H * W * 3, 1, W * 3, 3
        nbytes = int(lib.dove_color_fix_workspace_bytes(code, N, H, W))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        rc = lib.dove_color_fix(C.byref(cv), 1.0, 0.0, C.byref(sv), 0.5, 0.5, N, H, W, code, L.COLORFIX_CLAMP, C.byref(ov),
                                C.c_void_p(ws.data_ptr()), nbytes, L.stream_ptr())
        assert rc == 0, lib.dove_last_error()
        torch.cuda.synchronize()
        want = colorfix.color_fix(clip.permute(1, 0, 2, 3), pad[:, :, 2:2 + H, 3:3 + W], mode, out_dtype=torch.uint8,
                                  style_affine=(0.5, 0.5))
        assert torch.equal(out, want)
        # in place: out is the very view given as content
        buf = c.clone()
        bv = L.ImageView()
        bv.data, bv.dtype, bv.sn, bv.sc, bv.sh, bv.sw = buf.data_ptr(), L.F32, 3 * H * W, H * W, W, 1
        rc = lib.dove_color_fix(C.byref(bv), 1.0, 0.0, C.byref(sv), 0.5, 0.5, N, H, W, code, 0, C.byref(bv),
                                C.c_void_p(ws.data_ptr()), nbytes, L.stream_ptr())
        assert rc == 0, lib.dove_last_error()
        assert torch.equal(buf, _f32(c, pad[:, :, 2:2 + H, 3:3 + W], mode, style_affine=(0.5, 0.5)))


def test_cli_color_fix_end_to_end(golden_dir, tmp_path, capsys, monkeypatch):
    from dove_amd import cli, colorfix, prepost
    inp = tmp_path / "in"
    inp.mkdir()
    rng = np.random.default_rng(5)
    np.save(inp / "clip0.npy", rng.integers(0, 256, size=(5, 16, 16, 3), dtype=np.uint8))
    emb = os.path.join(golden_dir, "empty_prompt_embedding.safetensors")
    seen = {}
    real = prepost.postprocess_frames

    def spy(video, *a, **k):                                      # keeps the run's `out` and `video` for the by-hand fix
        seen["out"], seen["source"], seen["pads"] = video.clone(), k.get("source"), a
        return real(video, *a, **k)

    monkeypatch.setattr(prepost, "postprocess_frames", spy)

    def run(tag, *extra):
        out = tmp_path / tag
        cli.main(["--input_dir", str(inp), "--random_init", "--num_layers", "1", "--prompt_embedding", emb, "--output_path", str(out),
                  *extra])
        return np.load(out / "clip0.npy"), capsys.readouterr().out

    plain, text_plain = run("plain")
    none, text_none = run("none", "--color_fix", "none")
    assert plain.tobytes() == none.tobytes() and seen["source"] is None
    assert "--color_fix" not in text_plain and "--color_fix" not in text_none
    fixed, text = run("wavelet", "--color_fix", "wavelet")
    assert text.count("--color_fix wavelet") == 1                 # printed once per run
    assert fixed.shape == plain.shape == (5, 64, 64, 3) and not np.array_equal(fixed, plain)
    pad_f, pad_h, pad_w = seen["pads"][:3]
    F, H, W = seen["out"].shape[2] - pad_f, seen["out"].shape[3] - 4 * pad_h, seen["out"].shape[4] - 4 * pad_w
    assert (F, H, W) == (5, 64, 64)
    c = seen["out"][0, :, :F, :H, :W].permute(1, 0, 2, 3)
    s = seen["source"][0, :, :F, :H, :W].permute(1, 0, 2, 3)
    by_hand = colorfix.color_fix(c, s, "wavelet", out_dtype=torch.float32, clamp=False, style_affine=(0.5, 0.5))
    want = (by_hand.clamp(0, 1) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(fixed, want)
    # what the fix is for: the result's low band is the source's.  Per frame and channel, mean(low5(result) - low5(source)) ~ 0
    src01 = (0.5 * s.float() + 0.5).cpu().numpy()
    d = (R.low5(by_hand.cpu().numpy()) - R.low5(src01)).mean(axis=(2, 3))
    before = (R.low5(c.float().cpu().numpy()) - R.low5(src01)).mean(axis=(2, 3))
    print(f"[colorfix] cli: |mean low5(result) - low5(source)| max {np.abs(d).max():.2e} (before the fix {np.abs(before).max():.2e})")
    assert np.abs(d).max() <= 1.0 / 255.0
    # the scored frames are the fixed ones
    gtd = tmp_path / "gt"
    gtd.mkdir()
    np.save(gtd / "clip0.npy", fixed)
    _, text = run("scored", "--color_fix", "wavelet", "--gt_dir", str(gtd), "--eval_metrics", "psnr")
    assert "[clip0.npy] PSNR=80.0000" in text


def test_tool_on_disk_results(tmp_path, capsys):
    from PIL import Image

    from dove_amd import colorfix, ops
    rng = np.random.default_rng(12)
    c, s = R.make_pair(rng, 3, 48, 64)
    cu, su = (np.ascontiguousarray(R.to_u8(x).transpose(0, 2, 3, 1)) for x in (c, s))
    small = np.ascontiguousarray(su[:, ::4, ::4])                  # a source 4 times smaller: upscaled by the bilinear kernel
    pred, src, out = tmp_path / "pred", tmp_path / "src", tmp_path / "out"
    for d in (pred, src, pred / "b", src / "b"):
        d.mkdir()
    np.save(pred / "a.npy", cu)
    np.save(src / "a.npy", su)
    for i in range(3):
        Image.fromarray(cu[i]).save(pred / "b" / f"{i:03d}.png")
        Image.fromarray(small[i]).save(src / "b" / f"{i:03d}.png")
    np.save(pred / "c.npy", cu)
    np.save(src / "c.npy", np.ascontiguousarray(su[:, :40]))         # neither the same size nor an integer factor: skipped
    np.save(pred / "d.npy", cu)                                      # no source: skipped
    done = colorfix.main(["--pred", str(pred), "--source", str(src), "--out", str(out), "--mode", "adain"])
    text = capsys.readouterr().out
    assert done == ["a", "b"] and "Skipping c:" in text and "Skipping d: no matching source file." in text
    got_a = np.load(out / "a.npy")
    worst, share = R.u8_gate(got_a.transpose(0, 3, 1, 2), R.to_u8(R.adain(cu.transpose(0, 3, 1, 2) / 255.0, su.transpose(0, 3, 1, 2) / 255.0)))
    assert worst <= 1 and share <= 1e-3
    got_b = np.stack([np.asarray(Image.open(out / "b" / f"{i:03d}.png")) for i in range(3)])
    up = ops.preprocess_u8(_gpu(small), 0, 0, 0, 4, torch.float32).permute(1, 0, 2, 3)
    want_b = colorfix.color_fix(_gpu(cu), up, "adain", out_dtype=torch.uint8, style_affine=(0.5, 0.5))
    assert np.array_equal(got_b, want_b.cpu().numpy())
