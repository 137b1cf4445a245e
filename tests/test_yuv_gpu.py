"""GPU side of the Y4M video I/O: dove_rgb_to_yuv_u8 and dove_yuv_to_rgb_u8 (csrc/yuv.hip) equal tests/yuv_ref.py bit for bit."""
import numpy as np
import pytest
import torch

import yuv_ref as R

pytestmark = pytest.mark.gpu

MATRICES = ("bt601", "bt709")
RANGES = ("limited", "full")
SIZES = [(2, 2, 2), (3, 5, 7), (2, 6, 9), (2, 7, 16), (1, 1, 1), (2, 16, 24), (1, 33, 40)]      # (F, H, W): odd, tiny, vector widths


def _fmt(chroma, matrix, rng, siting="centre"):
    from dove_amd import yuv
    return yuv.YuvFormat(chroma, matrix, rng, siting)


def _frames(F, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)


def _video(F, H, W, seed, dtype):
    """[3,F,H,W] in about [-0.1, 1.1] with exact k/255 and out-of-range values mixed in."""
    g = np.random.default_rng(seed)
    v = g.random((3, F, H, W), dtype=np.float32) * 1.2 - 0.1
    k = g.integers(0, 256, size=v.shape).astype(np.float32) / np.float32(255)
    v = np.where(g.random(v.shape) < 0.3, k, v)
    flat = v.reshape(-1)
    flat[:6] = [-1.0, 0.0, 1.0, 2.0, 1.0 / 255, 254.0 / 255][:flat.size]
    t = torch.from_numpy(v).to(dtype)
    return t, t.float().numpy()


@pytest.mark.parametrize("chroma", ("444", "422", "420", "mono"))
@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_rgb_to_yuv_from_u8_frames_is_bit_exact(matrix, rng, chroma):
    from dove_amd import yuv
    for F, H, W in SIZES:
        rgb = _frames(F, H, W, F * 1000 + H * 31 + W)
        got = yuv.rgb_to_yuv(torch.from_numpy(rgb).cuda(), _fmt(chroma, matrix, rng))
        want = R.rgb_to_yuv(rgb, matrix, rng, chroma)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), (F, H, W)


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32))
@pytest.mark.parametrize("chroma", ("444", "422", "420"))
def test_rgb_to_yuv_fused_float_route_is_bit_exact(chroma, dtype):
    """[3,F,H,W] float input: equal to the definition on the quantised frames, to postprocess_u8 followed by the u8 route, and across
    two calls."""
    from dove_amd import ops, yuv
    for matrix, rng in (("bt601", "limited"), ("bt709", "full"), ("bt601", "full"), ("bt709", "limited")):
        for F, H, W in SIZES:
            t, host = _video(F, H, W, H * 100 + W, dtype)
            dev = t.cuda()
            fmt = _fmt(chroma, matrix, rng)
            got = yuv.rgb_to_yuv(dev, fmt)
            q = R.quantise(host).transpose(1, 2, 3, 0)                             # [F,H,W,3]
            assert np.array_equal(got.cpu().numpy(), R.rgb_to_yuv(np.ascontiguousarray(q), matrix, rng, chroma)), (F, H, W)
            frames = ops.postprocess_u8(dev, F, H, W)
            assert np.array_equal(frames.cpu().numpy(), q)
            assert torch.equal(yuv.rgb_to_yuv(frames, fmt), got)
            assert torch.equal(yuv.rgb_to_yuv(dev, fmt), got)
            assert torch.equal(yuv.rgb_to_yuv(dev[None], fmt), got)


@pytest.mark.parametrize("chroma", ("444", "422", "420"))
def test_rgb_to_yuv_through_a_cropped_view(chroma):
    """The crop that removes the padding is a pointer offset and smaller extents: nothing is copied, and rows start unaligned."""
    from dove_amd import yuv
    t, host = _video(5, 37, 52, 11, torch.bfloat16)
    dev = t.cuda()
    for (Fo, Ho, Wo) in ((4, 33, 45), (5, 32, 48), (3, 37, 40)):
        got = yuv.rgb_to_yuv(dev, _fmt(chroma, "bt601", "limited"), crop=(Fo, Ho, Wo))
        q = np.ascontiguousarray(R.quantise(host)[:, :Fo, :Ho, :Wo].transpose(1, 2, 3, 0))
        assert np.array_equal(got.cpu().numpy(), R.rgb_to_yuv(q, "bt601", "limited", chroma)), (Fo, Ho, Wo)
    sub = dev[:, 1:4, 3:30, 5:46]                                                  # an interior window: every row starts odd
    got = yuv.rgb_to_yuv(sub, _fmt(chroma, "bt709", "full"))
    q = np.ascontiguousarray(R.quantise(host)[:, 1:4, 3:30, 5:46].transpose(1, 2, 3, 0))
    assert np.array_equal(got.cpu().numpy(), R.rgb_to_yuv(q, "bt709", "full", chroma))
    u8 = torch.from_numpy(_frames(4, 21, 30, 5)).cuda()
    got = yuv.rgb_to_yuv(u8, _fmt(chroma, "bt601", "full"), crop=(3, 19, 27))
    assert np.array_equal(got.cpu().numpy(), R.rgb_to_yuv(np.ascontiguousarray(u8.cpu().numpy()[:3, :19, :27]), "bt601", "full", chroma))
    with pytest.raises(ValueError, match="does not fit"):
        yuv.rgb_to_yuv(u8, _fmt(chroma, "bt601", "full"), crop=(5, 19, 27))


@pytest.mark.parametrize("chroma", ("444", "420"))
def test_rgb_to_yuv_at_the_clip_size_33x720x1280(chroma):
    from dove_amd import yuv
    g = torch.Generator(device="cuda").manual_seed(1)
    dev = (torch.rand(3, 33, 720, 1280, generator=g, device="cuda") * 1.1 - 0.05).to(torch.bfloat16)
    fmt = _fmt(chroma, "bt601", "limited")
    got = yuv.rgb_to_yuv(dev, fmt)
    assert tuple(got.shape) == (33, R.frame_bytes(720, 1280, chroma))
    assert torch.equal(yuv.rgb_to_yuv(dev, fmt), got)
    host = dev[:, 30:].float().cpu().numpy()                                       # the definition on the last three frames
    q = np.ascontiguousarray(R.quantise(host).transpose(1, 2, 3, 0))
    assert np.array_equal(got[30:].cpu().numpy(), R.rgb_to_yuv(q, "bt601", "limited", chroma))
    q0 = np.ascontiguousarray(R.quantise(dev[:, :1].float().cpu().numpy()).transpose(1, 2, 3, 0))
    assert np.array_equal(got[:1].cpu().numpy(), R.rgb_to_yuv(q0, "bt601", "limited", chroma))


@pytest.mark.parametrize("tag", sorted(R.TAGS))
@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_yuv_to_rgb_is_bit_exact(matrix, rng, tag):
    from dove_amd import y4m, yuv
    chroma, siting = R.TAGS[tag]
    assert y4m.COLOURSPACES[tag] == (chroma, siting)
    for F, H, W in SIZES + [(2, 720, 1280)]:
        payload = np.random.default_rng(H * 7 + W).integers(0, 256, size=(F, R.frame_bytes(H, W, chroma)), dtype=np.uint8)
        got = yuv.yuv_to_rgb(torch.from_numpy(payload).cuda(), H, W, _fmt(chroma, matrix, rng, siting))
        assert tuple(got.shape) == (F, H, W, 3) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), R.yuv_to_rgb(payload, H, W, matrix, rng, chroma, siting)), (F, H, W)


def test_yuv_to_rgb_feeds_preprocess_unchanged():
    from dove_amd import ops, prepost, yuv
    F, H, W = 5, 30, 45
    payload = np.random.default_rng(2).integers(0, 256, size=(F, R.frame_bytes(H, W, "420")), dtype=np.uint8)
    rgb = yuv.yuv_to_rgb(torch.from_numpy(payload).cuda(), H, W, _fmt("420", "bt601", "limited", "left"))
    want_rgb = R.yuv_to_rgb(payload, H, W, "bt601", "limited", "420", "left")
    video, pad_f, pad_h, pad_w, _ = prepost.preprocess_frames(torch.from_numpy(want_rgb), 4)
    assert torch.equal(ops.preprocess_u8(rgb, pad_f, pad_h, pad_w, 4, torch.bfloat16)[None], video)


def test_load_frames_reads_y4m(tmp_path):
    from dove_amd import prepost, y4m
    H, W = 18, 26
    payload = np.random.default_rng(4).integers(0, 256, size=(70, R.frame_bytes(H, W, "422")), dtype=np.uint8)   # more than one block
    path = str(tmp_path / "clip.y4m")
    with y4m.Y4MWriter(path, W, H, 25, "422", True) as wr:
        wr.write(payload)
    got = prepost.load_frames(path, yuv_matrix="bt709")
    assert not got.is_cuda and np.array_equal(got.numpy(), R.yuv_to_rgb(payload, H, W, "bt709", "full", "422", "left"))
    got = prepost.load_frames(path, yuv_range="limited")                           # the flag overrides the stream's tag
    assert np.array_equal(got.numpy(), R.yuv_to_rgb(payload, H, W, "bt601", "limited", "422", "left"))
