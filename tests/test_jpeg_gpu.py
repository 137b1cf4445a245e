"""GPU JPEG encoder (csrc/jpeg.hip, dove_amd/jpeg.py, dove_amd/avi.py): every file is byte-identical to tests/jpeg_ref.py's definition,
does not depend on batch, call or view, stays inside dove_jpeg_bound, and decodes in Pillow to within jpeg_ref.PILLOW_BOUND of the
library's own decode of the same levels."""
import io
import os

import numpy as np
import pytest
import torch

import jpeg_ref as J
from test_jpeg_cpu import check_avi

pytestmark = pytest.mark.gpu

SUBS = ("420", "444")
QUALITIES = (1, 50, 95, 100)


def _pil(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _encode_u8(frames: np.ndarray, quality, sub: str):
    """uint8 [F,H,W,3] -> list of files through ops.jpeg_encode, with the sizes checked against ops.jpeg_bound."""
    from dove_amd import ops
    F, H, W, _ = frames.shape
    out, sizes = ops.jpeg_encode(torch.from_numpy(frames).cuda().permute(0, 3, 1, 2), quality, sub)
    sizes = sizes.cpu().tolist()
    bound = ops.jpeg_bound(H, W, sub)
    assert out.shape == (F, bound) and all(0 < s <= bound for s in sizes)
    host = out.cpu().numpy()
    return [host[i, :s].tobytes() for i, s in enumerate(sizes)]


def _shapes(sub: str):
    """The issue's small shapes; one interval exactly; a one-MCU tail interval; 10 intervals over 2 MCU rows of 37 MCUs, so that the RST
    index wraps and an interval crosses the row end."""
    from dove_amd import ops
    R, side = ops.jpeg_restart_mcus(), 16 if sub == "420" else 8
    assert R == J.RESTART_MCUS and -(-2 * 37 // R) >= 9 and 37 % R
    return [(1, 1), (8, 8), (16, 16), (17, 33), (40, 56), (side, R * side), (side - 3, R * side + 1), (side + 3, 36 * side + 5)]


@pytest.mark.parametrize("kind", J.KINDS)
@pytest.mark.parametrize("sub", SUBS)
def test_bytes_equal_the_definition(sub, kind):
    for h, w in _shapes(sub):
        frames = np.stack([J.image(h, w, kind, seed=q) for q in QUALITIES])
        files = _encode_u8(frames, list(QUALITIES), sub)                       # one call, a quality per frame
        for data, x, q in zip(files, frames, QUALITIES):
            want = J.encode(x, q, sub)
            assert data == want, (h, w, q, len(data), len(want))


def test_largest_levels_and_dense_stuffing_equal_the_definition():
    for sub in SUBS:
        frames = np.stack([J.basis_frame(40, 56, v, u) for v, u in ((4, 4), (7, 7), (0, 1), (0, 0))] + [J.image(40, 56, "noise", seed=3)])
        for data, x in zip(_encode_u8(frames, 100, sub), frames):
            assert data == J.encode(x, 100, sub)


def test_invariance_repeat_batch_quality_and_views():
    from dove_amd import ops
    for sub in SUBS:
        h, w = 19, 149
        frames = np.stack([J.image(h, w, "smooth", seed=i) for i in range(3)])
        files = _encode_u8(frames, 90, sub)
        assert _encode_u8(frames, 90, sub) == files                                   # a repeat call
        assert _encode_u8(frames[1:2], 90, sub) == files[1:2]                         # frame 1 alone
        assert _encode_u8(frames[::-1].copy(), 90, sub) == files[::-1]                # another batch position
        mixed = _encode_u8(frames, [90, 30, 90], sub)                                 # a neighbour's quality changes nothing
        assert mixed[0] == files[0] and mixed[2] == files[2] and mixed[1] == J.encode(frames[1], 30, sub)
        dev = torch.from_numpy(frames).cuda()
        planar = dev.permute(0, 3, 1, 2).contiguous()                                 # [F,3,H,W] in memory
        big = torch.zeros(3, h + 5, w + 7, 3, dtype=torch.uint8, device="cuda")
        big[:, 2:2 + h, 3:3 + w] = dev
        for view in (planar, big[:, 2:2 + h, 3:3 + w].permute(0, 3, 1, 2)):           # a strided u8 NHWC crop
            out, sizes = ops.jpeg_encode(view, 90, sub)
            assert [out[i, :s].cpu().numpy().tobytes() for i, s in enumerate(sizes.cpu().tolist())] == files


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32))
def test_float_clip_views_equal_postprocess_then_u8(dtype):
    from dove_amd import jpeg, prepost
    g = np.random.default_rng(5)
    F, H, W = 5, 24, 44
    v = g.random((3, F, H, W), dtype=np.float32) * 1.2 - 0.1                          # [-0.1, 1.1]: both clamps act
    k = g.integers(0, 256, size=v.shape).astype(np.float32) / np.float32(255)         # exact k / 255: the truncation's edge
    video = torch.from_numpy(np.where(g.random(v.shape) < 0.3, k, v)).to(dtype).cuda()
    frames = prepost.postprocess_frames(video[None], 1, 1, 2)                         # crops 1 frame, 4 rows, 8 columns
    Fo, Ho, Wo = frames.shape[:3]
    assert (Fo, Ho, Wo) == (F - 1, H - 4, W - 8)
    for sub in SUBS:
        want = jpeg.encode(frames, 95, sub)
        assert want == [J.encode(x, 95, sub) for x in frames.cpu().numpy()]
        crop = video[:, :Fo, :Ho, :Wo]
        assert jpeg.encode(crop, 95, sub) == want                                     # [3,F,H,W], read in place
        assert jpeg.encode(crop.permute(1, 0, 2, 3), 95, sub) == want                 # [F,3,H,W]


def test_sizes_stay_inside_the_bound_for_quality_100_noise():
    from dove_amd import ops
    x = np.stack([J.image(200, 333, "noise"), J.image(200, 333, "binary")])
    for sub in SUBS:
        files = _encode_u8(x, 100, sub)                                               # _encode_u8 asserts sizes <= bound
        assert max(len(f) for f in files) <= ops.jpeg_bound(200, 333, sub)
        for data, img in zip(files, x):
            assert _pil(data).shape == img.shape
    assert np.abs(_pil(files[0]).astype(int) - x[0].astype(int)).mean() < 2          # 4:4:4 at quality 100 keeps the noise


def test_production_size_frame_decodes_to_the_library_roundtrip():
    """One 2880 x 5120 frame, 4:2:0: Pillow's decode of the file against ops.jpeg_roundtrip, the device's own decode of the same levels."""
    from dove_amd import ops
    H, W = 2880, 5120
    g = torch.Generator(device="cuda").manual_seed(0)
    y, x = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    base = torch.stack([127.5 + 120 * torch.sin(x / 37.0) * torch.cos(y / 23.0), 127.5 + 120 * torch.sin((x + y) / 91.0),
                        (x * 255 / (W - 1)).float()], -1)
    frame = (base + 12 * torch.randn(H, W, 3, device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
    out, sizes = ops.jpeg_encode(frame[None].permute(0, 3, 1, 2), 95, "420")
    n = int(sizes.item())
    assert 0 < n <= ops.jpeg_bound(H, W, "420") and n < H * W * 3
    got = _pil(out[0, :n].cpu().numpy().tobytes())
    want = ops.jpeg_roundtrip(frame[None].float(), 95)[0].cpu().numpy()
    assert got.shape == (H, W, 3)
    assert int(np.abs(got.astype(np.int16) - want.astype(np.int16)).max()) <= J.PILLOW_BOUND


def test_save_frames_and_save_avi(tmp_path):
    from dove_amd import avi, jpeg, prepost
    frames = np.stack([J.image(40, 52, "smooth", seed=i) for i in range(5)])
    prepost.save_frames_as_jpeg(torch.from_numpy(frames), str(tmp_path / "a"), 90, "420")          # a host tensor is uploaded
    assert sorted(os.listdir(tmp_path / "a")) == [f"{i:03d}.jpg" for i in range(5)]
    files = [(tmp_path / "a" / f"{i:03d}.jpg").read_bytes() for i in range(5)]
    assert files == [J.encode(x, 90, "420") for x in frames]
    names = [f"x{i}.jpg" for i in range(5)]                                                          # groups of one frame, own names
    paths = jpeg.save_frames(torch.from_numpy(frames).cuda(), str(tmp_path / "b"), names=names, quality=90, subsampling="420", budget_bytes=1)
    assert [os.path.basename(p) for p in paths] == names and [open(p, "rb").read() for p in paths] == files
    assert jpeg.save_avi(torch.from_numpy(frames), str(tmp_path / "c.avi"), fps=24, quality=90, subsampling="420") == 5
    check_avi((tmp_path / "c.avi").read_bytes(), files, 52, 40, 24)
    groups = (torch.from_numpy(frames[a:b]) for a, b in ((0, 2), (2, 5)))                            # an iterable of frame groups
    assert jpeg.save_avi(groups, str(tmp_path / "d.avi"), fps=24, quality=90, subsampling="420", budget_bytes=1) == 5
    assert (tmp_path / "d.avi").read_bytes() == (tmp_path / "c.avi").read_bytes()
    with pytest.raises(avi.AviError):
        jpeg.save_avi(torch.from_numpy(frames), "-")
    jpeg.main([str(tmp_path / "a"), "--avi", str(tmp_path / "e.avi"), "--quality", "80", "--fps", "12", "--subsampling", "444"])
    back = prepost.load_frames(str(tmp_path / "a")).numpy()                                          # the tool reads the .jpg folder
    check_avi((tmp_path / "e.avi").read_bytes(), [J.encode(x, 80, "444") for x in back], 52, 40, 12)


def test_cli_jpg_save_and_avi_save(golden_dir, tmp_path):
    from dove_amd import cli, ops
    from test_jpeg_cpu import walk_riff
    gold = np.load(os.path.join(golden_dir, "cli_npy_before_y4m.npz"))
    inp = tmp_path / "in"
    inp.mkdir()
    np.save(inp / "clip0.npy", gold["clip"])
    common = ["--input_dir", str(inp), "--random_init", "--num_layers", "1", "--prompt_embedding",
              os.path.join(golden_dir, "empty_prompt_embedding.safetensors"), "--save_format", "yuv420p", "--fps", "24"]
    cli.main(common + ["--output_path", str(tmp_path / "png"), "--png_save"])
    cli.main(common + ["--output_path", str(tmp_path / "jpg"), "--jpg_save", "--jpeg_quality", "90"])
    cli.main(common + ["--output_path", str(tmp_path / "avi"), "--avi_save", "--jpeg_quality", "90"])
    names = sorted(os.listdir(tmp_path / "png" / "clip0"))
    frames = np.stack([_pil((tmp_path / "png" / "clip0" / n).read_bytes()) for n in names])
    assert np.array_equal(frames, gold["frames"])
    want = ops.jpeg_roundtrip(torch.from_numpy(frames).cuda().float(), 90).cpu().numpy().astype(np.int16)
    assert sorted(os.listdir(tmp_path / "jpg" / "clip0")) == [n[:-4] + ".jpg" for n in names]
    files = [(tmp_path / "jpg" / "clip0" / (n[:-4] + ".jpg")).read_bytes() for n in names]
    for data, w in zip(files, want):
        assert int(np.abs(_pil(data).astype(np.int16) - w).max()) <= J.PILLOW_BOUND
    assert sorted(p.name for p in (tmp_path / "avi").iterdir()) == ["clip0.avi"]
    data = (tmp_path / "avi" / "clip0.avi").read_bytes()
    check_avi(data, files, frames.shape[2], frames.shape[1], 24)
    assert len(walk_riff(data)["/movi/00dc"]) == len(names)
    for flags in (["--jpg_save", "--avi_save"], ["--avi_save", "--png_save"], ["--jpg_save", "--y4m_save"]):
        with pytest.raises(ValueError, match="choose one output form"):
            cli.main(common + ["--output_path", str(tmp_path / "x")] + flags)
    with pytest.raises(ValueError, match="yuv422p"):
        cli.main(common[:-4] + ["--output_path", str(tmp_path / "x"), "--avi_save", "--save_format", "yuv422p"])
