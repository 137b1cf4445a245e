"""GPU PNG encoder (csrc/png.hip, dove_amd/png.py): every file decodes in PIL to its input, its zlib stream inflates to
tests/png_ref.py's filtered stream bit for bit, and its size stays inside the flat-code bound and the per-segment entropy bound."""
import io
import os
import zlib

import numpy as np
import pytest
import torch

import png_ref as R

pytestmark = pytest.mark.gpu


def _decode(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def _sizes(c):
    from dove_amd import ops
    rows = ops.png_segment_rows(100, c)
    return [(1, 1), (1, 7), (3, 5), (16, 16), (17, 33), (64, 100), (rows - 1, 100), (rows, 100), (rows + 1, 100), (2 * rows + 1, 100),
            (5, 255), (5, 256), (5, 257)]


def _encode_u8(frames: np.ndarray):
    """uint8 [F,H,W,C] -> list of files through ops.png_encode, with the raw sizes checked against ops.png_bound."""
    from dove_amd import ops
    F, H, W, C = frames.shape
    out, sizes = ops.png_encode(torch.from_numpy(frames).cuda().permute(0, 3, 1, 2))
    sizes = sizes.cpu().tolist()
    assert out.shape == (F, ops.png_bound(H, W, C)) and all(0 < s <= ops.png_bound(H, W, C) for s in sizes)
    host = out.cpu().numpy()
    return [host[i, :s].tobytes() for i, s in enumerate(sizes)]


def _check_file(data: bytes, img: np.ndarray, flat: bool = False):
    """One file against its [H,W,C] image: PIL round trip, CRCs, Adler-32 (zlib.decompress checks it), the filtered stream, the sizes."""
    from dove_amd import ops
    H, W, C = img.shape
    assert np.array_equal(_decode(data), img if C == 3 else img[:, :, 0])
    ihdr, idat, chunks = R.parse(data)
    assert ihdr == dict(width=W, height=H, depth=8, colour_type=2 if C == 3 else 0, compression=0, filter=0, interlace=0)
    want = R.filtered_stream(img)
    assert zlib.decompress(idat) == want
    rows = ops.png_segment_rows(W, C)
    assert chunks == -(-H // rows)
    assert len(data) <= ops.png_bound(H, W, C)
    assert len(idat) <= R.entropy_bound(want, rows, W * C + 1), (len(idat), R.entropy_bound(want, rows, W * C + 1))
    if flat:
        assert len(data) <= R.flat_code_size(want, rows, W * C + 1)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("c", (1, 3))
def test_round_trip_stream_and_size(c, kind):
    for h, w in _sizes(c):
        frames = R.images(h, w, c, kind, frames=3)
        files = _encode_u8(frames)
        for data, img in zip(files, frames):
            _check_file(data, img, flat=kind == "noise")


def test_invariance_repeat_batch_and_views():
    from dove_amd import ops
    for h, w in ((17, 33), (64, 100), (5, 256)):
        frames = R.images(h, w, 3, "smooth", frames=3, seed=1)
        files = _encode_u8(frames)
        assert _encode_u8(frames) == files                                            # a repeat call
        assert _encode_u8(frames[1:2]) == files[1:2]                                  # frame 1 alone
        dev = torch.from_numpy(frames).cuda()
        planar = dev.permute(0, 3, 1, 2).contiguous()                                 # [F,3,H,W] in memory
        big = torch.zeros(3, h + 5, w + 7, 3, dtype=torch.uint8, device="cuda")
        big[:, 2:2 + h, 3:3 + w] = dev
        for view in (planar, big[:, 2:2 + h, 3:3 + w].permute(0, 3, 1, 2)):
            out, sizes = ops.png_encode(view)
            got = [out[i, :s].cpu().numpy().tobytes() for i, s in enumerate(sizes.cpu().tolist())]
            assert got == files


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32))
def test_float_clip_views_equal_postprocess_then_u8(dtype):
    from dove_amd import png, prepost
    g = np.random.default_rng(5)
    F, H, W = 5, 24, 44
    v = g.random((3, F, H, W), dtype=np.float32) * 1.2 - 0.1                          # [-0.1, 1.1]: both clamps act
    k = g.integers(0, 256, size=v.shape).astype(np.float32) / np.float32(255)         # exact k / 255: the truncation's edge
    video = torch.from_numpy(np.where(g.random(v.shape) < 0.3, k, v)).to(dtype).cuda()
    frames = prepost.postprocess_frames(video[None], 1, 1, 2)                         # crops 1 frame, 4 rows, 8 columns
    Fo, Ho, Wo = frames.shape[:3]
    assert (Fo, Ho, Wo) == (F - 1, H - 4, W - 8)
    want = png.encode(frames)
    crop = video[:, :Fo, :Ho, :Wo]
    assert png.encode(crop) == want                                                   # [3,F,H,W], read in place
    assert png.encode(crop.permute(1, 0, 2, 3)) == want                               # [F,3,H,W]
    for data, img in zip(want, frames.cpu().numpy()):
        _check_file(data, img)


def _inflate(data: torch.Tensor, segment_bytes: int) -> bytes:
    from dove_amd import lib as L
    from dove_amd import ops
    out, size = ops.zlib_huffman(data.cuda(), segment_bytes)
    n = int(size.item())
    assert 0 < n <= int(L.load().dove_zlib_huffman_bound(data.numel(), segment_bytes))
    return zlib.decompress(out[:n].cpu().numpy().tobytes())


def test_coder_limits_code_lengths_to_15_bits():
    """Byte k occurs Fib(k) times, k = 0..22 (46367 bytes, one 64 KiB segment): an unrestricted Huffman code is 22 deep there."""
    fib = [0, 1]
    while len(fib) < 23:
        fib.append(fib[-1] + fib[-2])
    buf = np.concatenate([np.full(f, k, np.uint8) for k, f in enumerate(fib)])
    buf = np.random.default_rng(0).permutation(buf)
    assert _inflate(torch.from_numpy(buf), 65536) == buf.tobytes()


def test_coder_edge_buffers():
    g = np.random.default_rng(1)
    seg = 1024
    cases = [np.full(5000, 7, np.uint8), np.full(3000, 255, np.uint8), np.array([200], np.uint8)]
    cases += [g.integers(0, 256, size=n, dtype=np.uint8) for n in (seg - 1, seg, seg + 1, 5 * seg + 3)]
    cases += [np.clip(g.normal(0, 3, size=40000), -128, 127).astype(np.int8).view(np.uint8)]
    for buf in cases:
        for s in (seg, 32768):
            assert _inflate(torch.from_numpy(buf), s) == buf.tobytes(), (len(buf), s)


def test_production_size_frames():
    one = R.images(720, 1280, 3, "smooth", frames=1)
    (data,) = _encode_u8(one)
    _check_file(data, one[0])
    three = R.images(720, 1280, 3, "smooth", frames=3, seed=2)
    for data, img in zip(_encode_u8(three), three):
        _check_file(data, img)


def test_save_frames_surfaces(tmp_path):
    from dove_amd import png, prepost
    frames = R.images(40, 52, 3, "smooth", frames=5)
    prepost.save_frames_as_png(torch.from_numpy(frames), str(tmp_path / "a"), encoder="gpu")       # a host tensor is uploaded
    assert sorted(os.listdir(tmp_path / "a")) == [f"{i:03d}.png" for i in range(5)]
    for i, fr in enumerate(frames):
        assert np.array_equal(_decode((tmp_path / "a" / f"{i:03d}.png").read_bytes()), fr)
    # frame groups of one frame (a tiny budget) write the same files under the caller's names
    names = [f"x{i}.png" for i in range(5)]
    paths = png.save_frames(torch.from_numpy(frames).cuda(), str(tmp_path / "b"), names=names, budget_bytes=1)
    assert [os.path.basename(p) for p in paths] == names
    for i in range(5):
        assert (tmp_path / "b" / names[i]).read_bytes() == (tmp_path / "a" / f"{i:03d}.png").read_bytes()
    grey = png.encode(torch.from_numpy(frames[:, :, :, 0]))                                        # [F,H,W] uint8: grey files
    assert np.array_equal(_decode(grey[2]), frames[2, :, :, 0])


def _same_pngs(a, b):
    """Two folders hold the same file names, and every file decodes to the same pixels."""
    names = sorted(n for n in os.listdir(a) if n.endswith(".png"))
    assert names and names == sorted(n for n in os.listdir(b) if n.endswith(".png"))
    for n in names:
        assert np.array_equal(_decode(open(os.path.join(a, n), "rb").read()), _decode(open(os.path.join(b, n), "rb").read())), n
        R.parse(open(os.path.join(b, n), "rb").read())
    return names


def test_degrade_and_colorfix_tools_png_encoder_gpu_equals_pil(tmp_path):
    from PIL import Image

    from dove_amd import colorfix, degrade
    clip = R.images(48, 64, 3, "smooth", frames=5, seed=3)
    src = tmp_path / "gt"
    src.mkdir()
    np.save(src / "a.npy", clip)
    for enc in ("pil", "gpu"):
        degrade.main(["--input_dir", str(src), "--output_path", str(tmp_path / f"lq_{enc}"), "--preset", "bicubic", "--scale", "4",
                      "--block", "2", "--png_save", "--png_encoder", enc])
    assert _same_pngs(tmp_path / "lq_pil" / "a", tmp_path / "lq_gpu" / "a") == [f"{i:03d}.png" for i in range(5)]
    pred, source = tmp_path / "pred", tmp_path / "source"
    for d in (pred, source, pred / "b", source / "b"):
        d.mkdir()
    style = R.images(48, 64, 3, "smooth", frames=5, seed=4)
    for i in range(3):
        Image.fromarray(clip[i]).save(pred / "b" / f"{i:03d}.png")
        Image.fromarray(style[i]).save(source / "b" / f"{i:03d}.png")
    Image.fromarray(clip[4]).save(pred / "e.png")                      # a single image: written as one file
    Image.fromarray(style[4]).save(source / "e.png")
    for enc in ("pil", "gpu"):
        done = colorfix.main(["--pred", str(pred), "--source", str(source), "--out", str(tmp_path / f"fix_{enc}"), "--mode", "wavelet",
                              "--png_encoder", enc])
        assert done == ["b", "e"]
    assert len(_same_pngs(tmp_path / "fix_pil" / "b", tmp_path / "fix_gpu" / "b")) == 3
    assert _same_pngs(tmp_path / "fix_pil", tmp_path / "fix_gpu") == ["e.png"]


def test_cli_png_encoder_gpu_equals_pil(golden_dir, tmp_path):
    from dove_amd import cli
    inp = tmp_path / "in"
    inp.mkdir()
    clip = np.random.default_rng(0).integers(0, 256, size=(5, 16, 16, 3), dtype=np.uint8)
    np.save(inp / "clip0.npy", clip)
    emb = os.path.join(golden_dir, "empty_prompt_embedding.safetensors")
    common = ["--input_dir", str(inp), "--random_init", "--num_layers", "1", "--prompt_embedding", emb, "--png_save"]
    cli.main(common + ["--output_path", str(tmp_path / "pil")])
    cli.main(common + ["--output_path", str(tmp_path / "gpu"), "--png_encoder", "gpu"])
    names = sorted(os.listdir(tmp_path / "pil" / "clip0"))
    assert names == sorted(os.listdir(tmp_path / "gpu" / "clip0")) == [f"{i:03d}.png" for i in range(5)]
    for n in names:
        a, b = _decode((tmp_path / "pil" / "clip0" / n).read_bytes()), _decode((tmp_path / "gpu" / "clip0" / n).read_bytes())
        assert a.shape == (64, 64, 3) and np.array_equal(a, b)
        R.parse((tmp_path / "gpu" / "clip0" / n).read_bytes())
