"""CPU side of the GPU PNG encoder: the numpy restatement in tests/png_ref.py is right, the size condition of the GPU
tests can be met, the host functions of the ABI, and the surfaces keep PIL as their default."""
import io
import os
import zlib

import numpy as np
import pytest
import torch

import png_ref as R

SHAPES = [(1, 1), (1, 7), (3, 5), (16, 16), (17, 33), (96, 160)]


def _decode(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("c", (1, 3))
def test_filtered_stream_decodes_to_the_image(c, kind):
    for h, w in SHAPES:
        for img in R.images(h, w, c, kind, frames=2):
            stream = R.filtered_stream(img)
            assert len(stream) == h * (w * c + 1)
            got = _decode(R.wrap(stream, h, w, c))
            assert np.array_equal(got, img if c == 3 else img[:, :, 0]), (h, w, c, kind)


def test_filter_choice_takes_the_lower_id_on_a_tie():
    img = np.zeros((3, 4, 3), np.uint8)                      # every filter costs 0 on every row
    assert R.filtered_rows(img)[0].tolist() == [0, 0, 0]
    img = np.tile(np.arange(0, 40, 10, dtype=np.uint8)[None, :, None], (2, 1, 3))
    assert R.filtered_rows(img)[0].tolist() == [1, 2]        # row 0: Sub (90) beats None (180) and ties with Paeth; row 1: Up is 0


def test_parser_checks_crcs():
    data = R.wrap(R.filtered_stream(R.images(5, 6, 3, "noise")[0]), 5, 6, 3)
    ihdr, idat, n = R.parse(data)
    assert ihdr == dict(width=6, height=5, depth=8, colour_type=2, compression=0, filter=0, interlace=0) and n == 1
    bad = bytearray(data)
    bad[45] ^= 1
    with pytest.raises(AssertionError):
        R.parse(bytes(bad))


@pytest.mark.parametrize("rows", (1, 16))
@pytest.mark.parametrize("kind", R.KINDS)
def test_zlib_huffman_only_meets_the_entropy_bound(kind, rows):
    """What the GPU test asks of the encoder, met by zlib's own literal-only coder on every segment: Z_HUFFMAN_ONLY plus a sync flush stays
    inside (H0 n + n) / 8 + 256."""
    worst = 0.0
    for c in (1, 3):
        for img in R.images(96, 160, c, kind, frames=2):
            stream = R.filtered_stream(img)
            for seg in R.segments(stream, rows, 160 * c + 1):
                co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
                size = len(co.compress(seg) + co.flush(zlib.Z_SYNC_FLUSH))
                worst = max(worst, size / R.segment_entropy_bytes(seg))
    assert worst <= 1.0, worst


def test_segment_geometry_and_bound_are_host_functions():
    from dove_amd import ops
    for w in (1, 7, 1280, 10922):
        for c in (1, 3):
            rows = ops.png_segment_rows(w, c)
            assert rows == -(-32768 // (w * c + 1)), (w, c)
            assert rows * (w * c + 1) >= 32768 > (rows - 1) * (w * c + 1)
    assert ops.png_segment_rows(1280, 3) == 9
    assert ops.png_segment_rows(0, 3) == 0 and ops.png_segment_rows(4, 2) == 0 and ops.png_bound(0, 4, 3) == 0
    g = np.random.default_rng(0)
    for h, w, c in [(1, 1, 1), (17, 33, 3), (96, 160, 3), (720, 1280, 3), (9, 1280, 1)]:
        stream = np.full(h * (w * c + 1), 255, np.uint8).tobytes()           # the flat code's worst case: every symbol takes 9 bits
        rows = ops.png_segment_rows(w, c)
        segs = -(-h // rows)
        assert ops.png_bound(h, w, c) == (len(stream) * 9 + 7) // 8 + 256 * segs + 64
        assert ops.png_bound(h, w, c) >= R.flat_code_size(stream, rows, w * c + 1)
        noise = g.integers(0, 256, size=len(stream), dtype=np.uint8).tobytes()
        assert ops.png_bound(h, w, c) >= R.flat_code_size(noise, rows, w * c + 1)


def test_encoder_arguments_are_validated_before_any_device_call():
    import ctypes as C

    from dove_amd import lib as L
    lib = L.load()
    v = L.ImageView()
    v.data, v.dtype, v.sn, v.sc, v.sh, v.sw = 1, L.U8, 48, 1, 12, 3
    assert lib.dove_png_encode(C.byref(v), 1, 4, 4, 2, None, 0, None, None, None) == -1 and b"channels" in lib.dove_last_error()
    assert lib.dove_png_encode(C.byref(v), 0, 4, 4, 3, None, 0, None, None, None) == -1 and b"shape" in lib.dove_last_error()
    assert lib.dove_png_encode(C.byref(v), 1, 4, 4, 3, None, 0, None, None, None) == -1 and b"workspace" in lib.dove_last_error()
    assert lib.dove_zlib_huffman(None, 10, 512, None, 0, None, None, None) == -1 and b"segment_bytes" in lib.dove_last_error()
    assert lib.dove_zlib_huffman(None, 0, 1024, None, 0, None, None, None) == -1 and b"nbytes" in lib.dove_last_error()
    assert lib.dove_zlib_huffman_bound(10, 512) == 0 and lib.dove_zlib_huffman_bound(1000, 1024) == 1125 + 256 + 64


def test_save_frames_as_png_default_writes_what_pil_writes(tmp_path):
    from PIL import Image

    from dove_amd import prepost
    frames = R.images(12, 20, 3, "smooth", frames=3)
    prepost.save_frames_as_png(torch.from_numpy(frames), str(tmp_path / "a"))
    assert sorted(os.listdir(tmp_path / "a")) == ["000.png", "001.png", "002.png"]
    for i, fr in enumerate(frames):
        want = io.BytesIO()
        Image.fromarray(fr).save(want, format="PNG")
        assert (tmp_path / "a" / f"{i:03d}.png").read_bytes() == want.getvalue()
    with pytest.raises(ValueError):
        prepost.save_frames_as_png(torch.from_numpy(frames), str(tmp_path / "b"), encoder="zip")


def test_parsers_accept_png_encoder_and_default_to_pil():
    from dove_amd import cli, colorfix, degrade
    for parser, need in ((cli.build_parser(), ["--input_dir", "x"]), (degrade.build_parser(), ["--input_dir", "x"]),
                         (colorfix.build_parser(), ["--pred", "a", "--source", "b", "--out", "c"])):
        assert parser.parse_args(need).png_encoder == "pil"
        assert parser.parse_args(need + ["--png_encoder", "gpu"]).png_encoder == "gpu"
        with pytest.raises(SystemExit):
            parser.parse_args(need + ["--png_encoder", "zlib"])


def test_layouts_of_the_python_module():
    from dove_amd import png
    assert tuple(png.as_nchw(torch.zeros(2, 5, 6, 3, dtype=torch.uint8)).shape) == (2, 3, 5, 6)
    assert tuple(png.as_nchw(torch.zeros(2, 5, 6, dtype=torch.uint8)).shape) == (2, 1, 5, 6)
    assert tuple(png.as_nchw(torch.zeros(3, 4, 5, 6)).shape) == (4, 3, 5, 6)                    # [3,F,H,W]
    assert tuple(png.as_nchw(torch.zeros(4, 3, 5, 6, dtype=torch.bfloat16)).shape) == (4, 3, 5, 6)
    assert tuple(png.as_nchw(torch.zeros(3, 3, 5, 6), layout="cfhw").shape) == (3, 3, 5, 6)
    with pytest.raises(ValueError):
        png.as_nchw(torch.zeros(2, 5, 6, 4, dtype=torch.uint8))
    with pytest.raises(TypeError):
        png.as_nchw(torch.zeros(2, 3, 5, 6, dtype=torch.float64))
    assert png.group_frames(720, 1280, 3) >= 33 and png.group_frames(720, 1280, 3, budget_bytes=1) == 1
