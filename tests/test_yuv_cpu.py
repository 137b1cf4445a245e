"""CPU side of the Y4M video I/O: the integer definition of the colour conversion (tests/yuv_ref.py) against float64 and against Pillow,
the container (dove_amd.y4m), the incremental chunk planner (dove_amd.stream.ChunkPlanner) and the new header symbols."""
import io
import os
import re
import threading

import numpy as np
import pytest

import yuv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRICES = ("bt601", "bt709")
RANGES = ("limited", "full")
GRID = [(9, 0), (17, 8), (33, 8), (25, 8), (12, 4), (16, 8), (10, 9)]


# ---- 1. the definition is sane -----------------------------------------------------------------------------------------------------
def _float_forward(rgb, matrix, rng):
    fwd, _, off = R.float_matrices(matrix, rng)
    return np.clip(np.rint(rgb.astype(np.float64) @ fwd.T + np.array(off, dtype=np.float64)), 0, 255).astype(np.int64)


def _float_inverse(yuv, matrix, rng):
    _, inv, off = R.float_matrices(matrix, rng)
    return np.clip(np.rint((yuv.astype(np.float64) - np.array(off, dtype=np.float64)) @ inv.T), 0, 255).astype(np.int64)


@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_fixed_point_is_the_float_formula_within_one_lsb(matrix, rng):
    """2,000,000 random triples: the 16-bit fixed point differs from clip(rint(float64 formula)) by at most 1 LSB, and at all on at most
    0.5 % of the samples (the restatement alone gives about 0.1 %; a wrong coefficient shifts whole ranges of values)."""
    g = np.random.default_rng(20260116)
    rgb = g.integers(0, 256, size=(1, 1000, 2000, 3), dtype=np.uint8)
    got = R.rgb_to_yuv(rgb, matrix, rng, "444").reshape(3, -1).T.astype(np.int64)
    want = _float_forward(rgb.reshape(-1, 3), matrix, rng)
    d = np.abs(got - want)
    print(f"[yuv] forward {matrix} {rng}: max {d.max()}, share {(d > 0).mean():.5f}")
    assert d.max() <= 1 and (d > 0).mean() <= 0.005
    yuv = g.integers(0, 256, size=(1, 3 * 1000 * 2000), dtype=np.uint8)
    got = R.yuv_to_rgb(yuv, 1000, 2000, matrix, rng, "444").reshape(-1, 3).astype(np.int64)
    want = _float_inverse(yuv.reshape(3, -1).T, matrix, rng)
    d = np.abs(got - want)
    print(f"[yuv] inverse {matrix} {rng}: max {d.max()}, share {(d > 0).mean():.5f}")
    assert d.max() <= 1 and (d > 0).mean() <= 0.005


def test_bt601_full_agrees_with_pillow_within_one_lsb():
    """Pillow's YCbCr is JFIF bt601 full range, an independent implementation; it truncates where this rounds, so many samples differ by
    exactly 1 and none by more."""
    from PIL import Image
    g = np.random.default_rng(7)
    rgb = g.integers(0, 256, size=(1024, 2048, 3), dtype=np.uint8)
    pil = np.asarray(Image.fromarray(rgb, "RGB").convert("YCbCr")).astype(np.int64)
    got = R.rgb_to_yuv(rgb[None], "bt601", "full", "444").reshape(3, 1024, 2048).transpose(1, 2, 0).astype(np.int64)
    d = np.abs(got - pil)
    print(f"[yuv] Pillow forward: max {d.max()}, share {(d > 0).mean():.4f}")
    assert d.max() <= 1
    ycc = g.integers(0, 256, size=(1024, 2048, 3), dtype=np.uint8)
    pil = np.asarray(Image.fromarray(ycc, "YCbCr").convert("RGB")).astype(np.int64)
    payload = np.ascontiguousarray(ycc.transpose(2, 0, 1)).reshape(1, -1)
    got = R.yuv_to_rgb(payload, 1024, 2048, "bt601", "full", "444")[0].astype(np.int64)
    d = np.abs(got - pil)
    print(f"[yuv] Pillow inverse: max {d.max()}, share {(d > 0).mean():.4f}")
    assert d.max() <= 1


@pytest.mark.parametrize("matrix", MATRICES)
def test_full_range_444_round_trip_within_one_lsb(matrix):
    g = np.random.default_rng(3)
    rgb = g.integers(0, 256, size=(2, 300, 500, 3), dtype=np.uint8)
    back = R.yuv_to_rgb(R.rgb_to_yuv(rgb, matrix, "full", "444"), 300, 500, matrix, "full", "444")
    assert np.abs(back.astype(np.int64) - rgb.astype(np.int64)).max() <= 1


@pytest.mark.parametrize("chroma", ("444", "422", "420"))
@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_grey_has_neutral_chroma(matrix, rng, chroma):
    grey = np.repeat(np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1), 3, axis=3)
    out = R.rgb_to_yuv(grey, matrix, rng, chroma)
    assert (out[:, 256:] == 128).all()
    if rng == "full":
        assert np.array_equal(out[0, :256], np.arange(256, dtype=np.uint8))


def test_tables_of_the_package_are_those_of_the_definition():
    from dove_amd import yuv
    for matrix in MATRICES:
        for rng in RANGES:
            fwd, inv, off = yuv.int_matrices(matrix, rng)
            rf, ri, ro = R.int_matrices(matrix, rng)
            assert fwd == rf.flatten().tolist() and inv == ri.flatten().tolist() and tuple(off) == tuple(ro)
    assert yuv.save_format_to_chroma("yuv420p") == "420" and yuv.save_format_to_chroma("yuv444p") == "444"
    assert yuv.save_format_to_chroma("yuv422p") == "422"
    with pytest.raises(ValueError, match="yuv444p, yuv422p, yuv420p"):
        yuv.save_format_to_chroma("rgb24")


# ---- 2. container ------------------------------------------------------------------------------------------------------------------
def _payloads(n, h, w, chroma, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(n, R.frame_bytes(h, w, chroma)), dtype=np.uint8)


@pytest.mark.parametrize("via_pipe", (False, True))
@pytest.mark.parametrize("chroma,h,w", [("444", 6, 8), ("422", 5, 7), ("420", 5, 7), ("420", 16, 24), ("mono", 3, 5)])
def test_container_round_trip(tmp_path, chroma, h, w, via_pipe):
    from dove_amd import y4m
    data = _payloads(5, h, w, chroma, seed=h * w)
    assert y4m.frame_bytes(h, w, chroma) == data.shape[1]
    if via_pipe:                                                     # non-seekable: the reader never asks for the frame count
        r, wfd = os.pipe()

        def produce():
            with os.fdopen(wfd, "wb") as f, y4m.Y4MWriter(f, w, h, (30000, 1001), chroma, True) as wr:
                wr.write(data[:2])
                wr.write(data[2:])
        t = threading.Thread(target=produce, daemon=True)
        t.start()
        src = os.fdopen(r, "rb")
        assert not src.seekable()
    else:
        path = str(tmp_path / "clip.y4m")
        with y4m.Y4MWriter(path, w, h, (30000, 1001), chroma, True) as wr:
            wr.write(data)
            assert wr.frames_written == 5
        src = path
    with y4m.Y4MReader(src) as rd:
        assert (rd.width, rd.height, rd.chroma, rd.fps, rd.full_range) == (w, h, chroma, (30000, 1001), True)
        assert rd.frame_bytes == data.shape[1]
        a, b, c = rd.read(3), rd.read(3), rd.read(3)
    if via_pipe:
        src.close()
        t.join(10)
        assert not t.is_alive()
    assert a.dtype.is_floating_point is False and tuple(a.shape) == (3, data.shape[1]) and b.shape[0] == 2 and c.shape[0] == 0
    assert np.array_equal(np.concatenate([a.numpy(), b.numpy()]), data)


def test_writer_header_text():
    from dove_amd import y4m
    buf = io.BytesIO()
    with y4m.Y4MWriter(buf, 64, 48, 24, "420", False) as wr:
        wr.write(_payloads(1, 48, 64, "420"))
    raw = buf.getvalue()
    assert raw.startswith(b"YUV4MPEG2 W64 H48 F24:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\nFRAME\n")
    assert len(raw) == len(wr.header) + 6 + 48 * 64 * 3 // 2


@pytest.mark.parametrize("tag,fix", [("C420p10", "yuv420p"), ("C444p12", "yuv444p"), ("C411", "yuv420p"), ("C444alpha", "yuv444p"),
                                     ("C422p10", "yuv422p"), ("It", "yadif"), ("Ib", "yadif"), ("Im", "yadif")])
def test_refused_tags_are_named(tag, fix):
    from dove_amd import y4m
    fields = ["YUV4MPEG2", "W16", "H8", "F25:1", "Ip", "A1:1", "C420jpeg"]
    fields[4 if tag.startswith("I") else 6] = tag
    with pytest.raises(ValueError) as e:
        y4m.Y4MReader(io.BytesIO(" ".join(fields).encode() + b"\n"))
    assert tag in str(e.value) and fix in str(e.value) and "ffmpeg" in str(e.value)


def test_other_malformed_streams_raise():
    from dove_amd import y4m
    with pytest.raises(ValueError, match="not a YUV4MPEG2"):
        y4m.Y4MReader(io.BytesIO(b"RIFF....AVI \n"))
    with pytest.raises(ValueError, match="XCOLORRANGE=BROAD"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 F1:1 XCOLORRANGE=BROAD\n"))
    with pytest.raises(ValueError, match="FRAME"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W2 H2 C444\nFRAMX\n" + bytes(12))).read(1)


def test_truncated_frame_raises_and_clean_eof_ends():
    from dove_amd import y4m
    head = b"YUV4MPEG2 W4 H2 F25:1 Ip A1:1 C444\n"
    full = b"FRAME\n" + bytes(range(24))
    rd = y4m.Y4MReader(io.BytesIO(head + full + full))
    assert rd.read(8).shape[0] == 2 and rd.read(8).shape[0] == 0       # clean EOF at a frame boundary
    rd = y4m.Y4MReader(io.BytesIO(head + full + full[:-5]))
    with pytest.raises(ValueError, match="truncated"):
        rd.read(8)
    rd = y4m.Y4MReader(io.BytesIO(head + full + b"FRA"))
    with pytest.raises(ValueError, match="ends inside"):
        rd.read(8)


def test_ffmpeg_header_parses():
    from dove_amd import y4m, yuv
    line = b"YUV4MPEG2 W320 H180 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=LIMITED"
    rd = y4m.Y4MReader(io.BytesIO(line + b"\n"))
    assert (rd.width, rd.height, rd.fps, rd.tag, rd.chroma, rd.siting_h, rd.full_range) == (320, 180, (30000, 1001), "C420mpeg2", "420",
                                                                                            "left", False)
    assert rd.frame_bytes == 320 * 180 * 3 // 2 and rd.read(4).shape == (0, rd.frame_bytes)
    assert yuv.format_of_reader(rd) == yuv.YuvFormat("420", "bt601", "limited", "left")
    rd = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H8 F25:1 I? XCOLORRANGE=FULL\n"))       # no C tag: 420jpeg
    assert (rd.chroma, rd.siting_h, rd.full_range) == ("420", "centre", True)
    assert {t: y4m.COLOURSPACES[t] for t in R.TAGS} == R.TAGS


# ---- 3. planner --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_len,overlap_t", GRID)
def test_incremental_planner_equals_make_temporal_chunks(chunk_len, overlap_t):
    from dove_amd import stream, tiling
    la = stream.lookahead(chunk_len, overlap_t)
    assert la == 2 * chunk_len - overlap_t
    for F in range(overlap_t + 1, 300):
        planner, got, furthest = stream.ChunkPlanner(chunk_len, overlap_t), [], 0
        while True:
            start = planner.start
            known = min(F, planner.need())                          # one lookahead window at a time, never further
            assert known - start <= la
            chunk = planner.next(known, eof=known == F and planner.need() > F)
            if chunk is None:
                break
            assert chunk[0] == start and chunk[1] <= known
            got.append(chunk[:2])
            furthest = max(furthest, known)
            if chunk[2]:
                assert planner.next(F, True) is None
                break
        assert got == tiling.make_temporal_chunks(F, chunk_len, overlap_t), (F, got)


def test_planner_edges():
    from dove_amd import stream, tiling
    assert tiling.make_temporal_chunks(8, 17, 8) == [] and stream.ChunkPlanner(17, 8).next(8, True) is None    # F <= overlap_t: no chunk
    assert stream.ChunkPlanner(0, 8).next(41, True) == (0, 41, True) and stream.ChunkPlanner(0, 8).need() is None
    with pytest.raises(ValueError, match="chunk_len must be greater than overlap"):
        stream.ChunkPlanner(8, 8)
    with pytest.raises(RuntimeError, match="known frames"):
        stream.ChunkPlanner(17, 8).next(20, False)
    assert stream.output_size(32, 48, 4) == (128, 192) and stream.output_size(30, 45, 4) == (30 * 4, 45 * 4)
    assert stream.output_size(30, 45, 2) == (32 * 2 - 2 * 4, 48 * 2 - 3 * 4)          # the reference's hard-coded pad * 4


# ---- 4. ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_covers_the_yuv_calls():
    from dove_amd import lib as L
    with open(os.path.join(ROOT, "include", "dove_hip.h")) as f:
        src = f.read()
    for name in ("dove_rgb_to_yuv_u8", "dove_yuv_to_rgb_u8", "dove_yuv_frame_bytes"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in L.SIGNATURES or name in L.PLAIN
    assert int(re.search(r"#define\s+DOVE_ABI_VERSION\s+(\d+)", src).group(1)) == 15
    assert "dove_yuv_format" in src and [n for n, _ in L.YuvFormat._fields_] == ["coef", "offset", "chroma", "siting_h"]
    with open(os.path.join(ROOT, "dove_amd", "csrc", "build.sh")) as f:
        assert re.search(r'SRCS="[^"]*\byuv\b', f.read())


def test_frame_bytes_and_argument_checks_need_no_gpu():
    import ctypes as C

    from dove_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    codes = {"444": L.YUV_444, "422": L.YUV_422, "420": L.YUV_420, "mono": L.YUV_MONO}
    for chroma, code in codes.items():
        for h, w in ((1, 1), (2, 2), (5, 7), (720, 1280), (33, 1)):
            assert lib.dove_yuv_frame_bytes(h, w, code) == R.frame_bytes(h, w, chroma)
    assert lib.dove_yuv_frame_bytes(0, 4, 0) == 0 and lib.dove_yuv_frame_bytes(4, 4, 9) == 0
    fmt, view = L.YuvFormat(), L.ImageView()
    fmt.chroma = 7
    assert lib.dove_rgb_to_yuv_u8(C.byref(view), 1, 4, 4, C.byref(fmt), None, None) == -1 and b"chroma" in lib.dove_last_error()
    fmt.chroma = L.YUV_420
    assert lib.dove_rgb_to_yuv_u8(C.byref(view), 1, 4, 4, C.byref(fmt), None, None) == -1 and b"null pointer" in lib.dove_last_error()
    assert lib.dove_yuv_to_rgb_u8(None, 1, 0, 4, C.byref(fmt), None, None) == -1 and b"bad shape" in lib.dove_last_error()
    fmt.coef[0] = 1 << 20
    assert lib.dove_yuv_to_rgb_u8(None, 1, 4, 4, C.byref(fmt), None, None) == -1 and b"coefficients" in lib.dove_last_error()


def test_cli_refuses_save_format_only_where_a_y4m_is_written(tmp_path):
    """--save_format stays accepted and unused without --y4m_save (tests/test_e2e_gpu.py passes yuv420p on an .npy run); with it, a value
    that is not a planar 8-bit YUV format is refused before any model is built."""
    from dove_amd import cli
    with pytest.raises(ValueError, match="--save_format rgb24"):
        cli.main(["--input_dir", str(tmp_path), "--random_init", "--y4m_save", "--save_format", "rgb24"])
    with pytest.raises(ValueError, match="choose one"):
        cli.main(["--input_dir", str(tmp_path), "--random_init", "--y4m_save", "--png_save"])
