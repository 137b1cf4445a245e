"""The definition of the GPU JPEG encoder (tests/jpeg_ref.py) against degrade_ref and Pillow, the AVI writer against an independent RIFF
walker, and the C ABI's refusals - all without a GPU."""
import io
import struct

import numpy as np
import pytest
import torch

import degrade_ref as D
import jpeg_ref as J

SUBS = ("420", "444")


def _pil(data: bytes):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def _check_file(data: bytes, x: np.ndarray, q: int, sub: str, lev: np.ndarray = None):
    """One file of the definition (or the device) against its frame: Pillow's view of the header, Pillow's pixels within PILLOW_BOUND of
    the definition's own decode, and the independent Huffman decoder's levels."""
    H, W, _ = x.shape
    lev = J.levels(x, q, sub) if lev is None else lev
    im = _pil(data)
    assert im.size == (W, H) and im.mode == "RGB"
    want_q = {0: D.quant_table(D.JPEG_LUMA, q).reshape(64), 1: D.quant_table(D.JPEG_CHROMA, q).reshape(64)}
    got_q = {k: np.asarray(v) for k, v in im.quantization.items()}
    assert sorted(got_q) == [0, 1]
    for k in (0, 1):                                     # Pillow hands the table out in zigzag or natural order, depending on its version
        assert np.array_equal(got_q[k], want_q[k]) or np.array_equal(got_q[k], want_q[k][J.ZIGZAG]), (k, got_q[k])
    assert im.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)] if sub == "420" else im.layer == [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    ref = J.decode_pixels(lev, H, W, q, sub).astype(np.int64)
    err = int(np.abs(np.asarray(im).astype(np.int64) - ref).max())
    assert err <= J.PILLOW_BOUND, err
    assert np.array_equal(J.decode_levels(data), lev)
    return err


@pytest.mark.parametrize("kind", J.KINDS)
def test_levels_are_the_forward_half_of_degrade_ref(kind):
    """levels x Q through degrade_ref's inverse half (decode_pixels uses its DCT matrix, upsampling and colour matrix) is jpeg_frame."""
    for h, w in J.SHAPES:
        for q in J.QUALITIES:
            x = J.image(h, w, kind)
            lev = J.levels(x, q, "420")
            assert np.array_equal(J.decode_pixels(lev, h, w, q, "420"), D.jpeg_frame(x, q)), (h, w, q)
            assert np.abs(lev[..., 1:]).max() < 1023 and lev[..., 0, 0].min() >= -1024 and lev[..., 0, 0].max() <= 1016   # no clamp binds


def test_huffman_tables_are_well_formed_and_what_libjpeg_writes():
    for name, (bits, vals) in J.TABLES.items():
        assert len(bits) == 16 and sum(bits) == len(vals) == len(set(vals)) == (12 if name.startswith("dc") else 162)
        kraft = sum(n * 2.0 ** -(i + 1) for i, n in enumerate(bits))
        assert kraft < 1
        for sym, (code, length) in J.huffman_codes(bits, vals).items():
            assert code != (1 << length) - 1, (name, sym)                       # no all-ones code
    from PIL import Image                                                       # a non-optimised libjpeg file carries the Annex-K tables
    buf = io.BytesIO()
    Image.fromarray(J.image(16, 16, "noise")).save(buf, "JPEG", quality=90)
    data, pos, seen = buf.getvalue(), 2, {}
    while data[pos + 1] != 0xDA:
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        while data[pos + 1] == 0xC4 and body:
            cnt = sum(body[1:17])
            seen[body[0]] = (list(body[1:17]), list(body[17:17 + cnt]))
            body = body[17 + cnt:]
        pos += 2 + n
    for tc_th, name in ((0x00, "dc_luma"), (0x10, "ac_luma"), (0x01, "dc_chroma"), (0x11, "ac_chroma")):
        assert seen[tc_th] == (list(J.TABLES[name][0]), list(J.TABLES[name][1])), name


@pytest.mark.parametrize("kind", J.KINDS)
@pytest.mark.parametrize("sub", SUBS)
def test_pillow_decodes_the_definition_and_the_levels_round_trip(sub, kind):
    """Measured on the build machine (Pillow 12.2, libjpeg-turbo): max |Pillow - decode_pixels| = 3 for 4:2:0 and 3 for 4:4:4 over these
    360 cases; PILLOW_BOUND = 4 is asserted."""
    worst = 0
    for h, w in J.SHAPES:
        for q in J.QUALITIES:
            x = J.image(h, w, kind)
            worst = max(worst, _check_file(J.encode(x, q, sub), x, q, sub))
    print(f"max |Pillow - definition| {sub} {kind}: {worst}")


@pytest.mark.parametrize("sub", SUBS)
def test_largest_levels_and_dc_differences_stay_decodable(sub):
    big_ac, big_dc = 0, 0
    for v, u in ((4, 4), (7, 7), (0, 1), (1, 0), (1, 1), (0, 0)):
        x = J.basis_frame(40, 56, v, u)
        lev = J.levels(x, 100, sub)
        _check_file(J.encode(x, 100, sub), x, 100, sub, lev)
        big_ac = max(big_ac, int(np.abs(lev.reshape(-1, 64)[:, 1:]).max()))
        big_dc = max(big_dc, int(np.ptp(lev[..., 0, 0])))
    assert big_ac > 800 and big_dc > 2000                                       # size categories 10 and 11 were coded


@pytest.mark.parametrize("sub", SUBS)
def test_dense_stuffing_and_interval_ends(sub):
    x = J.image(40, 56, "noise", seed=3)
    data = J.encode(x, 100, sub)
    assert data.count(b"\xff\x00") > 20
    _check_file(data, x, 100, sub)
    side = 16 if sub == "420" else 8
    full = ff = None
    for seed in range(4000):                             # one interval: its bit count decides the padding
        x = J.image(side, side, "noise", seed=seed)
        bits = []
        data = J.encode_levels(J.levels(x, 100, sub), side, side, 100, sub, bit_counts=bits)
        if full is None and bits[0] % 8 == 0:
            full = (x, data)
        if ff is None and data.endswith(b"\xff\x00\xff\xd9"):
            ff = (x, data)
        if full and ff:
            break
    assert full and ff
    for x, data in (full, ff):
        _check_file(data, x, 100, sub)


# ---- AVI ----------------------------------------------------------------------------------------------------------------------------------
def walk_riff(data: bytes):
    """An independent reader: -> (chunks as {path: [(payload offset, size)]}, with every size field and the even padding checked)."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    found = {}

    def walk(pos, end, path):
        while pos < end:
            fourcc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
            assert pos + 8 + size <= end, (path, fourcc)
            if fourcc == b"LIST":
                walk(pos + 12, pos + 8 + size, path + "/" + data[pos + 8:pos + 12].decode())
                found.setdefault(path + "/LIST:" + data[pos + 8:pos + 12].decode(), []).append((pos + 8, size))
            else:
                found.setdefault(path + "/" + fourcc.decode(), []).append((pos + 8, size))
            pos += 8 + size + (size & 1)
        assert pos == end, path
    walk(12, len(data), "")
    return found


def check_avi(data: bytes, files, width, height, fps):
    """The structure of an AVI file holding ``files`` (the standalone JPEG files, in order)."""
    c = walk_riff(data)
    (a, n), = c["/hdrl/avih"]
    avih = struct.unpack("<14I", data[a:a + n])
    assert n == 56 and avih[0] == 1000000 // fps and avih[3] & 0x10 and avih[4] == len(files) and avih[6] == 1 and avih[8:10] == (width, height)
    (a, n), = c["/hdrl/strl/strh"]
    strh = struct.unpack("<4s4sIHHIIIIIIII4H", data[a:a + n])
    assert strh[0] == b"vids" and strh[1] == b"MJPG" and (strh[6], strh[7]) == (1, fps) and strh[9] == len(files) and strh[-2:] == (width, height)
    (a, n), = c["/hdrl/strl/strf"]
    strf = struct.unpack("<IiiHH4sIiiII", data[a:a + n])
    assert strf[:6] == (40, width, height, 1, 24, b"MJPG")
    frames = c["/movi/00dc"]
    assert len(frames) == len(files)
    (movi_at, _), = c["/LIST:movi"]                      # offset of the 'movi' fourcc
    (a, n), = c["/idx1"]
    assert n == 16 * len(files)
    for i, ((off, size), want) in enumerate(zip(frames, files)):
        assert data[off:off + size] == want
        assert _pil(data[off:off + size]).size == (width, height)
        cid, flags, ioff, isize = struct.unpack("<4sIII", data[a + 16 * i:a + 16 * i + 16])
        assert cid == b"00dc" and flags & 0x10 and isize == size and movi_at + ioff + 8 == off


def test_avi_structure_and_the_4gib_guard(tmp_path):
    from dove_amd import avi
    files = [J.encode(J.image(17, 33, "smooth", seed=i), 50 + i, "444") for i in range(5)]
    assert any(len(f) & 1 for f in files) and any(not len(f) & 1 for f in files)      # both paddings occur
    path = tmp_path / "a.avi"
    with avi.MjpegAviWriter(str(path), 33, 17, 24) as w:
        for f in files:
            w.write(f)
    check_avi(path.read_bytes(), files, 33, 17, 24)
    with pytest.raises(avi.AviError, match="seekable"):
        avi.MjpegAviWriter("-", 33, 17, 24)
    w = avi.MjpegAviWriter(str(tmp_path / "b.avi"), 33, 17, 24)
    w.write(files[0])
    w._movi = avi.RIFF_LIMIT - 400                       # as if almost 4 GiB of frames had been written
    with pytest.raises(avi.AviError, match="4 GiB"):
        w.write(files[1])
    w._movi = 4 + 8 + len(files[0]) + (len(files[0]) & 1)
    w.close()
    check_avi((tmp_path / "b.avi").read_bytes(), files[:1], 33, 17, 24)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_encoder_arguments_are_validated_before_any_device_call():
    import ctypes as C

    from dove_amd import lib as L
    lib = L.load()
    v = L.ImageView()
    v.data, v.dtype, v.sn, v.sc, v.sh, v.sw = 1, L.U8, 48, 1, 12, 3
    q = (C.c_int * 1)(95)

    def call(n, h, w, quality, sub, ws_bytes=0):
        return lib.dove_jpeg_encode(C.byref(v), n, h, w, quality, sub, None, ws_bytes, None, None, None)
    assert call(1, 4, 4, (C.c_int * 1)(0), 0) == -1 and b"quality" in lib.dove_last_error()
    assert call(1, 4, 4, (C.c_int * 1)(101), 1) == -1 and b"quality" in lib.dove_last_error()
    assert call(1, 4, 4, q, 2) == -1 and b"subsampling" in lib.dove_last_error()
    assert call(0, 4, 4, q, 0) == -1 and b"shape" in lib.dove_last_error()
    assert call(1, 4, 65536, q, 0) == -1 and b"65535" in lib.dove_last_error()
    assert call(1, 4, 4, q, 0, ws_bytes=lib.dove_jpeg_workspace_bytes(1, 4, 4, 0) - 1) == -1 and b"workspace" in lib.dove_last_error()
    R = lib.dove_jpeg_restart_mcus()
    assert R == J.RESTART_MCUS
    # 17 x 33: 2 x 3 MCUs of 6 blocks (4:2:0), 3 x 5 MCUs of 3 blocks (4:4:4); 629 header bytes, 416 per block, 2 per interval
    assert lib.dove_jpeg_bound(17, 33, 0) == 629 + 416 * 36 + 2 * 1 and lib.dove_jpeg_bound(17, 33, 1) == 629 + 416 * 45 + 2 * 2
    assert lib.dove_jpeg_bound(2880, 5120, 0) == 629 + 416 * 180 * 320 * 6 + 2 * 7200
    assert lib.dove_jpeg_bound(0, 8, 0) == 0 and lib.dove_jpeg_bound(8, 8, 2) == 0 and lib.dove_jpeg_bound(8, 65536, 1) == 0
    slot420, slot444 = 2 * 9960 + 16, -(-(2 * 4980 + 16) // 16) * 16
    assert lib.dove_jpeg_workspace_bytes(1, 17, 33, 0) == 256 + 256 + 1 * slot420
    assert lib.dove_jpeg_workspace_bytes(3, 17, 33, 1) == 256 + 256 + 6 * slot444
    assert lib.dove_jpeg_workspace_bytes(0, 17, 33, 0) == 0
    assert len(J.header(17, 33, 50, "420", R)) == 629


def test_python_surfaces_without_a_device():
    from dove_amd import cli, jpeg, ops
    assert ops.jpeg_subsampling_code("420") == 0 and ops.jpeg_subsampling_code("444") == 1
    with pytest.raises(ValueError):
        ops.jpeg_subsampling_code("422")
    assert jpeg.group_frames(720, 1280, "420") >= 1 and jpeg.group_frames(720, 1280, "444", budget_bytes=1) == 1
    with pytest.raises(ValueError):
        jpeg._rgb_nchw(torch.zeros(2, 5, 6, dtype=torch.uint8), None)                  # grey
    p = cli.build_parser()
    a = p.parse_args(["--input_dir", "x", "--avi_save", "--jpeg_quality", "80"])
    assert a.avi_save and not a.jpg_save and a.jpeg_quality == 80 and p.parse_args(["--input_dir", "x"]).jpeg_quality == 95
    assert cli.jpeg_subsampling("yuv444p") == "444" and cli.jpeg_subsampling("yuv420p") == "420"
    with pytest.raises(ValueError, match="4:2:2"):
        cli.jpeg_subsampling("yuv422p")
    for flags in (["--jpg_save", "--avi_save"], ["--jpg_save", "--png_save"], ["--avi_save", "--y4m_save"]):
        with pytest.raises(ValueError, match="choose one output form"):
            cli.main(["--input_dir", "x", "--random_init"] + flags)
    with pytest.raises(ValueError, match="yuv422p"):
        cli.main(["--input_dir", "x", "--random_init", "--jpg_save", "--save_format", "yuv422p"])
