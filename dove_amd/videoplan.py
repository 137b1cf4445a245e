"""The library's host planner (include/dove_hip.h ``dove_plan_*`` / ``dove_chunk_planner_*``; csrc/video.hip) behind the signatures of
``dove_amd.tiling`` and ``dove_amd.stream.ChunkPlanner``: what a C host plans a whole video with.  Pure host code - no GPU is touched.
The Python pipeline keeps using ``tiling``; this module exists so that the two can be held against each other
(tests/test_video_plan_cpu.py) and for hosts that want the library's own answer."""
from __future__ import annotations

import ctypes as C

from . import lib as L

REGION_KEYS = tuple(f"{kind}_{axis}_{end}" for kind in ("valid", "out") for axis in "thw" for end in ("start", "end"))


def _fail(what: str):
    msg = L.load().dove_last_error().decode()
    # the planner's own messages are the reference's texts, raised as dove_amd.tiling raises them
    if msg.startswith("Error:"):
        raise RuntimeError(msg)
    if "must be greater than overlap" in msg:
        raise ValueError(msg)
    raise RuntimeError(f"{what} failed: {msg}")


def match_padding(F: int, H: int, W: int):
    f, h, w = C.c_int(), C.c_int(), C.c_int()
    if L.load().dove_plan_padding(F, H, W, C.byref(f), C.byref(h), C.byref(w)) != 0:
        _fail("dove_plan_padding")
    return f.value, h.value, w.value


def output_size(h: int, w: int, upscale: int):
    ho, wo = C.c_int(), C.c_int()
    if L.load().dove_plan_output_size(h, w, upscale, C.byref(ho), C.byref(wo)) != 0:
        _fail("dove_plan_output_size")
    return ho.value, wo.value


def _filled(call, width: int, what: str):
    """Count, allocate, fill: ``call(buffer or None, cap)`` returns the number of entries."""
    n = call(None, 0)
    if n < 0:
        _fail(what)
    buf = (C.c_int * max(width * n, 1))()
    if call(buf, n) != n:
        _fail(what)
    return [tuple(buf[width * i:width * (i + 1)]) for i in range(n)]


def make_temporal_chunks(F: int, chunk_len: int, overlap_t: int = 8):
    return _filled(lambda b, cap: L.load().dove_plan_temporal_chunks(F, chunk_len, overlap_t, b, cap), 2, "dove_plan_temporal_chunks")


def make_spatial_tiles(H: int, W: int, tile_size_hw, overlap_hw=(32, 32)):
    return _filled(lambda b, cap: L.load().dove_plan_spatial_tiles(H, W, tile_size_hw[0], tile_size_hw[1], overlap_hw[0], overlap_hw[1], b, cap),
                   4, "dove_plan_spatial_tiles")


def _region(valid, out) -> dict:
    return dict(zip(REGION_KEYS, tuple(valid) + tuple(out)))


def get_valid_tile_region(t0, t1, h0, h1, w0, w1, video_shape, overlap_t, overlap_h, overlap_w) -> dict:
    _, _, F, H, W = video_shape
    piece, valid, out = (C.c_int * 6)(t0, t1, h0, h1, w0, w1), (C.c_int * 6)(), (C.c_int * 6)()
    if L.load().dove_plan_valid_region(piece, F, H, W, overlap_t, overlap_h, overlap_w, valid, out) != 0:
        _fail("dove_plan_valid_region")
    return _region(valid, out)


def plan(video_shape, chunk_len=0, overlap_t=8, tile_size_hw=(0, 0), overlap_hw=(32, 32)):
    """``tiling.plan``: [((t0, t1, h0, h1, w0, w1), region dict)] chunk-major, tile-minor."""
    _, _, F, H, W = video_shape
    args = (F, H, W, chunk_len, overlap_t, tile_size_hw[0], tile_size_hw[1], overlap_hw[0], overlap_hw[1])
    lib = L.load()
    n = lib.dove_plan_pieces(*args, None, None, None, 0)
    if n < 0:
        _fail("dove_plan_pieces")
    pieces, valid, out = ((C.c_int * max(6 * n, 1))() for _ in range(3))
    if lib.dove_plan_pieces(*args, pieces, valid, out, n) != n:
        _fail("dove_plan_pieces")
    return [(tuple(pieces[6 * i:6 * i + 6]), _region(valid[6 * i:6 * i + 6], out[6 * i:6 * i + 6])) for i in range(n)]


def check_coverage(boxes, F: int, H: int, W: int):
    """``boxes``: (t0, t1, h0, h1, w0, w1) out-boxes.  Raises RuntimeError with the reference's message unless they cover F x H x W once."""
    flat = [int(v) for b in boxes for v in b]
    buf = (C.c_int * max(len(flat), 1))(*flat)
    if L.load().dove_plan_check_coverage(buf, len(flat) // 6, F, H, W) != 0:
        _fail("dove_plan_check_coverage")


def out_box(region: dict):
    return tuple(region[k] for k in REGION_KEYS[6:])


class ChunkPlanner:
    """``stream.ChunkPlanner`` on the library's planner."""

    def __init__(self, chunk_len: int, overlap_t: int = 8):
        self._h = C.c_void_p()
        if L.load().dove_chunk_planner_create(chunk_len, overlap_t, C.byref(self._h)) != 0:
            _fail("dove_chunk_planner_create")

    def __del__(self):
        try:
            if self._h:
                L.load().dove_chunk_planner_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def need(self):
        n = int(L.load().dove_chunk_planner_need(self._h))
        return None if n < 0 else n

    def next(self, known: int, eof: bool):
        t0, t1, last = C.c_longlong(), C.c_longlong(), C.c_int()
        rc = L.load().dove_chunk_planner_next(self._h, known, int(eof), C.byref(t0), C.byref(t1), C.byref(last))
        if rc < 0:
            _fail("dove_chunk_planner_next")
        return (t0.value, t1.value, bool(last.value)) if rc else None
