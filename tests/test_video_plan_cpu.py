"""The library's host planner (csrc/video.hip: dove_plan_*, dove_chunk_planner_*) against the golden vectors of the reference's own
functions and, exhaustively, against dove_amd.tiling / dove_amd.stream.ChunkPlanner.  Pure host code: runs without a GPU."""
import ctypes as C
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

from dove_amd import lib as L
from dove_amd import stream, tiling
from dove_amd import videoplan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAMES = range(1, 131)
CHUNK_LENS = (0, 9, 17, 25, 33)
OVERLAPS_T = (0, 4, 8, 16)
SIZES = ((64, 96), (80, 112), (128, 192), (144, 176), (160, 208))          # H x W around multiples of 16 (what the x16 padding leaves)
# (tile, overlap): one tile, the stream tests' 3 x 2, a non-square one, a tile larger than some frames, and tiles not larger than the overlap
TILES = (((0, 0), (32, 32)), ((64, 96), (32, 32)), ((48, 80), (16, 32)), ((96, 96), (0, 16)), ((32, 64), (32, 32)), ((64, 16), (32, 32)))
LACK, DOUBLE = "Error: Lack of write in region !!!", "Error: Write count > 1 in region !!!"


def outcome(fn, *a):
    """(result, None) or (None, (exception type, message)): both planners must agree on either."""
    try:
        return fn(*a), None
    except (ValueError, RuntimeError) as e:
        return None, (type(e), str(e))


@pytest.fixture(scope="module")
def gold(golden_dir):
    with open(os.path.join(golden_dir, "tiler_golden.json")) as f:
        return json.load(f)


def test_golden_vectors_through_the_c_planner(gold):
    assert len(gold["temporal"]) >= 10 and len(gold["spatial"]) >= 10 and len(gold["region"]) >= 5
    for c in gold["temporal"]:
        if "raises" in c:
            with pytest.raises(ValueError, match=c["msg"]):
                P.make_temporal_chunks(c["F"], c["chunk_len"], c["overlap_t"])
        else:
            assert [list(x) for x in P.make_temporal_chunks(c["F"], c["chunk_len"], c["overlap_t"])] == c["out"], c
    for c in gold["spatial"]:
        if "raises" in c:
            with pytest.raises(ValueError, match=c["msg"]):
                P.make_spatial_tiles(c["H"], c["W"], c["tile"], c["overlap"])
        else:
            assert [list(x) for x in P.make_spatial_tiles(c["H"], c["W"], c["tile"], c["overlap"])] == c["out"], c
    for plan, cov in zip(gold["region"], gold["coverage"]):
        # the arguments tests/test_tiling.py hands dove_amd.tiling.plan for these vectors
        items = P.plan(plan["shape"], plan["chunk_len"], plan["overlap_t"] or 8, plan["tile"], plan["overlap_hw"] if plan["tile"] != [0, 0] else (32, 32))
        assert len(items) == len(plan["regions"])
        for (args, reg), g in zip(items, plan["regions"]):
            assert list(args) == g["args"] and reg == g["out"]
            ov_t = plan["overlap_t"] if plan["chunk_len"] else 0
            ov_hw = plan["overlap_hw"] if plan["tile"] != [0, 0] else (0, 0)
            assert P.get_valid_tile_region(*args, plan["shape"], ov_t, ov_hw[0], ov_hw[1]) == g["out"]
        assert cov["min"] == cov["max"] == 1
        _, _, F, H, W = plan["shape"]
        P.check_coverage([P.out_box(r) for _, r in items], F, H, W)


def test_padding_and_output_size_agree_with_tiling():
    for F, H, W in itertools.product((1, 2, 8, 9, 10, 33, 100, 129), (16, 17, 31, 32, 178, 180, 720), (16, 20, 316, 320, 1279)):
        assert P.match_padding(F, H, W) == tiling.match_padding(F, H, W)
        for up in (1, 2, 4):
            assert P.output_size(H, W, up) == stream.output_size(H, W, up)
    assert P.match_padding(8, 178, 316) == (1, 14, 4) and P.output_size(180, 320, 4) == (720, 1280)


def test_plans_agree_with_tiling_exhaustively():
    """Every (F, chunk_len, overlap_t, H x W, tile) of the ranges: the same pieces and regions or the same error, and the host coverage
    check accepts what tiling.check_coverage accepts.

    The reference's check runs on a per-voxel count tensor; one such tensor per case (130 x 160 x 208 voxels, 78 000 cases) is out of
    reach, and not needed: a plan is a product, every chunk with every tile, so the count at (t, y, x) is ct[t] * cs[y, x] with ct the
    number of chunks whose kept frames hold t and cs the number of tiles whose kept pixels hold (y, x).  A product of non-negative integers
    is 1 everywhere exactly when both factors are, 0 somewhere exactly when a factor is (both axes being non-empty), so
    tiling.check_coverage is run on ct and on cs - built with tiling.stitch - and its verdict on the product follows."""
    def spatial_verdict(H, W, tile, ov):
        if outcome(tiling.make_spatial_tiles, H, W, tile, ov if tile != (0, 0) else (0, 0))[1]:
            return None
        wc = torch.zeros(1, 1, 1, H, W, dtype=torch.int32)
        for (_, _, h0, h1, w0, w1), reg in tiling.plan((1, 3, 1, H, W), 0, 0, tile, ov):
            assert 0 <= h0 < h1 <= H and 0 <= w0 < w1 <= W
            tiling.stitch(torch.zeros(1, 1, 1, H, W), wc, torch.zeros(1, 1, 1, h1 - h0, w1 - w0), reg)
        return outcome(tiling.check_coverage, wc)[1]

    def temporal_verdict(F, n, ov):
        chunks, err = outcome(tiling.make_temporal_chunks, F, n, ov if n else 0)
        if err:
            return None
        wc = torch.zeros(1, 1, F, 1, 1, dtype=torch.int32)
        for (t0, t1, *_), reg in tiling.plan((1, 3, F, 1, 1), n, ov, (0, 0)):
            tiling.stitch(torch.zeros(1, 1, F, 1, 1), wc, torch.zeros(1, 1, t1 - t0, 1, 1), reg)
        return outcome(tiling.check_coverage, wc)[1]

    sv = {(s, t): spatial_verdict(*s, *t) for s in SIZES for t in TILES}
    tv = {(F, n, ov): temporal_verdict(F, n, ov) for F in FRAMES for n in CHUNK_LENS for ov in OVERLAPS_T}
    cases = errors = rejected = 0
    for F, n, ov in itertools.product(FRAMES, CHUNK_LENS, OVERLAPS_T):
        assert outcome(P.make_temporal_chunks, F, n, ov) == outcome(tiling.make_temporal_chunks, F, n, ov)
        for (H, W), (tile, ovhw) in itertools.product(SIZES, TILES):
            shape = (1, 3, F, H, W)
            want, werr = outcome(tiling.plan, shape, n, ov, tile, ovhw)
            got, gerr = outcome(P.plan, shape, n, ov, tile, ovhw)
            assert gerr == werr and got == want, (shape, n, ov, tile, ovhw, gerr, werr)
            cases += 1
            if werr:
                errors += 1
                continue
            t_err, s_err = tv[(F, n, ov)], sv[((H, W), (tile, ovhw))]
            lack = any(e and e[1] == LACK for e in (t_err, s_err))
            expect = None if not (t_err or s_err) else (RuntimeError, LACK if lack else DOUBLE)
            verdict = outcome(P.check_coverage, [P.out_box(r) for _, r in got], F, H, W)[1]
            assert verdict == expect, (shape, n, ov, tile, ovhw, verdict, expect)
            rejected += verdict is not None
    assert cases == len(FRAMES) * len(CHUNK_LENS) * len(OVERLAPS_T) * len(SIZES) * len(TILES)
    assert errors > 0 and rejected > 0                             # both kinds of case were met: errors of the planner, and the no-chunk hole


def test_spatial_tiles_agree_on_their_own():
    for (H, W), (tile, ov) in itertools.product(SIZES + ((1080, 1920), (720, 1280), (17, 33)), TILES + (((544, 960), (32, 32)), ((0, 64), (8, 8)))):
        assert outcome(P.make_spatial_tiles, H, W, tile, ov) == outcome(tiling.make_spatial_tiles, H, W, tile, ov), (H, W, tile, ov)


def test_both_planner_errors():
    with pytest.raises(ValueError, match="chunk_len must be greater than overlap"):
        P.make_temporal_chunks(33, 8, 8)
    with pytest.raises(ValueError, match="Tile size must be greater than overlap"):
        P.make_spatial_tiles(128, 192, (32, 64), (32, 32))
    with pytest.raises(ValueError, match="chunk_len must be greater than overlap"):
        P.ChunkPlanner(9, 16)


def drive(planner_cls, n, ov, F, block, eager):
    """Feed a planner the way stream.sr_stream does: frames arrive in blocks until need() is met; the end of the stream is known with a
    short block (``eager``: as soon as the last frame is in, as a host that knows the length would).  Returns the trace of every need() and
    next()."""
    pl, err = outcome(planner_cls, n, ov)
    if err:
        return [("init", err)]
    trace, known, eof = [], 0, False
    for _ in range(F + 4):
        need = pl.need()
        trace.append(("need", need))
        while not eof and (need is None or known < need):
            got = min(block, F - known)
            known += got
            eof = got < block or (eager and known == F)
        chunk, err = outcome(pl.next, known, eof)
        trace.append(("next", known, eof, chunk, err and err[0]))
        if err or chunk is None or chunk[2]:
            break
    return trace


def test_incremental_planner_agrees_with_stream_chunk_planner():
    """Frames arrive in blocks of 1, 7 and chunk_len - overlap_t, for every clip length of the range - so the end of the stream falls on
    every position a chunk, an overlap or a merged tail can give it - and is learnt either with a short read or with the last frame."""
    runs = 0
    for n, ov in itertools.product(CHUNK_LENS, OVERLAPS_T):
        for F in FRAMES:
            for block in sorted({1, 7, max(n - ov, 1)}):
                for eager in (False, True):
                    want = drive(stream.ChunkPlanner, n, ov, F, block, eager)
                    got = drive(P.ChunkPlanner, n, ov, F, block, eager)
                    assert got == want, (n, ov, F, block, eager)
                    runs += 1
            # and the chunks of a known length are make_temporal_chunks's
            if n == 0 or n > ov:
                pl, chunks = P.ChunkPlanner(n, ov), []
                while (c := pl.next(F, True)) is not None:
                    chunks.append(c[:2])
                    if c[2]:
                        break
                assert chunks == tiling.make_temporal_chunks(F, n, ov if n else 0)
    assert runs > 10000
    pl = P.ChunkPlanner(17, 8)
    with pytest.raises(RuntimeError, match="needs 26 known frames"):
        pl.next(25, False)
    with pytest.raises(RuntimeError, match="needs the end of the stream"):
        P.ChunkPlanner(0, 8).next(5, False)


def test_host_coverage_check_rejects_holes_and_double_writes():
    P.check_coverage([(0, 4, 0, 8, 0, 8), (4, 9, 0, 8, 0, 8)], 9, 8, 8)
    with pytest.raises(RuntimeError, match=re.escape(LACK)):
        P.check_coverage([], 9, 8, 8)                                            # the "no chunk" case: nothing is written
    assert tiling.make_temporal_chunks(8, 17, 8) == [] and P.plan((1, 3, 8, 32, 48), 17, 8) == []
    with pytest.raises(RuntimeError, match=re.escape(LACK)):
        P.check_coverage([(0, 4, 0, 8, 0, 8), (5, 9, 0, 8, 0, 8)], 9, 8, 8)      # frame 4 is never written
    with pytest.raises(RuntimeError, match=re.escape(DOUBLE)):
        P.check_coverage([(0, 5, 0, 8, 0, 8), (4, 9, 0, 8, 0, 8)], 9, 8, 8)      # frame 4 twice
    with pytest.raises(RuntimeError, match=re.escape(DOUBLE)):
        P.check_coverage([(0, 9, 0, 8, 0, 5), (0, 9, 0, 8, 3, 8), (0, 9, 2, 4, 4, 5)], 9, 8, 8)
    with pytest.raises(RuntimeError, match=re.escape(LACK)):                     # a hole AND a double write: the reference tests the hole first
        P.check_coverage([(0, 5, 0, 8, 0, 8), (4, 8, 0, 8, 0, 8)], 9, 8, 8)
    with pytest.raises(RuntimeError, match="outside the region"):
        P.check_coverage([(0, 10, 0, 8, 0, 8)], 9, 8, 8)
    # random box lists against a per-voxel count
    g = np.random.default_rng(0)
    seen = set()
    for _ in range(300):
        F, H, W = (int(v) for v in g.integers(1, 7, size=3))
        boxes = []
        for _ in range(int(g.integers(0, 5))):
            lo = [int(g.integers(0, d)) for d in (F, H, W)]
            hi = [int(g.integers(l + 1, d + 1)) for l, d in zip(lo, (F, H, W))]
            boxes.append((lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))
        if g.integers(0, 3) == 0:                                                # an exact cover: two halves along one axis
            cut = int(g.integers(0, F + 1))
            boxes = [(0, cut, 0, H, 0, W), (cut, F, 0, H, 0, W)]
        wc = torch.zeros(1, 1, F, H, W, dtype=torch.int32)
        for b in boxes:
            wc[:, :, b[0]:b[1], b[2]:b[3], b[4]:b[5]] += 1
        want = outcome(tiling.check_coverage, wc)[1]
        assert outcome(P.check_coverage, boxes, F, H, W)[1] == want, (boxes, F, H, W)
        seen.add(want and want[1])
    assert seen == {None, LACK, DOUBLE}


def test_abi_version_and_new_symbols():
    with open(os.path.join(ROOT, "include", "dove_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+DOVE_ABI_VERSION\s+15\b", header)
    lib = L.load()
    assert lib.dove_abi_version() == 15
    new = ["dove_plan_padding", "dove_plan_output_size", "dove_plan_temporal_chunks", "dove_plan_spatial_tiles", "dove_plan_valid_region",
           "dove_plan_pieces", "dove_plan_check_coverage", "dove_chunk_planner_create", "dove_chunk_planner_need", "dove_chunk_planner_next",
           "dove_chunk_planner_destroy", "dove_philox_u32", "dove_randn", "dove_stitch", "dove_video_workspace_bytes", "dove_video_open",
           "dove_video_info", "dove_video_push", "dove_video_end_of_input", "dove_video_need", "dove_video_step", "dove_video_close"]
    bound = set(L.SIGNATURES) | set(L.PLAIN)
    for name in new:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/dove_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound, f"{name} is not bound in dove_amd/lib.py"
    # the parameter struct of the binding is the header's, field for field in size
    assert C.sizeof(L.VideoParams) % 8 == 0 and L.VideoParams().struct_size == C.sizeof(L.VideoParams)
    bad = L.VideoParams()
    bad.struct_size -= 8
    assert lib.dove_video_workspace_bytes(None, C.byref(bad)) == 0               # no context: refused before anything is read


def test_session_arguments_are_checked_without_a_gpu():
    lib = L.load()
    h = C.c_void_p()
    assert lib.dove_video_open(None, C.byref(L.VideoParams()), C.byref(h)) == -1 and b"null pointer" in lib.dove_last_error()
    n = C.c_int()
    assert lib.dove_video_step(None, None, 0, C.byref(n), None, None) == -1
    assert lib.dove_randn(None, 7, 4, 0, 0, 0, None) == -1 and b"dtype" in lib.dove_last_error()
    assert lib.dove_randn(None, L.F32, 0, 0, 0, 0, None) == 0                    # nothing to draw: no launch
    box = (C.c_int * 6)(0, 2, 0, 4, 0, 9)
    assert lib.dove_stitch(1, 2, 4, 8, box, 1, 2, 4, 8, 0, 0, 0, None) == -1 and b"does not fit inside" in lib.dove_last_error()
