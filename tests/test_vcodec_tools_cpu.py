"""The codec round trip's H.264 tool set without a device: tests/vcodec_tools_ref.py (the definition csrc/vcodec.hip reproduces byte for
byte) against the properties intra prediction, quarter-sample motion and the deblocking filter must have, the branch coverage of the clips
the device test compares, the Degrader's ``sim-h264`` option, and the host-side refusals (they come before any HIP call)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import vcodec_ref as R
import vcodec_tools_ref as T
from dove_amd import degrade as D
from dove_amd import ops
from test_vcodec_cpu import texture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "tests", "golden", "degradation_config.yaml")


def bilinear_window(Tx, h, w, y_off, x_off):
    """The h x w window of the texture at a fractional offset."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    y, x = yy + y_off, xx + x_off
    y0, x0 = np.floor(y).astype(int), np.floor(x).astype(int)
    fy, fx = (y - y0)[..., None], (x - x0)[..., None]
    return (1 - fy) * (1 - fx) * Tx[y0, x0] + (1 - fy) * fx * Tx[y0, x0 + 1] + fy * (1 - fx) * Tx[y0 + 1, x0] + fy * fx * Tx[y0 + 1, x0 + 1]


def tools_clip(n, h, w, seed):
    """A texture sliding by (1.25, 2.75) samples per frame plus noise; on frames of two macroblock rows also a band that is constant
    along y (vertical prediction) and a still strip that is constant along x (horizontal prediction, vectors that differ from the moving
    part's with no residual to code)."""
    Tx = texture(h + 24, w + 24, seed)
    fr = []
    for t in range(n):
        f = (bilinear_window(Tx, h, w, 4 + 1.25 * t, 4 + 2.75 * t) - 128) * 1.5 + 128
        if h >= 32:
            f[16:32, :w // 2] = Tx[5, :w // 2][None] * 1.3 - 30
            f[:, w - 12:] = Tx[:h, 7][:, None] * 0.9 + 10
        fr.append(f)
    fr = np.stack(fr) + np.random.default_rng(seed).normal(0, 1.5, (n, h, w, 3))
    return np.ascontiguousarray(fr, dtype=np.float32)


# The clips of the device test (tests/test_vcodec_tools_gpu.py): name -> (frames, height, width, gop, the bitrate that lands between 16 and 50)
SHAPES = {"3x4 macroblocks, groups of 3 and 2": (5, 40, 56, 3, 4000), "odd sizes": (4, 33, 47, 4, 3000), "one macroblock": (2, 16, 16, 2, 1500)}
BITRATES = ("QP 51", "mid", "QP 0")
TOOLSETS = (0, T.INTRA16, T.QPEL, T.DEBLOCK, T.ALL_TOOLS)
SEED = 1


def clip_of(shape):
    n, h, w, _, _ = SHAPES[shape]
    return tools_clip(n, h, w, SEED + h)


@functools.lru_cache(maxsize=None)
def reference(shape, rate, tools):
    """(frames, QPs, bits, branch counters) of the definition, computed once per case and shared by the tests of both files."""
    gop, mid = SHAPES[shape][3:]
    out = T.vcodec_roundtrip(clip_of(shape), {"QP 51": 0, "mid": mid, "QP 0": 10 ** 7}[rate], gop, tools, want_stats=True)
    for a in out[:3]:
        a.setflags(write=False)
    return out


# ---- tools = 0 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_no_tools_is_the_plain_codec(shape):
    gop, mid = SHAPES[shape][3:]
    for rate, bitrate in (("QP 51", 0), ("mid", mid), ("QP 0", 10 ** 7)):
        want, want_qp, want_bits = R.vcodec_roundtrip(clip_of(shape), bitrate, gop, want_stats=True)
        got, qp, bits, _ = reference(shape, rate, 0)
        assert np.array_equal(got, want) and qp.tolist() == want_qp.tolist() and bits.tolist() == want_bits.tolist()
        assert (rate == "QP 51" and set(qp) == {51}) or (rate == "QP 0" and set(qp) == {0}) or (rate == "mid" and all(16 <= q < 51 for q in qp))


# ---- INTRA16 ----------------------------------------------------------------------------------------------------------------------
def striped_planes(axis):
    """(Y, Cb, Cr) of 48 x 64 that are constant along ``axis``, in runs of four samples across it: every 4x4 block is flat, and a flat
    block is exact at QP 0 (its DC level times 10 is within 32 of 64 times its value), so a neighbour row / column is the source's."""
    rng = np.random.default_rng(4)
    out = []
    for ph, pw in ((48, 64), (24, 32), (24, 32)):
        length = pw if axis == 0 else ph
        line = np.repeat(rng.integers(2, 12, length // 4) * 20 + rng.integers(0, 9, length // 4), 4).astype(np.int64)
        out.append(np.tile(line, (ph, 1)) if axis == 0 else np.tile(line[:, None], (1, pw)))
    return out


def test_a_frame_constant_along_y_is_predicted_vertically():
    cur = striped_planes(0)
    rec, bits, lm, cm, nzl = T.intra_frame(cur, 0)
    assert all(np.array_equal(r, c) for r, c in zip(rec, cur))
    assert (lm[1:] == 0).all() and (cm[1:] == 2).all()                            # V is luma index 0 and chroma index 2
    assert not nzl[1:].any() and nzl[0].all()                                     # all-zero levels below the first macroblock row


def test_a_frame_constant_along_x_is_predicted_horizontally():
    cur = striped_planes(1)
    rec, bits, lm, cm, nzl = T.intra_frame(cur, 0)
    assert all(np.array_equal(r, c) for r, c in zip(rec, cur))
    assert (lm[:, 1:] == 1).all() and (cm[:, 1:] == 1).all()
    assert not nzl[:, 1:].any() and nzl[:, 0].all()


def test_a_flat_frame_is_predicted_as_its_dc_and_the_first_macroblock_as_128():
    """On a flat frame V, H and DC are the same prediction, the frame's value, with SAD 0: the winner is the cheapest index that exists.
    For chroma that is DC (index 0) in every macroblock.  For luma the stated cost, SAD + LAMBDA ue_len(index) with ties to the lower
    index, gives V (index 0) under a row above, H beside a column to the left only, and DC where it is the only candidate: macroblock
    (0, 0), whose DC is 128."""
    for value in (128, 141):
        cur = [np.full(s, value, dtype=np.int64) for s in ((48, 64), (24, 32), (24, 32))]
        rec, bits, lm, cm, nzl = T.intra_frame(cur, 0)
        assert all((r == value).all() for r in rec)
        assert (cm == 0).all()
        assert lm[0, 0] == 2 and (lm[0, 1:] == 1).all() and (lm[1:] == 0).all()
        assert not nzl.reshape(-1)[1:].any()                                      # every other macroblock is predicted as the value
        assert (nzl[0, 0] == 0) == (value == 128)                                 # macroblock (0, 0) is predicted as 128
    none = T._candidates(np.zeros((32, 32), dtype=np.int64), 0, 0, 16, (0, 1, 2))
    assert list(none) == [2] and (none[2][0] == 128).all() and none[2][1] == "none"
    rec = np.arange(32 * 32).reshape(32, 32) % 251
    both, top, left = (T._candidates(rec, r, c, 16, (0, 1, 2))[2] for r, c in ((1, 1), (1, 0), (0, 1)))
    assert both[0][0, 0] == (rec[15, 16:32].sum() + rec[16:32, 15].sum() + 16) >> 5 and both[1] == "both"
    assert top[0][0, 0] == (rec[15, 0:16].sum() + 8) >> 4 and left[0][0, 0] == (rec[0:16, 15].sum() + 8) >> 4 and top[1] == left[1] == "one"
    cb = T._candidates(rec, 1, 1, 8, (2, 1, 0))
    assert cb[0][0][0, 0] == (rec[7, 8:16].sum() + rec[8:16, 7].sum() + 8) >> 4 and (cb[2][0][3] == rec[7, 8:16]).all() and (cb[1][0][:, 3] == rec[8:16, 7]).all()
    assert T._candidates(rec, 0, 1, 8, (2, 1, 0))[0][0][0, 0] == (rec[0:8, 7].sum() + 4) >> 3


def test_intra_bits_count_both_mode_indices():
    # a flat 128 frame of 2 x 2 macroblocks: 24 empty blocks each; luma DC (3 bits), H (3), V (1), V (1); chroma DC (1 bit) in all four
    cur = [np.full(s, 128, dtype=np.int64) for s in ((32, 32), (16, 16), (16, 16))]
    assert T.intra_frame(cur, 30)[1] == 4 * 24 + (3 + 3 + 1 + 1) + 4 * 1
    # constant along y: below the first row 24 empty blocks, ue_len(V = 0) = 1 and ue_len(chroma V = 2) = 3 per macroblock
    cur = striped_planes(0)
    top = [c[:s] for c, s in zip(cur, (16, 8, 8))]
    assert T.intra_frame(cur, 0)[1] - T.intra_frame(top, 0)[1] == 2 * 4 * (24 + 1 + 3)


# ---- QPEL -------------------------------------------------------------------------------------------------------------------------
def test_every_phase_of_a_constant_is_the_constant():
    for value in (0, 77, 255):
        assert (T.luma_phases(np.full((9, 13), value), 3) == value).all()


def test_horizontal_phases_of_a_ramp_are_the_ramp():
    # slope 4: the sample at x + fx / 4 is 4 x + fx + 10 exactly; the half sample needs no rounding and the quarter samples round half up
    ref = np.tile(4 * np.arange(40) + 10, (8, 1))
    PP = T.luma_phases(ref)
    for fx in range(4):
        assert (PP[0, fx][:, 2:-3] == ref[:, 2:-3] + fx).all()
    # slope 1: the half sample is x + 1/2 rounded half up, the quarter samples the rounded means with their neighbours
    ref = np.tile(np.arange(40) + 10, (8, 1))
    PP = T.luma_phases(ref)
    assert (PP[0, 2][:, 2:-3] == ref[:, 2:-3] + 1).all() and (PP[0, 1][:, 2:-3] == ref[:, 2:-3] + 1).all() and (PP[0, 3][:, 2:-3] == ref[:, 2:-3] + 1).all()
    assert (PP[2, 0][2:-3] == ref[2:-3]).all() and (PP[2, 2][2:-3, 2:-3] == ref[2:-3, 2:-3] + 1).all()


@pytest.mark.parametrize("phase", [(0, 2), (2, 0), (2, 2)])
def test_a_half_sample_plane_is_found_at_its_vector_with_sad_0(phase):
    """The second frame is the first frame's own b, h or j plane."""
    ref = texture(48, 64, 11)[..., 0].astype(np.int64)
    cur = T.luma_phases(ref)[phase]
    mv, _ = R.motion_search(cur, ref)
    mvq, sad = T.qpel_refine(cur, ref, mv)
    assert (mvq == np.array(phase)).all() and not sad.any(), (mv.tolist(), mvq.tolist(), sad.tolist())
    pred = T.predict_qpel((ref, ref[::2, ::2], ref[::2, ::2]), mvq)[0]
    assert np.array_equal(pred, cur)


def test_quarter_vectors_read_chroma_in_eighths():
    c = np.arange(24 * 32).reshape(24, 32) % 199
    y = np.zeros((48, 64), dtype=np.int64)
    mvq = np.zeros((3, 4, 2), dtype=np.int64)
    mvq[1, 2] = (5, -11)                            # base (0, -2), fractions yF = 5, xF = 5
    pc = T.predict_qpel((y, c, c), mvq)[1]
    assert np.array_equal(pc[:8], c[:8]) and np.array_equal(pc[8:16, :16], c[8:16, :16])
    A, B, Cc, Dd = c[10, 17], c[10, 18], c[11, 17], c[11, 18]
    assert pc[10, 19] == (3 * 3 * A + 5 * 3 * B + 3 * 5 * Cc + 5 * 5 * Dd + 32) >> 6


# ---- DEBLOCK ----------------------------------------------------------------------------------------------------------------------
def random_planes(seed, smooth):
    rng = np.random.default_rng(seed)
    if smooth:
        t = texture(48, 64, seed).astype(np.int64)
        return [t[..., 0], t[::2, ::2, 1], t[::2, ::2, 2]]
    return [rng.integers(0, 256, s) for s in ((48, 64), (24, 32), (24, 32))]


def test_deblocking_is_the_identity_up_to_qp_15():
    mvq = np.random.default_rng(0).integers(-31, 32, (3, 4, 2))
    nz = np.random.default_rng(1).integers(0, 2, (12, 16)).astype(bool)
    for qp in range(16):
        for planes in (random_planes(qp, True), random_planes(qp, False)):
            for intra in (True, False):
                out = T.deblock_frame(planes, qp, intra, nz, mvq)
                assert all(np.array_equal(o, p) for o, p in zip(out, planes)), (qp, intra)
    out = T.deblock_frame(random_planes(3, True), 16, True)
    assert not np.array_equal(out[0], random_planes(3, True)[0])                  # and no longer at 16


def step_planes(step):
    y = np.full((16, 32), 100, dtype=np.int64)
    y[:, 16:] += step
    return [y, np.full((8, 16), 128, dtype=np.int64), np.full((8, 16), 128, dtype=np.int64)]


def test_a_small_step_across_a_macroblock_edge_changes_three_samples_a_side_and_a_large_one_none():
    qp = 40
    alpha = int(T.ALPHA[qp])
    planes = step_planes(10)                                                      # 10 < (alpha >> 2) + 2: the strong branch on both sides
    out = T.deblock_frame(planes, qp, True)
    changed = out[0] != planes[0]
    assert (changed == (np.abs(np.arange(32) - 15.5) < 3)[None]).all()            # columns 13..18 of every row
    assert (np.diff(out[0][0, 12:20]) >= 0).all() and out[0][0, 12] == 100 and out[0][0, 19] == 110
    for step in (alpha, alpha + 40):
        planes = step_planes(step)
        assert all(np.array_equal(o, p) for o, p in zip(T.deblock_frame(planes, qp, True), planes))
    planes = step_planes(alpha - 1)                                               # the weak bS = 4 branch: p0 and q0 only
    changed = T.deblock_frame(planes, qp, True)[0] != planes[0]
    assert (changed == (np.abs(np.arange(32) - 15.5) < 1)[None]).all()


def test_a_static_p_frame_without_residual_is_returned_unchanged():
    planes = random_planes(5, False)
    for qp in (20, 36, 51):
        for vec in ((0, 0), (-9, 30)):
            mvq = np.tile(np.array(vec), (3, 4, 1))
            bsv, bsh = T.boundary_strengths(False, np.zeros((12, 16), dtype=bool), mvq)
            assert not bsv.any() and not bsh.any()
            out = T.deblock_frame(planes, qp, False, np.zeros((12, 16), dtype=bool), mvq)
            assert all(np.array_equal(o, p) for o, p in zip(out, planes))


def test_boundary_strengths():
    nz = np.zeros((8, 8), dtype=bool)
    nz[1, 2] = True
    mvq = np.zeros((2, 2, 2), dtype=np.int64)
    mvq[0, 1] = (0, 4)                                                            # differs by 4 from its left and lower neighbours
    mvq[1, 0] = (3, -3)                                                           # and this one by less than 4 from (0, 0) above and beside it
    bsv, bsh = T.boundary_strengths(False, nz, mvq)
    assert not bsv[:, 0].any() and not bsh[0].any()                               # picture borders
    assert bsv[1, 2] == bsv[1, 3] == bsh[1, 2] == bsh[2, 2] == 2
    assert (bsv[:4, 4] == 1).all() and not bsv[4:, 4].any()                       # (0, 4) beside (0, 0): 1; (3, -3) beside (0, 0): 0
    assert (bsh[4, 4:] == 1).all() and not bsh[4, :4].any()                       # (0, 4) above (0, 0): 1; (0, 0) above (3, -3): 0
    assert not bsv[0, 1:4].any() and not bsv[0, 5:].any()                         # inside a macroblock without levels
    iv, ih = T.boundary_strengths(True, nz, None)
    assert (iv[:, 4] == 4).all() and (iv[:, [1, 2, 3, 5, 6, 7]] == 3).all() and (ih[4] == 4).all() and (ih[[1, 2, 3, 5, 6, 7]] == 3).all()


def test_chroma_takes_the_luma_edge_at_twice_its_position():
    qp = 40
    y = np.full((32, 32), 100, dtype=np.int64)
    cb = np.full((16, 16), 100, dtype=np.int64)
    cb[:, 8:] += 6
    cr = cb.T.copy()
    nz = np.zeros((8, 8), dtype=bool)
    mvq = np.zeros((2, 2, 2), dtype=np.int64)
    out = T.deblock_frame([y, cb, cr], qp, False, nz, mvq)
    assert np.array_equal(out[1], cb) and np.array_equal(out[2], cr)              # bS 0 everywhere
    nz[0:2, 4] = True                                                             # luma rows 0..7 right of the luma edge at x = 16
    out = T.deblock_frame([y, cb, cr], qp, False, nz, mvq)
    changed = out[1] != cb
    assert changed[:4, 7:9].all() and not changed[:, :7].any() and not changed[:, 9:].any()       # p0 and q0 of chroma rows 0..3
    # then the horizontal pass: the chroma edge at y = 4 takes the luma edge at y = 8, which has levels above it in luma column 16..19 only,
    # and in chroma column 8 the vertical pass left 104 above 106
    assert changed[4, 8] and not changed[4, :8].any() and not changed[5:].any() and out[1][3, 8] == 105


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def test_tables():
    assert T.ALPHA.shape == T.BETA.shape == (52,) and T.TC0.shape == (52, 3)
    assert not T.ALPHA[:16].any() and not T.BETA[:16].any() and not T.TC0[:16].any() and T.ALPHA[16] > 0 and T.BETA[16] > 0
    assert (np.diff(T.ALPHA) >= 0).all() and (np.diff(T.BETA) >= 0).all() and (np.diff(T.TC0, axis=0) >= 0).all() and (np.diff(T.TC0, axis=1) >= 0).all()
    assert T.ALPHA[51] == 255 and T.BETA[51] == 18 and T.TC0[51].tolist() == [13, 17, 25]
    assert T.TC0[17].tolist() == [0, 0, 1] and T.TC0[40].tolist() == [4, 5, 7] and T.ALPHA[40] == 80 and T.BETA[40] == 13


def test_the_kernels_carry_the_same_tables():
    """The device test meets a handful of QPs; every row of the tables in csrc/vcodec.hip is held to the definition's here."""
    import re
    with open(os.path.join(ROOT, "dove_amd", "csrc", "vcodec.hip")) as f:
        src = f.read()

    def table(name):
        body = re.search(name + r"\[52\](?:\[3\])? = \{(.*?)\};", src, re.S).group(1)
        return [int(v) for v in re.findall(r"\d+", body)]
    assert table("DB_ALPHA") == T.ALPHA.tolist() and table("DB_BETA") == T.BETA.tolist() and table("DB_TC0") == T.TC0.reshape(-1).tolist()


# ---- the clips of the device test reach every branch ------------------------------------------------------------------------------
def test_the_device_clips_reach_every_branch():
    total = T.new_stats()
    for shape in SHAPES:
        for rate in BITRATES:
            st = reference(shape, rate, T.ALL_TOOLS)[3]
            for k, v in st.items():
                if isinstance(v, dict):
                    for kk in v:
                        total[k][kk] += v[kk]
                elif isinstance(v, list):
                    total[k] = [a + b for a, b in zip(total[k], v)]
                else:
                    total[k] = total[k] + v
    print({k: v.tolist() if isinstance(v, np.ndarray) else v for k, v in total.items()})
    assert all(total["luma_mode"]) and all(total["chroma_mode"]) and all(total["dc_case"].values())
    assert (total["phase"] > 0).all()
    assert all(total["bs"]) and len(total["bs"]) == 5
    assert total["bs4_strong"] and total["bs4_weak"]
    assert all(total["ap"]) and all(total["aq"]) and total["p1_update"]


# ---- rate effect ------------------------------------------------------------------------------------------------------------------
def test_the_tools_lower_the_qp_of_a_fractionally_sliding_texture():
    Tx = texture(48 + 16, 64 + 16, 0)
    x = np.stack([bilinear_window(Tx, 48, 64, 4 + 0.5 * t, 4 + 0.75 * t) for t in range(6)]).astype(np.float32)
    plain = R.vcodec_roundtrip(x, 3000, 3, want_stats=True)[1].tolist()
    tools = T.vcodec_roundtrip(x, 3000, 3, T.ALL_TOOLS, want_stats=True)[1].tolist()
    print("QP without tools", plain, "with all tools", tools)
    assert all(a <= b for a, b in zip(tools, plain)) and any(a < b for a, b in zip(tools, plain))


# ---- recipes and refusals ---------------------------------------------------------------------------------------------------------
def test_sim_h264_recipes_are_sim_recipes_with_tools():
    seen = 0
    for seed in range(20):
        sim = D.Degrader(CONFIG, 4, seed, video_codec="sim", gop=4).recipe(6, 200, 300)
        h264 = D.Degrader(CONFIG, 4, seed, video_codec="sim-h264", gop=4).recipe(6, 200, 300)
        assert h264["version"] == D.RECIPE_VERSION == 1 and len(sim["steps"]) == len(h264["steps"])
        for a, b in zip(sim["steps"], h264["steps"]):
            if a["op"] == "vcodec":
                assert sorted(a) == ["bitrate", "codec", "gop", "op", "stage"]
                assert b == dict(a, tools=["intra16", "qpel", "deblock"])
                seen += 1
            else:
                assert a == b
        assert json.loads(json.dumps(h264)) == h264
    assert seen >= 20


def test_tool_names_and_bits():
    assert ops.VCODEC_TOOLS == T.TOOL_NAMES == {"intra16": 1, "qpel": 2, "deblock": 4}
    assert tuple(ops.VCODEC_TOOLS) == D.VCODEC_TOOLS
    for mask in (ops.vcodec_tools_mask, T.tools_mask):
        assert mask(0) == mask(()) == mask([]) == 0 and mask(7) == mask(["intra16", "qpel", "deblock"]) == mask(("deblock", "qpel", "intra16")) == 7
        assert mask(["qpel"]) == 2 and mask(5) == 5
        for bad in (8, -1, 15, ["x264"], ["qpel", "cabac"]):
            with pytest.raises(ValueError, match="tool"):
                mask(bad)
    with pytest.raises(ValueError, match="tool"):
        ops.vcodec_tools_mask("qpel")                                              # a bare string is not a list of names
    # the operator refuses on the host: the frames are host tensors, a device check would raise another error
    with pytest.raises(ValueError, match="tool"):
        ops.vcodec_roundtrip(torch.zeros(2, 16, 16, 3), 1000, 2, tools=["b-frames"])
    with pytest.raises(ValueError, match="tool"):
        ops.vcodec_roundtrip(torch.zeros(2, 16, 16, 3), 1000, 2, tools=8)


def test_apply_recipe_refuses_unknown_tools_before_any_device_call():
    step = {"op": "vcodec", "stage": "test", "codec": "h264", "bitrate": 20000, "gop": 8}
    recipe = {"version": D.RECIPE_VERSION, "seed": 0, "scale": 1, "frames": 8, "input_size": [16, 16], "output_size": [16, 16], "steps": [step]}
    x = torch.zeros(8, 16, 16, 3, dtype=torch.uint8)
    for bad in (["cabac"], ["qpel", "B"], "qpel", 7):
        with pytest.raises(ValueError, match="tools"):
            D.apply_recipe(x, dict(recipe, steps=[dict(step, tools=bad)]))
    D.check_block(dict(recipe, steps=[dict(step, tools=["qpel"])]), 0, 8)
    D.check_block(dict(recipe, steps=[dict(step, tools=[])]), 0, 8)
    D.check_block(recipe, 0, 8)
    with pytest.raises(ValueError, match="video_codec"):
        D.Degrader(CONFIG, 4, 0, video_codec="sim-h265")
    args = D.build_parser().parse_args(["--input_dir", "a", "--output_path", "b", "--config", CONFIG, "--video_codec", "sim-h264"])
    assert args.video_codec == "sim-h264"


def test_entry_points_refuse_bad_arguments():
    from dove_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    one = C.c_void_p(256)                                                         # never dereferenced: the checks come first

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.dove_last_error(), (rc, lib.dove_last_error())
    base = lib.dove_vcodec_workspace_bytes(5, 33, 47, 4)
    assert lib.dove_vcodec_tools_workspace_bytes(5, 33, 47, 4, 0) == base
    r256 = lambda v: -(-v // 256) * 256
    # a prediction frame per group, the quarter vectors and a 16-bit map per macroblock, each rounded up to 256
    extra = r256(2 * 48 * 48 * 3 // 2) + r256(5 * 9 * 8) + r256(5 * 9 * 2)
    for tools in range(1, 8):
        assert lib.dove_vcodec_tools_workspace_bytes(5, 33, 47, 4, tools) == base + extra
    for tools in (8, -1, 16 + 7):
        assert lib.dove_vcodec_tools_workspace_bytes(5, 33, 47, 4, tools) == 0
        refused(lib.dove_vcodec_roundtrip_tools(one, 5, 33, 47, 20000, 4, tools, one, base + extra, one, None, None, None), "tools")
    assert lib.dove_vcodec_tools_workspace_bytes(0, 33, 47, 4, 7) == 0 and lib.dove_vcodec_tools_workspace_bytes(5, 33, 47, 0, 7) == 0
    ws = base + extra
    for tools in (0, 7):
        refused(lib.dove_vcodec_roundtrip_tools(one, 5, 33, 47, 20000, 0, tools, one, ws, one, None, None, None), "gop")
        refused(lib.dove_vcodec_roundtrip_tools(one, 5, 33, 47, -1, 4, tools, one, ws, one, None, None, None), "bitrate")
        refused(lib.dove_vcodec_roundtrip_tools(one, 5, 33, 47, 20000, 4, tools, C.c_void_p(264), ws, one, None, None, None), "aligned")
        refused(lib.dove_vcodec_roundtrip_tools(None, 5, 33, 47, 20000, 4, tools, one, ws, one, None, None, None), "null")
        refused(lib.dove_vcodec_roundtrip_tools(one, 0, 33, 47, 20000, 4, tools, one, ws, one, None, None, None), "bad shape")
    refused(lib.dove_vcodec_roundtrip_tools(one, 5, 33, 47, 20000, 4, 0, one, base - 1, one, None, None, None), "workspace")
    refused(lib.dove_vcodec_roundtrip_tools(one, 5, 33, 47, 20000, 4, 7, one, ws - 1, one, None, None, None), "workspace")
    refused(lib.dove_vcodec_roundtrip_tools(one, 5, 33, 47, 20000, 4, 2, one, base, one, None, None, None), "workspace")
