"""The whole-video session of the graph level (dove_video_*; graph.VideoSession) on the GPU: its bytes equal the composition of existing
code - GraphContext.sr_clip per piece with ops.randn noise, tiling.plan / stitch / check_coverage, then prepost, colorfix and yuv in
stream.sr_stream's order.  Small model (config.small_configs(num_layers=1)), LR frames of 32x48, as tests/test_stream_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import yuv_ref as R
from dove_amd import config, ops, prepost, tiling, weights
from dove_amd import lib as L
from dove_amd import yuv as yuvmod
from dove_amd.graph import GraphContext, VideoSession

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
H, W, UP = 32, 48, 4
TILES = dict(tile_size_hw=(64, 96), overlap_hw=(32, 32))           # 3 x 2 spatial tiles of the 128 x 192 frames
ONE = dict(tile_size_hw=(0, 0), overlap_hw=(32, 32))
CHUNKED = dict(chunk_len=17, overlap_t=8)
WHOLE = dict(chunk_len=0, overlap_t=8)
SEED = 20240607
IN_HEADER = b"YUV4MPEG2 W48 H32 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=LIMITED\n"
FMT_IN = yuvmod.YuvFormat("420", "bt601", "limited", "left")
FMT_IN_444 = yuvmod.YuvFormat("444", "bt709", "full")


@pytest.fixture(scope="module")
def setup(golden_dir):
    from safetensors.torch import load_file

    from dove_amd.scheduler import CogVideoXDPMScheduler
    v, t, s = config.small_configs(num_layers=1)
    wv = weights.random_state_dict(weights.vae_param_shapes(v), 7)
    wt = weights.random_state_dict(weights.dit_param_shapes(t), 7)
    ctx = GraphContext(v, t, wv, wt, "cuda")
    text = load_file(os.path.join(golden_dir, "empty_prompt_embedding.safetensors"))["prompt_embedding"].to(BF).cuda()
    if text.dim() == 3:
        text = text[0]
    sched = CogVideoXDPMScheduler(**dict(s, timestep_spacing="trailing"))
    sa, s1 = sched._coeffs(torch.tensor([399]), BF)
    return dict(ctx=ctx, text=text.contiguous(), sched=sched, sa=sa, s1=s1, cfg=(v, t, s, wv, wt))


def lr_payload(F, seed=0, chroma="420"):
    """A smooth random 4:2:0 (or 4:4:4) clip (payloads [F, frame_bytes])."""
    g = np.random.default_rng(seed)
    base = g.integers(40, 216, size=(1, R.frame_bytes(H, W, chroma)))
    return np.clip(base + g.integers(-30, 31, size=(F, base.shape[1])), 0, 255).astype(np.uint8)


def lr_rgb(F, seed=0):
    return R.yuv_to_rgb(lr_payload(F, seed), H, W, "bt601", "limited", "420", "left")


def composition(st, data, *, in_fmt=None, out_fmt=None, color_fix=None, noise_step=None, seed=SEED, sr_clip=None, chunk_len=0, overlap_t=8,
                tile_size_hw=(0, 0), overlap_hw=(32, 32), geom=(H, W, UP)):
    """The yardstick: existing code only.  ``data``: host uint8 frames [F,H,W,3] or payloads [F, bytes] -> (host uint8 output, pieces)."""
    ctx, text = st["ctx"], st["text"]
    H, W, UP = geom
    dev = torch.from_numpy(data).cuda()
    rgb = yuvmod.yuv_to_rgb(dev, H, W, in_fmt) if in_fmt is not None else dev
    F = rgb.shape[0]
    pad_f, pad_h, pad_w = tiling.match_padding(F, H, W)
    video = ops.preprocess_u8(rgb.contiguous(), pad_f, pad_h, pad_w, UP, BF)[None]
    items = tiling.plan(video.shape, chunk_len, overlap_t, tile_size_hw, overlap_hw)
    out = torch.zeros(video.shape, dtype=BF, device="cuda")
    wc = torch.zeros(video.shape, dtype=torch.int32, device="cuda")
    lat = st["cfg"][0]["latent_channels"]
    for p, ((t0, t1, h0, h1, w0, w1), region) in enumerate(items):
        T = 1 + (t1 - t0 - 1) // 4
        noise = ops.randn((lat, T, (h1 - h0) // 8, (w1 - w0) // 8), seed, 2 * p)
        pre = None
        if noise_step:
            pre = (ops.randn((T + T % 2, lat, (h1 - h0) // 8, (w1 - w0) // 8), seed, 2 * p + 1),) + tuple(noise_step[1:])
        clip = video[0, :, t0:t1, h0:h1, w0:w1].contiguous()
        if sr_clip is not None:
            piece = sr_clip(clip, noise)
        else:
            piece = ctx.sr_clip(clip, noise, text, 399, st["sa"], st["s1"], pre_noise=pre)
        tiling.stitch(out, wc, piece[None], region)
    tiling.check_coverage(wc)
    Ho, Wo = H * UP - pad_h * 4, W * UP - pad_w * 4
    if color_fix:
        frames = prepost.postprocess_frames(out, pad_f, pad_h, pad_w, color_fix=color_fix, source=video)
        res = yuvmod.rgb_to_yuv(frames, out_fmt) if out_fmt is not None else frames
    elif out_fmt is not None:
        res = yuvmod.rgb_to_yuv(out, out_fmt, crop=(F, Ho, Wo))
    else:
        res = prepost.postprocess_frames(out, pad_f, pad_h, pad_w)
    torch.cuda.synchronize()
    return res.cpu().numpy(), len(items)


def run_session(st, data, *, blocks=None, in_fmt=None, out_fmt=None, color_fix=None, noise_step=None, seed=SEED, aux=None, max_push=0,
                geom=(H, W, UP), **plan):
    """Push ``data`` (in ``blocks``-sized pushes, cycling; None = everything at once) whenever need() asks, step, collect."""
    H, W, UP = geom
    F = data.shape[0]
    dev = torch.from_numpy(data).cuda()
    sess = VideoSession(st["ctx"], W, H, st["text"], 399, st["sa"], st["s1"], upscale=UP, color_fix=color_fix, in_fmt=in_fmt, out_fmt=out_fmt,
                        noise_step=noise_step, seed=seed, max_frames=F if plan.get("chunk_len", 0) == 0 else 0,
                        max_push=max_push or (F if blocks is None else max(blocks)), aux=aux, **plan)
    outs, pos, steps, i = [], 0, 0, 0
    try:
        while not sess.done:
            need = sess.need()
            while pos < F and (need is None or need > 0):
                n = F - pos if blocks is None else min(blocks[i % len(blocks)], F - pos)
                i += 1
                sess.push(dev[pos:pos + n])
                pos += n
                need = sess.need()
            if pos == F:
                sess.end()
                assert sess.need() == 0
            outs.append(sess.step().cpu())
            steps += 1
            assert steps <= F + 2, "the session does not finish"
        torch.cuda.synchronize()
        assert sess.step().shape[0] == 0 and sess.done                # a step after the last chunk writes nothing
    finally:
        sess.close()
    return torch.cat(outs).numpy(), steps


CASES = [
    # id, F, plan, in, out, colour fix
    ("whole-clip", 9, dict(WHOLE, **ONE), None, None, None),
    ("one-chunk-wavelet", 17, dict(CHUNKED, **ONE), None, None, "wavelet"),
    ("merged-tail-tiles-420", 49, dict(CHUNKED, **TILES), "420", "420", None),
    ("padded-tail-tiles-444-adain", 44, dict(CHUNKED, **TILES), "420", "444", "adain"),
    ("nine-chunks-rgb-to-422", 89, dict(CHUNKED, **ONE), None, "422", None),
    ("tiles-whole-clip-wavelet-420", 9, dict(WHOLE, **TILES), "420", "420", "wavelet"),
    ("two-chunks-tiles-444-in-444-out", 26, dict(CHUNKED, **TILES), "444", "444", None),
]


@pytest.mark.parametrize("name,F,plan,cin,cout,color_fix", CASES, ids=[c[0] for c in CASES])
def test_session_equals_the_composition_byte_for_byte(setup, name, F, plan, cin, cout, color_fix):
    Fp = F + tiling.match_padding(F, H, W)[0]
    chunks = tiling.make_temporal_chunks(Fp, plan["chunk_len"], plan["overlap_t"] if plan["chunk_len"] else 0)
    want_chunks = {"whole-clip": [(0, 9)], "one-chunk-wavelet": [(0, 17)], "merged-tail-tiles-420": [(0, 17), (9, 26), (18, 35), (27, 49)],
                   "padded-tail-tiles-444-adain": [(0, 17), (9, 26), (18, 35), (27, 49)],      # 44 frames: five padded, the tail merged
                   "nine-chunks-rgb-to-422": [(9 * i, 9 * i + 17) for i in range(9)],          # 89 = 17 + 8 * 9: no merge, no padding
                   "tiles-whole-clip-wavelet-420": [(0, 9)],
                   "two-chunks-tiles-444-in-444-out": [(0, 17), (9, 33)]}[name]                 # 26 frames: seven padded
    assert chunks == want_chunks
    data = lr_payload(F, seed=F, chroma=cin) if cin else lr_rgb(F, seed=F)
    in_fmt = {None: None, "420": FMT_IN, "444": FMT_IN_444}[cin]         # 444 in: no chroma upsampling, three full planes per frame
    out_fmt = yuvmod.YuvFormat(cout, "bt601", "limited") if cout else None
    want, pieces = composition(setup, data, in_fmt=in_fmt, out_fmt=out_fmt, color_fix=color_fix, **plan)
    got, steps = run_session(setup, data, in_fmt=in_fmt, out_fmt=out_fmt, color_fix=color_fix, **plan)
    n_tiles = 6 if plan["tile_size_hw"] != (0, 0) else 1
    assert steps == len(chunks) and pieces == steps * n_tiles
    assert got.shape == want.shape and got.shape[0] == F
    assert got.tobytes() == want.tobytes()


def test_vae_tiling_option_applies_inside_the_session(setup):
    """DOVE_OPT_VAE_TILING on: the geometry of tests/test_graph_gpu.py::test_option_vae_tiling_bit_exact - sample size 96 x 160, so 48 x 80 px
    VAE tiles, 3 x 3 with ragged last ones, on a 9 x 112 x 192 clip (LR frames of that size at x1)."""
    ctx = setup["ctx"]
    geom = (112, 192, 1)
    data = np.random.default_rng(3).integers(0, 256, size=(9, 112, 192, 3), dtype=np.uint8)
    plain, _ = run_session(setup, data, geom=geom, **WHOLE, **ONE)
    try:
        ctx.set_option(L.OPT_VAE_SAMPLE_HEIGHT, 96)
        ctx.set_option(L.OPT_VAE_SAMPLE_WIDTH, 160)
        ctx.enable_tiling()
        want, _ = composition(setup, data, geom=geom, **WHOLE, **ONE)
        got, _ = run_session(setup, data, geom=geom, **WHOLE, **ONE)
    finally:
        ctx.enable_tiling(False)
        ctx.set_option(L.OPT_VAE_SAMPLE_HEIGHT, 480)
        ctx.set_option(L.OPT_VAE_SAMPLE_WIDTH, 720)
    assert got.shape == (9, 112, 192, 3) and got.tobytes() == want.tobytes()
    assert got.tobytes() != plain.tobytes()                           # the option did switch


def test_session_equals_the_facade_with_host_tables(setup):
    """The graph level is bit-identical to the Python facade when it is handed the facade's own RoPE tables and timestep projection
    (tests/test_graph_gpu.py): the session takes them per piece through ``aux``; the facade gets the session's noise as posterior_noise."""
    from dove_amd.inference import process_video
    from dove_amd.pipeline import CogVideoXPipeline
    from dove_amd.rope import prepare_rotary_positional_embeddings
    v, t, s, _, _ = setup["cfg"]
    pipe = CogVideoXPipeline.from_config(v, t, s, seed=7, device="cuda")
    tp = pipe.transformer.timestep_projection(399)

    def aux(T, h, w):
        return prepare_rotary_positional_embeddings(height=h * 8, width=w * 8, num_frames=T, transformer_config=pipe.transformer.config,
                                                    vae_scale_factor_spatial=8, device="cuda"), tp

    def facade(clip, noise):
        return process_video(pipe, clip[None], empty_prompt_embedding=setup["text"], posterior_noise=noise[None])[0]

    data = lr_rgb(26, seed=5)                                         # padded to 33: chunks (0, 17), (9, 33)
    plan = dict(CHUNKED, **ONE)
    want, pieces = composition(setup, data, sr_clip=facade, **plan)
    got, steps = run_session(setup, data, aux=aux, **plan)
    assert steps == pieces == 2
    assert got.tobytes() == want.tobytes()


def test_noise_step_draws_eps_from_the_odd_stream(setup):
    na, n1 = setup["sched"]._coeffs(torch.tensor([200]), BF)
    data = lr_rgb(17, seed=8)
    plan = dict(CHUNKED, **TILES)
    want, _ = composition(setup, data, noise_step=(200, na, n1), **plan)
    got, _ = run_session(setup, data, noise_step=(200, na, n1), **plan)
    base, _ = run_session(setup, data, **plan)
    assert got.tobytes() == want.tobytes() and got.tobytes() != base.tobytes()
    other, _ = run_session(setup, data, seed=SEED + 1, **plan)
    assert other.tobytes() != base.tobytes()                          # and the seed is the session's


def test_uneven_pushes_give_the_same_bytes(setup):
    data = lr_payload(49, seed=11)
    fmt = yuvmod.YuvFormat("420", "bt601", "limited")
    plan = dict(CHUNKED, **ONE)
    once, steps = run_session(setup, data, in_fmt=FMT_IN, out_fmt=fmt, **plan)
    uneven, steps2 = run_session(setup, data, blocks=(1, 5, 40), in_fmt=FMT_IN, out_fmt=fmt, **plan)
    assert steps == steps2 == 4 and uneven.tobytes() == once.tobytes()
    # need() is the planner's: 26 frames for the first chunk, 9 more for each further one, nothing once the end is known
    sess = VideoSession(setup["ctx"], W, H, setup["text"], 399, setup["sa"], setup["s1"], in_fmt=FMT_IN, out_fmt=fmt, **plan)
    try:
        dev = torch.from_numpy(data).cuda()
        assert sess.need() == 26
        sess.push(dev[:20])
        assert sess.need() == 6
        with pytest.raises(RuntimeError, match="needs 26 known frames"):
            sess.step()
        sess.push(dev[20:30])
        assert sess.need() == 0
        assert sess.step().shape[0] == 13 and sess.need() == 5        # frames 0..12 are final; the chunk at 9 needs 35 known frames
        with pytest.raises(RuntimeError, match="do not fit"):
            sess.push(torch.zeros(200, sess.in_frame_bytes, dtype=torch.uint8, device="cuda"))
        sess.end()
        assert sess.need() == 0
        tail = sess.step()                                            # 30 frames -> padded to 33: (9, 33) is the last chunk
        assert sess.done and tail.shape[0] == 30 - 13
    finally:
        sess.close()


def test_an_odd_overlap_writes_the_seam_frame_twice_and_is_refused(setup):
    """overlap_t 7: both chunks drop 7 // 2 = 3 frames of the 7 they share, so frame 13 is kept twice.  The reference's whole-clip count
    says so (tiling.check_coverage in the composition); the session, which never sees the whole clip, finds it at the seam."""
    data = lr_rgb(33, seed=4)
    plan = dict(chunk_len=17, overlap_t=7, **ONE)
    assert tiling.make_temporal_chunks(33, 17, 7) == [(0, 17), (10, 33)]
    with pytest.raises(RuntimeError, match=r"Error: Write count > 1 in region !!!"):
        composition(setup, data, **plan)
    sess = VideoSession(setup["ctx"], W, H, setup["text"], 399, setup["sa"], setup["s1"], **plan)
    try:
        sess.push(torch.from_numpy(data).cuda())
        sess.end()
        assert sess.step().shape[0] == 14                             # frames 0..13
        with pytest.raises(RuntimeError, match=r"Error: Write count > 1 in region !!!"):
            sess.step()                                               # (10, 33) keeps 13..32
        assert not sess.done
    finally:
        sess.close()


def test_a_failing_aux_fn_refuses_the_step_and_changes_nothing(setup):
    calls = []

    def aux(T, h, w):
        calls.append((T, h, w))
        if len(calls) == 1:
            raise RuntimeError("no tables yet")
        return None, None

    data = lr_rgb(9, seed=2)
    sess = VideoSession(setup["ctx"], W, H, setup["text"], 399, setup["sa"], setup["s1"], chunk_len=0, max_frames=9, aux=aux, seed=SEED, **ONE)
    try:
        sess.push(torch.from_numpy(data).cuda())
        sess.end()
        with pytest.raises(RuntimeError, match="aux_fn failed for a 4 x 16 x 24 latent grid"):
            sess.step()
        got = sess.step().cpu().numpy()                               # the same step again: nothing was advanced, piece 0 draws stream 0
        assert sess.done and calls == [(4, 16, 24), (4, 16, 24)]
    finally:
        sess.close()
    want, _ = composition(setup, data, **WHOLE, **ONE)
    assert got.tobytes() == want.tobytes()


def test_bounded_memory(setup):
    """Mirror of tests/test_stream_gpu.py::test_bounded_memory: twelve chunks need what four chunks with the same tail length need - the
    arena's high water plus the session's one allocation, which is sized before the first frame is known."""
    v, t, s, wv, wt = setup["cfg"]
    ctx = GraphContext(v, t, wv, wt, "cuda")                        # a context of its own: the high water is a lifetime maximum
    st = dict(setup, ctx=ctx)
    plan = dict(CHUNKED, **TILES)
    short, long_ = tiling.make_temporal_chunks(49, 17, 8), tiling.make_temporal_chunks(121, 17, 8)
    assert (len(short), len(long_)) == (4, 12) and short[-1][1] - short[-1][0] == long_[-1][1] - long_[-1][0]
    totals = {}
    for F in (49, 121):
        _, steps = run_session(st, lr_rgb(F, seed=3), blocks=(9,), **plan)
        probe = VideoSession(ctx, W, H, st["text"], 399, st["sa"], st["s1"], max_push=9, **plan)      # run_session's settings
        totals[F] = (ctx.workspace_high_water(), probe.workspace_bytes(), steps)
        probe.close()
    print(f"[video] 4 chunks: arena high water {totals[49][0] / 2**20:.1f} MiB + session {totals[49][1] / 2**20:.1f} MiB; 12 chunks: "
          f"{totals[121][0] / 2**20:.1f} MiB + {totals[121][1] / 2**20:.1f} MiB")
    assert totals[49][2] == 4 and totals[121][2] == 12
    assert totals[49][:2] == totals[121][:2] and totals[49][0] > 0 and totals[49][1] > 0


def test_errors_leave_the_context_usable(setup):
    ctx, text = setup["ctx"], setup["text"]
    v, t, s, wv, wt = setup["cfg"]
    kw = dict(in_fmt=None, out_fmt=None)
    # a clip of <= overlap_t frames has no chunk at all: the reference's coverage message
    sess = VideoSession(ctx, W, H, text, 399, setup["sa"], setup["s1"], chunk_len=17, overlap_t=9, **ONE, **kw)
    sess.push(torch.from_numpy(lr_rgb(1)).cuda())
    sess.end()
    with pytest.raises(RuntimeError, match="Error: Lack of write in region !!!"):
        sess.step()
    sess.close()
    # no input at all
    sess = VideoSession(ctx, W, H, text, 399, setup["sa"], setup["s1"], **CHUNKED, **ONE, **kw)
    sess.end()
    with pytest.raises(RuntimeError, match="holds no frame"):
        sess.step()
    sess.close()
    # an output buffer that is too small: refused before anything runs, and the same step then succeeds
    sess = VideoSession(ctx, W, H, text, 399, setup["sa"], setup["s1"], **WHOLE, **ONE, max_frames=9, **kw)
    sess.push(torch.from_numpy(lr_rgb(9, seed=2)).cuda())
    sess.end()
    small = torch.empty(8, UP * H, UP * W, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="this step writes 9 frames"):
        sess.step(small)
    assert not sess.done and sess.step().shape[0] == 9 and sess.done
    sess.close()
    # settings the planner refuses
    with pytest.raises(RuntimeError, match="chunk_len must be greater than overlap"):
        VideoSession(ctx, W, H, text, 399, setup["sa"], setup["s1"], chunk_len=8, overlap_t=8)
    with pytest.raises(RuntimeError, match="Tile size must be greater than overlap"):
        VideoSession(ctx, W, H, text, 399, setup["sa"], setup["s1"], tile_size_hw=(32, 32), overlap_hw=(32, 32), **CHUNKED)
    with pytest.raises(RuntimeError, match="max_frames"):
        VideoSession(ctx, W, H, text, 399, setup["sa"], setup["s1"], chunk_len=0)
    # a context with a communicator is refused
    multi = GraphContext(v, t, wv, wt, "cuda")
    multi.comm_init_custom(0, 2, lambda *a: 0, lambda *a: 0)
    with pytest.raises(RuntimeError, match="communicator"):
        VideoSession(multi, W, H, text, 399, setup["sa"], setup["s1"], **CHUNKED)
    multi.comm_destroy()
    # and the context still computes what it computed
    data = lr_rgb(9, seed=2)
    want, _ = composition(setup, data, **WHOLE, **ONE)
    got, _ = run_session(setup, data, **WHOLE, **ONE)
    assert got.tobytes() == want.tobytes()


def test_streaming_errors_surface_and_threads_end(setup):
    """tests/test_stream_gpu.py's test of the same name through ``stream.sr_stream_graph``: a broken output pipe, a truncated input and an
    input without a frame end the run with their error, no worker thread stays behind, and the context computes what it computed."""
    import io
    import threading
    import time

    from dove_amd import stream, y4m

    class Broken(io.BytesIO):
        def write(self, b):
            if self.tell() > 200:
                raise BrokenPipeError(32, "Broken pipe")
            return super().write(b)

    def attempt(raw, sink):
        reader = y4m.Y4MReader(io.BytesIO(raw))
        writer = y4m.Y4MWriter(sink, UP * W, UP * H, 25, "420", False)
        box = {}

        def work():
            try:
                stream.sr_stream_graph(setup["ctx"], setup["sched"], reader, writer, setup["text"], upscale=UP, seed=SEED, log=lambda m: None,
                                       **CHUNKED, **TILES)
            except BaseException as e:                               # noqa: BLE001
                box["error"] = e
        before = threading.active_count()
        t = threading.Thread(target=work, daemon=True)
        t.start()
        t.join(120)
        assert not t.is_alive(), "sr_stream_graph hangs"
        deadline = time.time() + 5
        while threading.active_count() > before and time.time() < deadline:
            time.sleep(0.05)
        assert threading.active_count() <= before, "worker threads left behind"
        got, _ = run_session(setup, data, **WHOLE, **ONE)             # and the context still computes what it computed
        assert got.tobytes() == want.tobytes()
        return box.get("error")

    data = lr_rgb(9, seed=2)
    want, _ = composition(setup, data, **WHOLE, **ONE)
    clip = IN_HEADER + b"".join(b"FRAME\n" + fr.tobytes() for fr in lr_payload(26, seed=1))
    assert isinstance(attempt(clip, Broken()), BrokenPipeError)
    err = attempt(clip[:-100], io.BytesIO())
    assert isinstance(err, ValueError) and "truncated" in str(err)
    err = attempt(IN_HEADER, io.BytesIO())
    assert isinstance(err, ValueError) and "no frame" in str(err)


def test_stream_tool_with_graph_equals_the_session(golden_dir):
    """python -m dove_amd.stream --graph on a Y4M pipe: stdout is the Y4M stream of the in-process session on the same weights and seed."""
    import argparse

    from dove_amd import cli, stream
    F = 44
    payload = lr_payload(F, seed=9)
    flags = ["--random_init", "--num_layers", "1", "--prompt_embedding", os.path.join(golden_dir, "empty_prompt_embedding.safetensors"),
             "--chunk_len", "17", "--overlap_t", "8", "--tile_size_hw", "64", "96", "--overlap_hw", "32", "32", "--save_format", "yuv420p",
             "--seed", "123", "--color_fix", "wavelet"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    data = IN_HEADER + b"".join(b"FRAME\n" + fr.tobytes() for fr in payload)
    child = subprocess.run([sys.executable, "-m", "dove_amd.stream", "--graph", "--input", "-", "--output", "-"] + flags, input=data,
                           capture_output=True, timeout=240, cwd=ROOT, env=env)
    log = child.stderr.decode(errors="replace")
    assert child.returncode == 0, log[-2000:]
    assert "[dove_amd.stream] done: 44 frames in 4 chunks (24 pieces)" in log
    header = b"YUV4MPEG2 W192 H128 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    fb = R.frame_bytes(UP * H, UP * W, "420")
    assert child.stdout.startswith(header) and len(child.stdout) == len(header) + F * (6 + fb)
    ap = argparse.ArgumentParser()
    cli.add_model_arguments(ap)
    ctx, emb, sched = stream.build_graph(ap.parse_args(flags))
    sa, s1 = sched._coeffs(torch.tensor([399]), BF)
    st = dict(ctx=ctx, text=emb.to(BF).cuda(), sa=sa, s1=s1)
    got, _ = run_session(st, payload, in_fmt=FMT_IN, out_fmt=yuvmod.YuvFormat("420", "bt601", "limited"), color_fix="wavelet", seed=123,
                         **CHUNKED, **TILES)
    assert child.stdout == header + b"".join(b"FRAME\n" + fr.tobytes() for fr in got)
    # --upscale_mode other than bilinear is refused with --graph, before any model is built
    bad = subprocess.run([sys.executable, "-m", "dove_amd.stream", "--graph", "--upscale_mode", "bicubic", "--input", "-", "--output", "-"] + flags,
                         input=data, capture_output=True, timeout=120, cwd=ROOT, env=env)
    assert bad.returncode == 2 and b"bilinear" in bad.stderr
