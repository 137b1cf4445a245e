"""Streaming SR (dove_amd.stream) on the GPU: byte-identical to the in-memory chunk loop, bounded device memory, and the Y4M ends of
the command-line tools.  Small model (config.small_configs(num_layers=1)), LR frames of 32x48."""
import io
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest
import torch

import yuv_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 32, 48
SR = dict(chunk_len=17, overlap_t=8, tile_size_hw=(64, 96), overlap_hw=(32, 32))      # 3 x 2 spatial tiles of the 128 x 192 frames
IN_HEADER = b"YUV4MPEG2 W48 H32 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=LIMITED\n"


@pytest.fixture(scope="module")
def setup(golden_dir):
    from safetensors.torch import load_file

    from dove_amd import config
    from dove_amd.pipeline import CogVideoXPipeline
    v, t, s = config.small_configs(num_layers=1)
    pipe = CogVideoXPipeline.from_config(v, t, s, seed=7, device="cuda")
    text = load_file(os.path.join(golden_dir, "empty_prompt_embedding.safetensors"))["prompt_embedding"]
    return pipe, text


def lr_payload(F, seed=0):
    """A smooth random 4:2:0 clip (payloads [F, frame_bytes])."""
    g = np.random.default_rng(seed)
    base = g.integers(40, 216, size=(1, R.frame_bytes(H, W, "420")))
    return np.clip(base + g.integers(-30, 31, size=(F, base.shape[1])), 0, 255).astype(np.uint8)


def y4m_bytes(header, payload):
    return header + b"".join(b"FRAME\n" + fr.tobytes() for fr in payload)


def in_memory_frames(pipe, text, rgb, generator, color_fix=None, settings=SR):
    """The chunk x tile loop of dove_amd.cli.main on the whole clip -> host uint8 [F,H,W,3]."""
    from dove_amd import prepost, tiling
    from dove_amd.inference import process_video
    video, pad_f, pad_h, pad_w, _ = prepost.preprocess_frames(torch.from_numpy(rgb), 4)
    items = tiling.plan(video.shape, settings["chunk_len"], settings["overlap_t"], settings["tile_size_hw"], settings["overlap_hw"])
    out = torch.zeros(video.shape, dtype=torch.bfloat16, device=video.device)
    wc = torch.zeros(video.shape, dtype=torch.int32, device=video.device)
    for (t0, t1, h0, h1, w0, w1), region in items:
        piece = process_video(pipe, video[:, :, t0:t1, h0:h1, w0:w1], empty_prompt_embedding=text, generator=generator)
        tiling.stitch(out, wc, piece, region)
    tiling.check_coverage(wc)
    frames = prepost.postprocess_frames(out, pad_f, pad_h, pad_w, color_fix=color_fix, source=video if color_fix else None)
    return frames.cpu().numpy(), len(items)


def run_stream(pipe, text, payload, generator, chroma, color_fix=None, settings=SR):
    from dove_amd import stream, y4m
    reader = y4m.Y4MReader(io.BytesIO(y4m_bytes(IN_HEADER, payload)))
    sink = io.BytesIO()
    writer = y4m.Y4MWriter(sink, 4 * W, 4 * H, reader.fps, chroma, False)
    done = {}

    def work():
        done["stats"] = stream.sr_stream(pipe, reader, writer, upscale=4, empty_prompt_embedding=text, color_fix=color_fix,
                                         generator=generator, log=lambda m: None, **settings)
    t = threading.Thread(target=work, daemon=True)                   # a deadlock fails the test instead of holding the card
    t.start()
    t.join(120)
    assert not t.is_alive(), "sr_stream did not finish"
    assert "stats" in done, "sr_stream raised"
    return sink.getvalue(), writer.header, done["stats"]


@pytest.mark.parametrize("F,chroma,color_fix,chunks", [(49, "420", None, [(0, 17), (9, 26), (18, 35), (27, 49)]),
                                                        (44, "444", None, [(0, 17), (9, 26), (18, 35), (27, 49)]),
                                                        (49, "422", "wavelet", None)])
def test_streaming_equals_in_memory_byte_for_byte(setup, F, chroma, color_fix, chunks):
    from dove_amd import tiling
    pipe, text = setup
    payload = lr_payload(F, seed=F)
    rgb = R.yuv_to_rgb(payload, H, W, "bt601", "limited", "420", "left")
    Fp = F + tiling.match_padding(F, H, W)[0]
    if chunks:
        assert Fp == 49 and tiling.make_temporal_chunks(Fp, 17, 8) == chunks          # F = 44: five padding frames and a merged tail
    frames, n_items = in_memory_frames(pipe, text, rgb, torch.Generator(device="cuda").manual_seed(5), color_fix)
    assert frames.shape == (F, 4 * H, 4 * W, 3)
    got, header, stats = run_stream(pipe, text, payload, torch.Generator(device="cuda").manual_seed(5), chroma, color_fix)
    want = y4m_bytes(header, R.rgb_to_yuv(frames, "bt601", "limited", chroma))
    assert stats == {"frames": F, "chunks": 4, "pieces": n_items} and n_items == 24
    assert len(got) == len(want)
    assert got == want


def test_streaming_errors_surface_and_threads_end(setup):
    """A broken output pipe, a truncated input and a clip of F <= overlap_t frames end the run with an error; nothing hangs."""
    from dove_amd import stream, y4m
    pipe, text = setup

    class Broken(io.BytesIO):
        def write(self, b):
            if self.tell() > 200:
                raise BrokenPipeError(32, "Broken pipe")
            return super().write(b)

    def attempt(data, sink, **kw):
        reader = y4m.Y4MReader(io.BytesIO(data))
        writer = y4m.Y4MWriter(sink, 4 * W, 4 * H, 25, "420", False)
        box = {}

        def work():
            try:
                stream.sr_stream(pipe, reader, writer, upscale=4, empty_prompt_embedding=text, log=lambda m: None, **dict(SR, **kw))
            except BaseException as e:                               # noqa: BLE001
                box["error"] = e
        before = threading.active_count()
        t = threading.Thread(target=work, daemon=True)
        t.start()
        t.join(120)
        assert not t.is_alive(), "sr_stream hangs"
        deadline = time.time() + 5
        while threading.active_count() > before and time.time() < deadline:
            time.sleep(0.05)
        assert threading.active_count() <= before, "worker threads left behind"
        return box.get("error")

    clip = y4m_bytes(IN_HEADER, lr_payload(26, seed=1))
    assert isinstance(attempt(clip, Broken()), BrokenPipeError)
    err = attempt(clip[:-100], io.BytesIO())
    assert isinstance(err, ValueError) and "truncated" in str(err)
    err = attempt(y4m_bytes(IN_HEADER, lr_payload(1, seed=1)), io.BytesIO(), chunk_len=17, overlap_t=9)   # one frame <= overlap_t: no chunk
    assert isinstance(err, RuntimeError) and str(err) == "Error: Lack of write in region !!!"
    err = attempt(IN_HEADER, io.BytesIO())
    assert isinstance(err, ValueError) and "no frame" in str(err)


@pytest.mark.parametrize("chunk_len,overlap_t,F_short,F_long,n_short,n_long", [(17, 8, 49, 121, 4, 12), (16, 8, 41, 73, 4, 8)])
def test_bounded_memory(setup, chunk_len, overlap_t, F_short, F_long, n_short, n_long):
    """More chunks need no more device memory than four chunks with the same tail length, and less than the in-memory loop on the same
    clip.  Clips are padded to 8N+1 frames, so with --chunk_len 17 --overlap_t 8 (stride 9) the tail length repeats every 72 frames: the
    4-chunk clip (49 frames, tail 22) is paired with the 12-chunk one (121); 4 against exactly 8 chunks with equal tails needs an even
    stride, which --chunk_len 16 --overlap_t 8 has (41 and 73 frames, tail 17)."""
    pipe, text = setup
    from dove_amd import tiling
    short, long_ = tiling.make_temporal_chunks(F_short, chunk_len, overlap_t), tiling.make_temporal_chunks(F_long, chunk_len, overlap_t)
    assert (len(short), len(long_)) == (n_short, n_long) and short[-1][1] - short[-1][0] == long_[-1][1] - long_[-1][0]
    assert tiling.match_padding(F_short, H, W)[0] == 0 and tiling.match_padding(F_long, H, W)[0] == 0
    settings = dict(SR, chunk_len=chunk_len, overlap_t=overlap_t)
    # the model and whatever it caches per piece shape (workspace, rotary tables) are resident before anything is measured
    run_stream(pipe, text, lr_payload(F_short, seed=3), torch.Generator(device="cuda").manual_seed(5), "420", settings=settings)
    peaks = {}
    for F, n in ((F_long, n_long), (F_short, n_short)):
        payload = lr_payload(F, seed=3)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _, _, stats = run_stream(pipe, text, payload, torch.Generator(device="cuda").manual_seed(5), "420", settings=settings)
        torch.cuda.synchronize()
        peaks[F] = torch.cuda.max_memory_allocated() - base
        assert stats["chunks"] == n
    rgb = R.yuv_to_rgb(lr_payload(F_long, seed=3), H, W, "bt601", "limited", "420", "left")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    in_memory_frames(pipe, text, rgb, torch.Generator(device="cuda").manual_seed(5), settings=settings)
    torch.cuda.synchronize()
    peak_mem = torch.cuda.max_memory_allocated() - base
    print(f"[stream] peak device memory above the model, --chunk_len {chunk_len} --overlap_t {overlap_t}: {n_long} chunks "
          f"{peaks[F_long] / 2**20:.1f} MiB, {n_short} chunks {peaks[F_short] / 2**20:.1f} MiB, in-memory loop on the {n_long}-chunk clip "
          f"{peak_mem / 2**20:.1f} MiB")
    assert peaks[F_long] <= peaks[F_short]
    assert peak_mem > peaks[F_long]


def _model_flags(golden_dir):
    return ["--random_init", "--num_layers", "1", "--prompt_embedding", os.path.join(golden_dir, "empty_prompt_embedding.safetensors")]


def test_stream_module_as_a_child_process(golden_dir):
    """python -m dove_amd.stream --input - --output -: stdout is ONLY the Y4M stream, equal to the in-memory loop of the same model and
    seed; the log is on stderr."""
    import argparse

    from dove_amd import cli
    F = 49
    payload = lr_payload(F, seed=9)
    flags = _model_flags(golden_dir) + ["--chunk_len", "17", "--overlap_t", "8", "--tile_size_hw", "64", "96", "--overlap_hw", "32", "32",
                                        "--save_format", "yuv420p", "--seed", "123"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    child = subprocess.run([sys.executable, "-m", "dove_amd.stream", "--input", "-", "--output", "-"] + flags,
                           input=y4m_bytes(IN_HEADER, payload), capture_output=True, timeout=240, cwd=ROOT, env=env)
    log = child.stderr.decode(errors="replace")
    assert child.returncode == 0, log[-2000:]
    assert "[dove_amd.stream] done: 49 frames in 4 chunks (24 pieces)" in log and "C420mpeg2" in log
    header = b"YUV4MPEG2 W192 H128 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert child.stdout.startswith(header)
    assert len(child.stdout) == len(header) + F * (6 + R.frame_bytes(4 * H, 4 * W, "420"))
    # the same model, seed and global generator state in this process
    ap = argparse.ArgumentParser()
    cli.add_model_arguments(ap)
    pipe, emb = cli.build_pipe(ap.parse_args(flags))
    rgb = R.yuv_to_rgb(payload, H, W, "bt601", "limited", "420", "left")
    frames, _ = in_memory_frames(pipe, emb, rgb, None)
    assert child.stdout == y4m_bytes(header, R.rgb_to_yuv(frames, "bt601", "limited", "420"))


def test_cli_y4m_in_and_out(golden_dir, tmp_path):
    from dove_amd import cli, metrics, y4m
    inp, gt, out = tmp_path / "in", tmp_path / "gt", tmp_path / "out"
    inp.mkdir()
    gt.mkdir()
    h, w, F = 20, 28, 7
    g = np.random.default_rng(0)
    payload = g.integers(0, 256, size=(F, R.frame_bytes(h, w, "420")), dtype=np.uint8)
    with y4m.Y4MWriter(str(inp / "clip0.y4m"), w, h, 30, "420", False) as wr:
        wr.write(payload)
    gt_payload = g.integers(0, 256, size=(F, R.frame_bytes(4 * h, 4 * w, "444")), dtype=np.uint8)
    with y4m.Y4MWriter(str(gt / "clip0.y4m"), 4 * w, 4 * h, 30, "444", True) as wr:
        wr.write(gt_payload)
    common = ["--input_dir", str(inp)] + _model_flags(golden_dir)
    cli.main(common + ["--output_path", str(out), "--y4m_save", "--fps", "24", "--save_format", "yuv420p", "--eval_metrics", "psnr,ssim",
                       "--gt_dir", str(gt)])
    raw = (out / "clip0.y4m").read_bytes()
    header = raw[:raw.index(b"\n") + 1]
    assert header == b"YUV4MPEG2 W112 H80 F24:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    fb = R.frame_bytes(80, 112, "420")
    assert len(raw) == len(header) + F * (6 + fb) and not (out / "clip0.npy").exists()
    body = np.frombuffer(raw[len(header):], dtype=np.uint8).reshape(F, 6 + fb)
    assert bytes(body[0, :6]) == b"FRAME\n"
    pred = R.yuv_to_rgb(np.ascontiguousarray(body[:, 6:]), 80, 112, "bt601", "limited", "420", "centre")
    gt_rgb = R.yuv_to_rgb(gt_payload, 80, 112, "bt601", "full", "444")
    want = metrics.clip_metrics(torch.from_numpy(pred), torch.from_numpy(gt_rgb), ["psnr", "ssim"])
    with open(out / "metrics_psnr_ssim.json") as f:
        got = json.load(f)
    assert got["per_sample"] == {"psnr": [want["psnr"]], "ssim": [want["ssim"]]} and got["count"] == 1
    # the same flags without --y4m_save write the frames the Y4M file was converted from ...
    out2 = tmp_path / "out2"
    cli.main(common + ["--output_path", str(out2), "--fps", "24", "--save_format", "yuv420p"])
    frames = np.load(out2 / "clip0.npy")
    assert frames.shape == (F, 80, 112, 3) and raw == y4m_bytes(header, R.rgb_to_yuv(frames, "bt601", "limited", "420"))
    # ... and with --chunk_len the file is streamed chunk by chunk: the bytes of the in-memory run with the same chunks
    chunked = ["--chunk_len", "5", "--overlap_t", "2", "--save_format", "yuv444p", "--yuv_matrix", "bt709", "--yuv_range", "full"]
    out3, out4 = tmp_path / "out3", tmp_path / "out4"
    cli.main(common + ["--output_path", str(out3), "--y4m_save"] + chunked)
    cli.main(common + ["--output_path", str(out4)] + chunked)
    raw3 = (out3 / "clip0.y4m").read_bytes()
    header3 = b"YUV4MPEG2 W112 H80 F16:1 Ip A1:1 C444 XCOLORRANGE=FULL\n"
    assert raw3 == y4m_bytes(header3, R.rgb_to_yuv(np.load(out4 / "clip0.npy"), "bt709", "full", "444"))


def test_cli_npy_run_writes_what_it_wrote_before_this_feature(golden_dir, tmp_path):
    """An .npy run without --y4m_save is untouched: the bytes recorded from the commit before this feature, same flags and seed."""
    from dove_amd import cli
    gold = np.load(os.path.join(golden_dir, "cli_npy_before_y4m.npz"))
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    np.save(inp / "clip0.npy", gold["clip"])
    cli.main(["--input_dir", str(inp), "--output_path", str(out), "--fps", "24", "--save_format", "yuv420p"] + _model_flags(golden_dir))
    assert sorted(p.name for p in out.iterdir()) == ["clip0.npy"]
    got = np.load(out / "clip0.npy")
    assert got.shape == gold["frames"].shape and np.array_equal(got, gold["frames"])
