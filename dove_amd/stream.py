"""Streaming super-resolution of a long clip in bounded memory: ``python -m dove_amd.stream --input IN.y4m|- --output OUT.y4m|-``.

The reference's temporal stitch is a crop: ``tiling.get_valid_tile_region`` keeps half of each overlap and every voxel is written once.
A chunk's valid frames are therefore final as soon as that chunk is done.  ``sr_stream`` runs the chunk x tile loop of ``cli.main`` /
``inference.run_clip`` without ever holding the clip: frames come from a reader, every chunk's valid frames leave through a writer, and
the device holds one chunk of low-resolution input, one chunk of SR output and one chunk of write counts.  Pieces run in the order of the
in-memory loop (chunk-major, tile-minor) from the same generator, so the result is bit-identical to it.

The chunk list equals ``tiling.make_temporal_chunks(F_padded, chunk_len, overlap_t)`` but is produced incrementally (``ChunkPlanner``):
a lookahead of ``2 * chunk_len - overlap_t`` frames from a chunk's start decides whether that chunk is the last one (the next one would
be short and is merged, or the clip ends inside it).

    ffmpeg -i in.mkv -f yuv4mpegpipe - | python -m dove_amd.stream --input - --output - ... | ffmpeg -i - out.mkv

``--graph`` runs the same stream through the library's whole-video session (``graph.VideoSession``; include/dove_hip.h ``dove_video_*``):
the reader and writer threads stay, the chunk x tile loop, the noise (``dove_randn`` seeded by ``--seed``), the stitch, the colour fix and
the conversions run inside libdove_hip.so - what a C host gets from the same calls.
"""
from __future__ import annotations

import queue
import sys
import threading

import torch

from . import ops, prepost, tiling
from . import yuv as yuvmod
from .inference import process_video

_POLL = 0.1                                     # seconds a blocked queue operation waits before it looks at the other threads' state


def lookahead(chunk_len: int, overlap_t: int) -> int:
    """Frames from a chunk's start that must be known (or the end of the clip) to decide whether the chunk is the last one."""
    return 2 * chunk_len - overlap_t


class ChunkPlanner:
    """``tiling.make_temporal_chunks`` one chunk at a time, without the frame count up front.

    ``need()`` is the number of frames that must be known to exist before ``next(known, eof)`` may be called without ``eof``;
    ``next`` returns ``(t0, t1, last)`` or None when no chunk is left.  ``known`` is the number of frames known so far, the total once
    ``eof`` is set.  ``chunk_len == 0`` is one chunk of the whole clip, which needs the end of the stream."""

    def __init__(self, chunk_len: int, overlap_t: int = 8):
        if chunk_len != 0 and chunk_len - overlap_t <= 0:
            raise ValueError("chunk_len must be greater than overlap")
        self.chunk_len, self.overlap_t = chunk_len, overlap_t if chunk_len else 0
        self.start, self.done = 0, False

    def need(self):
        return None if self.chunk_len == 0 else self.start + lookahead(self.chunk_len, self.overlap_t)

    def next(self, known: int, eof: bool):
        if self.done:
            return None
        s, n, ov = self.start, self.chunk_len, self.overlap_t
        if n == 0:
            if not eof:
                raise RuntimeError("chunk_len == 0 is one piece of the whole clip: the planner needs the end of the stream")
            self.done = True
            return (0, known, True)
        if not eof:
            if known < s + lookahead(n, ov):
                raise RuntimeError(f"the chunk at {s} needs {s + lookahead(n, ov)} known frames or the end of the stream, got {known}")
            chunk = (s, s + n, False)
        elif s == 0 and known <= ov:
            self.done = True                                        # make_temporal_chunks returns no chunk at all
            return None
        elif known <= s + n or known - (s + n - ov) < n:            # the clip ends inside it / the next chunk is short and merged
            chunk = (s, known, True)
        else:
            chunk = (s, s + n, False)
        self.start, self.done = s + n - ov, chunk[2]
        return chunk


def output_size(h: int, w: int, upscale: int, crop_scale: int = 4):
    """(H, W) of the frames written for h x w input: padded to x16, upscaled, and ``pad * crop_scale`` removed (the reference's
    hard-coded 4, ref :731)."""
    _, pad_h, pad_w = tiling.match_padding(1, h, w)
    return (h + pad_h) * upscale - pad_h * crop_scale, (w + pad_w) * upscale - pad_w * crop_scale


class FrameSource:
    """A clip that is already in memory ([F,H,W,3] uint8) behind the reader interface of ``sr_stream``."""

    def __init__(self, frames_u8: torch.Tensor):
        self.frames, self.pos = frames_u8, 0
        self.height, self.width = frames_u8.shape[1:3]

    def read(self, n: int) -> torch.Tensor:
        out = self.frames[self.pos:self.pos + n]
        self.pos += out.shape[0]
        return out


class _Worker(threading.Thread):
    """A thread whose exception is kept for the main thread."""

    def __init__(self, fn, name):
        super().__init__(name=name, daemon=True)
        self.fn, self.error = fn, None

    def run(self):
        try:
            self.fn()
        except BaseException as e:                                   # noqa: BLE001 - re-raised on the main thread
            self.error = e


def _get(q: queue.Queue, worker: _Worker, what: str):
    """q.get() that ends with the worker's error instead of waiting for a thread that died."""
    while True:
        try:
            return q.get(timeout=_POLL)
        except queue.Empty:
            if worker.error is not None:
                raise worker.error
            if not worker.is_alive() and q.empty():
                raise RuntimeError(f"the {what} thread ended without a result")


def _log(msg: str):
    print(msg, file=sys.stderr, flush=True)


def _geometry(reader, writer, upscale, chunk_len, overlap_t, yuv_matrix, yuv_range):
    """What both streaming loops start from -> ((H, W, pad_h, pad_w), (Ho, Wo), in_fmt, out_fmt, ov_t, block).  ``in_fmt`` is None for
    a reader of RGB frames; ``block`` is the number of frames the reader thread asks for at a time."""
    H, W = reader.height, reader.width
    in_fmt = yuvmod.format_of_reader(reader, yuv_matrix, yuv_range) if hasattr(reader, "chroma") else None
    out_fmt = yuvmod.YuvFormat(writer.chroma, yuv_matrix, "full" if writer.full_range else "limited")
    _, pad_h, pad_w = tiling.match_padding(1, H, W)
    Ho, Wo = output_size(H, W, upscale)
    if (writer.height, writer.width) != (Ho, Wo):
        raise ValueError(f"the writer is {writer.width}x{writer.height}; {W}x{H} input at x{upscale} gives {Wo}x{Ho} frames")
    ov_t = overlap_t if chunk_len > 0 else 0
    block = max(chunk_len - ov_t, 1) if chunk_len > 0 else 32
    return (H, W, pad_h, pad_w), (Ho, Wo), in_fmt, out_fmt, ov_t, block


class _StreamIO:
    """The threads and buffers around a streaming loop, as a context manager.  A reader thread prefetches blocks of frames into a bounded
    queue; a writer thread writes from two pinned buffers, which D2H copies on a side stream fill.  Entering starts the threads; leaving
    ends them, and their errors surface unless the body already failed."""

    def __init__(self, reader, writer, block, dev, join_timeout):
        self.reader, self.writer, self.block, self.dev, self.join_timeout = reader, writer, block, dev, join_timeout
        self.stop = threading.Event()
        self.in_q: queue.Queue = queue.Queue(maxsize=2)
        self.out_q: queue.Queue = queue.Queue(maxsize=2)
        self.free_q: queue.Queue = queue.Queue()
        self.side = torch.cuda.Stream(device=dev)
        self.pinned, self.keep = [None, None], [None, None]
        for i in range(2):
            self.free_q.put(i)
        self.rd, self.wr = _Worker(self.read_loop, "dove-stream-reader"), _Worker(self.write_loop, "dove-stream-writer")

    def put(self, q, item):
        while not self.stop.is_set():
            try:
                q.put(item, timeout=_POLL)
                return True
            except queue.Full:
                pass
        return False

    def read_loop(self):
        while not self.stop.is_set():
            blk = self.reader.read(self.block)
            if blk.shape[0] and not self.put(self.in_q, blk):
                return
            if blk.shape[0] < self.block:
                self.put(self.in_q, None)                           # end of the stream
                return

    def write_loop(self):
        while True:
            item = self.out_q.get()
            if item is None:
                return
            i, k, event = item
            event.synchronize()
            self.writer.write(self.pinned[i][:k])
            self.free_q.put(i)

    def __enter__(self):
        self.rd.start()
        self.wr.start()
        return self

    def __exit__(self, exc_type, exc, tb):
        """End the reader and writer threads; their errors surface unless the run already failed."""
        failed, rd, wr = exc_type is not None, self.rd, self.wr
        self.stop.set()
        while wr.is_alive():                                         # the sentinel goes in even when the queue is full of unwritten items
            try:
                self.out_q.put(None, timeout=_POLL)
                break
            except queue.Full:
                if failed:
                    try:
                        self.out_q.get_nowait()
                    except queue.Empty:
                        pass
        while rd.is_alive():                                         # a reader blocked on a full queue sees `stop` within _POLL
            try:
                self.in_q.get_nowait()
            except queue.Empty:
                pass
            rd.join(_POLL)
            if failed:
                break                                                # it may be blocked in read() on a pipe: a daemon thread, not waited for
        wr.join(self.join_timeout)
        rd.join(_POLL if failed else self.join_timeout)
        self.keep = [None, None]                # this object and its threads' targets form a cycle: device memory does not wait for the collector
        hung = [t.name for t in (rd, wr) if t.is_alive()]
        if not failed:
            for t in (wr, rd):
                if t.error is not None:
                    raise t.error
            if hung:
                raise RuntimeError(f"threads still running after {self.join_timeout} s: {', '.join(hung)}")

    def next_block(self):
        """The next block of frames, None at the end of the stream."""
        return _get(self.in_q, self.rd, "reader")

    def acquire(self) -> int:
        """Index of a pinned buffer; the writer hands a buffer back after its copy has completed."""
        return _get(self.free_q, self.wr, "writer")

    def release(self, i: int):
        """Hand back an index that was acquired but not emitted."""
        self.free_q.put(i)

    def emit(self, i: int, payload: torch.Tensor, k: int, keep=None):
        """Copy ``payload[:k]`` ([k, bytes] uint8 on the device) into pinned buffer ``i`` on the side stream and queue it for the writer."""
        if self.pinned[i] is None or self.pinned[i].shape[0] < k:
            self.pinned[i] = torch.empty(k, payload.shape[1], dtype=torch.uint8, pin_memory=True)
        self.side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.side):
            self.pinned[i][:k].copy_(payload[:k], non_blocking=True)
            event = torch.cuda.Event()
            event.record(self.side)
        # ``keep`` lives until buffer i comes round again (two chunks later): its release then depends on the chunk order alone, not on
        # when the side stream happened to finish
        self.keep[i] = keep
        while True:                                                  # a full queue stalls this thread, not the GPU
            if self.wr.error is not None:
                raise self.wr.error
            try:
                self.out_q.put((i, k, event), timeout=_POLL)
                return
            except queue.Full:
                pass


@torch.no_grad()
def sr_stream(pipe, reader, writer, *, upscale: int = 4, upscale_mode: str = "bilinear", chunk_len: int = 0, overlap_t: int = 8,
              tile_size_hw=(0, 0), overlap_hw=(32, 32), noise_step: int = 0, sr_noise_step: int = 399, prompt: str = "",
              empty_prompt_embedding=None, color_fix: str | None = None, generator=None, yuv_matrix: str = "bt601",
              yuv_range: str | None = None, join_timeout: float = 60.0, log=_log) -> dict:
    """Super-resolve the frames of ``reader`` into ``writer`` chunk by chunk.

    ``reader``: a ``y4m.Y4MReader`` (payloads are converted with ``yuv.yuv_to_rgb``; ``yuv_range`` overrides its range tag) or any object
    with ``read(n) -> [k,H,W,3] uint8``, ``height`` and ``width`` (``FrameSource``).  ``writer``: a ``y4m.Y4MWriter`` of
    ``output_size(height, width, upscale)``; its chroma layout and range, with ``yuv_matrix``, are the output format.
    Returns {"frames", "chunks", "pieces"}."""
    dev = pipe.vae.device
    (H, W, pad_h, pad_w), (Ho, Wo), in_fmt, out_fmt, ov_t, block = _geometry(reader, writer, upscale, chunk_len, overlap_t, yuv_matrix, yuv_range)
    Hs, Ws = (H + pad_h) * upscale, (W + pad_w) * upscale
    ov_hw = tuple(overlap_hw) if tuple(tile_size_hw) != (0, 0) else (0, 0)
    tiles = tiling.make_spatial_tiles(Hs, Ws, tuple(tile_size_hw), ov_hw)
    planner = ChunkPlanner(chunk_len, ov_t)
    if chunk_len == 0:
        log("[dove_amd.stream] --chunk_len 0 is one piece: the whole stream is read before anything is written (memory grows with the "
            "clip; set --chunk_len for bounded memory)")

    frames, base, total, eof, last_frame = [], 0, 0, False, None      # host frames [base, total) of the stream
    stats = {"frames": 0, "chunks": 0, "pieces": 0}
    with _StreamIO(reader, writer, block, dev, join_timeout) as io:
        while True:
            need = planner.need()
            while not eof and (need is None or total < need):
                blk = io.next_block()
                if blk is None:
                    eof = True
                    break
                frames.extend(blk.unbind(0))
                total += blk.shape[0]
                last_frame = frames[-1]
            if eof and total == 0:
                raise ValueError("the input stream holds no frame")
            F = total if eof else None                               # frames of the clip, once known
            Fp = total + tiling.match_padding(total, H, W)[0] if eof else total
            chunk = planner.next(Fp, eof)
            if chunk is None:
                if stats["chunks"] == 0:
                    raise RuntimeError("Error: Lack of write in region !!!")   # no chunk at all: the in-memory coverage check's text
                break
            t0, t1, last = chunk
            # the chunk's low-resolution frames; the padding repeats the last frame (tiling.match_padding)
            lr = torch.stack([frames[t - base] if t < total else last_frame for t in range(t0, t1)]).to(dev, non_blocking=True)
            rgb = yuvmod.yuv_to_rgb(lr, H, W, in_fmt) if in_fmt is not None else lr.contiguous()
            if upscale_mode == "bilinear":
                video = ops.preprocess_u8(rgb, 0, pad_h, pad_w, upscale, torch.bfloat16)[None]
            else:
                video = prepost.preprocess_frames_torch(rgb, 0, pad_h, pad_w, upscale, upscale_mode, torch.bfloat16)[None]
            del lr, rgb
            out = torch.zeros(video.shape, dtype=torch.bfloat16, device=dev)
            wc = torch.zeros(video.shape, dtype=torch.int32, device=dev)
            # "is the last chunk" is all get_valid_tile_region asks of the clip's length
            clip_shape = (1, 3, t1 if last else t1 + 1, Hs, Ws)
            for (h0, h1, w0, w1) in tiles:
                r = tiling.get_valid_tile_region(t0, t1, h0, h1, w0, w1, clip_shape, ov_t, ov_hw[0], ov_hw[1])
                piece = process_video(pipe, video[:, :, :, h0:h1, w0:w1], prompt=prompt, noise_step=noise_step,
                                      sr_noise_step=sr_noise_step, empty_prompt_embedding=empty_prompt_embedding, generator=generator)
                local = dict(r, out_t_start=r["out_t_start"] - t0, out_t_end=r["out_t_end"] - t0)
                tiling.stitch(out, wc, piece, local)
                del piece
                stats["pieces"] += 1
            a, b = r["valid_t_start"], r["valid_t_end"]              # the same for every tile of the chunk
            tiling.check_coverage(wc[:, :, a:b])
            del wc
            if F is not None:
                b = min(b, F - t0)                                   # minus the padded tail
            if b > a:
                if color_fix:
                    from . import colorfix
                    content = out[0, :, a:b, :Ho, :Wo].permute(1, 0, 2, 3)
                    style = video[0, :, a:b, :Ho, :Wo].permute(1, 0, 2, 3)
                    fixed = colorfix.color_fix(content, style, color_fix, out_dtype=torch.uint8, style_affine=(0.5, 0.5))
                    payload = yuvmod.rgb_to_yuv(fixed, out_fmt)
                    del fixed, content, style
                else:
                    payload = yuvmod.rgb_to_yuv(out[0, :, a:b], out_fmt, crop=(b - a, Ho, Wo))
                # the buffer is asked for only now, so that the GPU has worked on this chunk while the last one was being written
                io.emit(io.acquire(), payload, b - a, keep=payload)
                del payload
                stats["frames"] += b - a
            del out, video
            stats["chunks"] += 1
            log(f"[dove_amd.stream] chunk {stats['chunks']}: frames {t0}..{t1 - 1}{' (last)' if last else ''}, "
                f"{stats['frames']} frames written")
            drop = min(planner.start, total) - base                  # frames before the next chunk's start are done with
            if drop > 0:
                del frames[:drop]
                base += drop
            if last:
                break
    writer.flush()
    return stats


def build_graph(args):
    """The graph-level context the model flags of ``cli.add_model_arguments`` describe -> (GraphContext, empty-prompt embedding,
    scheduler).  The weights are the ones ``cli.build_pipe`` gives the pipeline (the same checkpoint, or the same seeded random init)."""
    import os

    from safetensors.torch import load_file

    from . import cli, config, weights
    from .graph import GraphContext
    from .scheduler import CogVideoXDPMScheduler
    cli.check_dtype(args)
    if args.lora_path:
        raise ValueError("--graph: --lora_path is fused into the Python pipeline's transformer; fuse it into the checkpoint first")
    if not os.path.exists(args.prompt_embedding):
        raise FileNotFoundError(f"empty-prompt embedding not found at {args.prompt_embedding} (the reference ships it; ref :668-676)")
    emb = load_file(args.prompt_embedding)["prompt_embedding"]
    if args.random_init or not args.model_path:
        v, t, s = config.default_configs()
        if args.num_layers:
            t["num_layers"] = args.num_layers
        vsd = weights.LazyStateDict(weights.vae_param_shapes(v), device="cuda")
        tsd = weights.LazyStateDict(weights.dit_param_shapes(t), device="cuda")
    else:
        import json
        v, vsd = weights.load_component(os.path.join(args.model_path, "vae"), weights.vae_param_shapes)
        t, tsd = weights.load_component(os.path.join(args.model_path, "transformer"), weights.dit_param_shapes)
        with open(os.path.join(args.model_path, "scheduler", "scheduler_config.json")) as f:
            s = {k: val for k, val in json.load(f).items() if not k.startswith("_")}
    ctx = GraphContext(v, t, vsd, tsd, "cuda")
    if args.is_vae_st:
        ctx.enable_tiling()
    return ctx, emb, CogVideoXDPMScheduler(**dict(s, timestep_spacing="trailing"))


@torch.no_grad()
def sr_stream_graph(ctx, scheduler, reader, writer, text, *, upscale: int = 4, chunk_len: int = 0, overlap_t: int = 8, tile_size_hw=(0, 0),
                    overlap_hw=(32, 32), noise_step: int = 0, sr_noise_step: int = 399, color_fix: str | None = None, seed: int = 0,
                    yuv_matrix: str = "bt601", yuv_range: str | None = None, max_frames: int = 256, join_timeout: float = 60.0,
                    log=_log) -> dict:
    """``sr_stream`` with the SR loop inside the library: frames from ``reader`` are pushed into a ``graph.VideoSession`` as the planner
    asks for them, every step's frames leave through ``writer``.  The same reader / writer threads, queues and pinned double buffers.
    ``max_frames`` bounds the clip only with ``chunk_len == 0`` (one piece of the whole clip, sized when the session opens)."""
    from .graph import VideoSession
    dev = ctx.device
    (H, W, pad_h, pad_w), _, in_fmt, out_fmt, _, block = _geometry(reader, writer, upscale, chunk_len, overlap_t, yuv_matrix, yuv_range)
    sa, s1 = scheduler._coeffs(torch.tensor([sr_noise_step]), torch.bfloat16)
    pre = (noise_step,) + tuple(scheduler._coeffs(torch.tensor([noise_step]), torch.bfloat16)) if noise_step else None
    if chunk_len == 0:
        log(f"[dove_amd.stream] --chunk_len 0 is one piece: the whole stream is read before anything is written, and the session is "
            f"sized for {max_frames} frames (memory grows with the clip; set --chunk_len for bounded memory)")
    sess = VideoSession(ctx, W, H, text, sr_noise_step, sa, s1, upscale=upscale, chunk_len=chunk_len, overlap_t=overlap_t,
                        tile_size_hw=tuple(tile_size_hw), overlap_hw=tuple(overlap_hw), color_fix=color_fix, in_fmt=in_fmt, out_fmt=out_fmt,
                        noise_step=pre, seed=seed, max_frames=max_frames if chunk_len == 0 else 0, max_push=block)

    stats = {"frames": 0, "chunks": 0, "pieces": 0}
    total, eof = 0, False
    n_tiles = len(tiling.make_spatial_tiles((H + pad_h) * upscale, (W + pad_w) * upscale, tuple(tile_size_hw),
                                            tuple(overlap_hw) if tuple(tile_size_hw) != (0, 0) else (0, 0)))
    payloads = [None, None]                                          # one persistent device buffer per pinned buffer: a step writes into it
    try:
        with _StreamIO(reader, writer, block, dev, join_timeout) as io:
            while not sess.done:
                need = sess.need()
                while not eof and (need is None or need > 0):
                    blk = io.next_block()
                    if blk is None:
                        eof = True
                        sess.end()
                        break
                    sess.push(blk.to(dev, non_blocking=True))
                    total += blk.shape[0]
                    need = sess.need()
                if eof and total == 0:
                    raise ValueError("the input stream holds no frame")
                i = io.acquire()                                     # before the step: it writes into this index's device buffer
                if payloads[i] is None:
                    payloads[i] = torch.empty(sess.max_step_frames, sess.out_frame_bytes, dtype=torch.uint8, device=dev)
                got = sess.step(payloads[i])
                k = got.shape[0]
                stats["chunks"] += 1
                stats["pieces"] += n_tiles
                if k > 0:
                    io.emit(i, got, k)
                    stats["frames"] += k
                else:
                    io.release(i)
                log(f"[dove_amd.stream] chunk {stats['chunks']}{' (last)' if sess.done else ''}: {stats['frames']} frames written")
    finally:                                                         # after the threads have ended
        torch.cuda.synchronize(dev)
        sess.close()
    writer.flush()
    return stats


def main(argv=None):
    import argparse
    import contextlib
    import os

    from . import cli, y4m
    ap = argparse.ArgumentParser(description="Streaming VSR using DOVE on MI355X: Y4M in, Y4M out, bounded memory (dove_amd)")
    ap.add_argument("--input", type=str, required=True, help="a .y4m file, or - for stdin (ffmpeg -f yuv4mpegpipe -)")
    ap.add_argument("--output", type=str, required=True, help="a .y4m file, or - for stdout; then every message goes to stderr")
    ap.add_argument("--prompt", type=str, default="")
    ap.add_argument("--graph", action="store_true",
                    help="run the SR loop inside libdove_hip.so (the whole-video session of the graph level, INTEGRATION.md 1e); "
                         "--seed then seeds the library's own generator (dove_randn), --upscale_mode must be bilinear")
    ap.add_argument("--max_frames", type=int, default=256, help="--graph with --chunk_len 0: the longest clip the session is sized for")
    cli.add_model_arguments(ap)
    ap.set_defaults(fps=None)                                        # the input's frame rate unless --fps is given
    args = ap.parse_args(argv)
    if args.graph and args.upscale_mode != "bilinear":
        ap.error(f"--graph upscales with the library's bilinear kernel; --upscale_mode {args.upscale_mode} needs the Python loop")
    if args.graph and args.prompt:
        ap.error("--graph runs the empty prompt (the cached embedding); a prompt needs the Python loop's text encoder")
    to_stdout = args.output == "-"
    sink = None
    if to_stdout:
        # nothing but the Y4M bytes may reach stdout: keep the real stdout for the writer and point descriptor 1 at stderr, so that
        # a print of any library - Python or native - lands in the log
        sys.stdout.flush()
        sink = os.fdopen(os.dup(1), "wb")
        os.dup2(2, 1)
    with contextlib.redirect_stdout(sys.stderr):
        chroma = yuvmod.save_format_to_chroma(args.save_format)
        if args.graph:
            ctx, emb, scheduler = build_graph(args)
        else:
            pipe, emb = cli.build_pipe(args)
        reader = y4m.Y4MReader(sys.stdin.buffer if args.input == "-" else args.input)
        Ho, Wo = output_size(reader.height, reader.width, args.upscale)
        fps = (args.fps, 1) if args.fps else reader.fps if reader.fps[0] > 0 and reader.fps[1] > 0 else (16, 1)
        writer = y4m.Y4MWriter(sink if to_stdout else args.output, Wo, Ho, fps, chroma, args.yuv_range == "full")
        _log(f"[dove_amd.stream] {reader.width}x{reader.height} {reader.tag} -> {Wo}x{Ho} {y4m.WRITE_TAGS[chroma]} "
             f"({args.yuv_matrix}, {args.yuv_range or 'limited'}), {fps[0]}:{fps[1]} fps")
        try:
            if args.graph:
                stats = sr_stream_graph(ctx, scheduler, reader, writer, emb, upscale=args.upscale, chunk_len=args.chunk_len,
                                        overlap_t=args.overlap_t, tile_size_hw=tuple(args.tile_size_hw), overlap_hw=tuple(args.overlap_hw),
                                        noise_step=args.noise_step, sr_noise_step=args.sr_noise_step,
                                        color_fix=None if args.color_fix == "none" else args.color_fix, seed=args.seed,
                                        yuv_matrix=args.yuv_matrix, yuv_range=args.yuv_range, max_frames=args.max_frames)
            else:
                stats = sr_stream(pipe, reader, writer, upscale=args.upscale, upscale_mode=args.upscale_mode, chunk_len=args.chunk_len,
                                  overlap_t=args.overlap_t, tile_size_hw=tuple(args.tile_size_hw), overlap_hw=tuple(args.overlap_hw),
                                  noise_step=args.noise_step, sr_noise_step=args.sr_noise_step, prompt=args.prompt,
                                  empty_prompt_embedding=emb, color_fix=None if args.color_fix == "none" else args.color_fix,
                                  yuv_matrix=args.yuv_matrix, yuv_range=args.yuv_range)
        finally:
            reader.close()
            writer.close()
        _log(f"[dove_amd.stream] done: {stats['frames']} frames in {stats['chunks']} chunks ({stats['pieces']} pieces)")
    return stats


if __name__ == "__main__":
    main()
