"""BASELINE configs[2]'s execution mode on the HIP kernels: ONE clip sharded over R ranks - halo-exact VAE (whole frame-batches
per rank at R <= 4; PAIRED PIECES of split frame-batches at R = 8, BASELINE's "frame-chunk = 4") + sequence/head-parallel DiT
(`dove_amd.dist.process_video_sharded`) - played as R processes on the ONE GPU the box has.

RCCL refuses two ranks on one device, so the ranks talk gloo and device tensors cross through host memory
(`dove_amd.dist._isend / _irecv / _all_to_all ...`: same messages, same order as over RCCL); every FLOP runs in the HIP kernels:
R = 8 is the only place where `groupnorm_sums_of` (conv-epilogue partial rows -> fp64 sums -> pair exchange), the
`_piece_role` rule of Upsample3D and the Ulysses DiT at world > 1 execute on a device.  The assert is BIT-IDENTITY with the
single-process `process_video` on every rank.  Reference shard axis: /root/reference/inference_script.py:249-279, 690-703."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F, H, W = 33, 128, 192      # every VAE level keeps >= 16 rows, so the production conv kernel (LDS-halo, fused statistics) runs at each


def _worker(rank, world, port, q):
    import faulthandler
    faulthandler.dump_traceback_later(270, exit=True)      # a stuck rank dumps its stack and exits instead of hanging the box
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dove_amd import config, dist as ddist, ops
        from dove_amd.inference import process_video
        from dove_amd.pipeline import CogVideoXPipeline
        v, t, s = config.small_configs(num_layers=2)
        pipe = CogVideoXPipeline.from_config(v, t, s, seed=21, device=dev, init_device=dev)
        g = torch.Generator().manual_seed(5)
        video = (torch.rand(1, 3, F, H, W, generator=g) * 2 - 1).to(torch.bfloat16).to(dev)
        noise = torch.randn(1, 16, 1 + (F - 1) // 4, H // 8, W // 8, generator=g).to(dev)
        text = torch.randn(226, t["text_embed_dim"], generator=g).to(torch.bfloat16).to(dev)
        ref = process_video(pipe, video, empty_prompt_embedding=text, posterior_noise=noise)
        recs = []
        ops.set_profiler(recs)
        out = ddist.process_video_sharded(pipe, video, empty_prompt_embedding=text, posterior_noise=noise)
        ops.set_profiler(None)
        kernels = sorted({r[4] for r in recs})
        # second pass: the halo plan is known, every receive is pre-posted (irecv) - same bits; then each rank keeps its frames
        again = ddist.process_video_sharded(pipe, video, empty_prompt_embedding=text, posterior_noise=noise)
        mine = ddist.process_video_sharded(pipe, video, empty_prompt_embedding=text, posterior_noise=noise, gather="none")
        torch.cuda.synchronize()
        nf = torch.tensor([0 if mine is None else mine.shape[2]])
        starts = [torch.zeros(1, dtype=torch.long) for _ in range(world)]
        dist.all_gather(starts, nf)
        s0 = int(sum(int(x) for x in starts[:rank]))
        own_ok = mine is None or bool(torch.equal(mine, ref[:, :, s0:s0 + mine.shape[2]]))
        d = (out.float() - ref.float()).abs()
        q.put(dict(rank=rank, equal=bool(torch.equal(out, ref)), again=bool(torch.equal(again, ref)), own=own_ok,
                   frames=int(nf), max_diff=float(d.max()), n_diff=int((d > 0).sum()), kernels=kernels,
                   halo_bytes=int(getattr(pipe.vae, "last_halo_bytes", 0)), finite=bool(torch.isfinite(out).all())))
    except BaseException:
        import traceback
        q.put(dict(rank=rank, error=traceback.format_exc()))
        os._exit(1)                                        # peers blocked on this rank are reaped by their own watchdog / the parent
    dist.barrier()
    dist.destroy_process_group()


def _run(world):
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q), daemon=True) for r in range(world)]
    for p in procs:
        p.start()
    import time
    res, t_end = [], time.time() + 300
    try:
        while time.time() < t_end and any(p.is_alive() for p in procs):
            while not q.empty():
                res.append(q.get())
            if any("error" in r for r in res):
                break
            time.sleep(0.2)
        while not q.empty():
            res.append(q.get())
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
            p.join(5)
    errs = [r for r in res if "error" in r]
    assert not errs, f"rank {errs[0]['rank']} failed:\n{errs[0]['error']}"
    assert all(p.exitcode == 0 for p in procs), f"rank exit codes {[p.exitcode for p in procs]}"
    return sorted(res, key=lambda r: r["rank"])


@pytest.mark.parametrize("world", [2, 4, 8])
def test_process_video_sharded_on_hip_bit_identical(world):
    assert torch.cuda.is_available()
    res = _run(world)
    assert len(res) == world
    print(f"[sharded x{world}] " + " | ".join(f"r{r['rank']}: eq {r['equal']} again {r['again']} own {r['own']} frames {r['frames']} "
                                               f"max|d| {r['max_diff']:.3g} ({r['n_diff']} px)" for r in res))
    assert all(r["finite"] for r in res)
    # the sharded ranks really ran the production kernels (fused GroupNorm statistics come from the LDS-halo conv's epilogue)
    assert any("conv3x3_halo4x_kernel" in r["kernels"] for r in res), res[0]["kernels"]
    assert sum(r["frames"] for r in res) == F, "per-rank frame slices do not add up to the clip"
    if world == 8:      # paired pieces: 5,4,4,4,4,4,4,4 px-frames - every rank decodes some
        assert [r["frames"] for r in res] == [5, 4, 4, 4, 4, 4, 4, 4]
    assert res[0]["halo_bytes"] > 0
    bad = [r for r in res if not (r["equal"] and r["again"] and r["own"])]
    assert not bad, f"sharded result differs from the single-process one on ranks {[r['rank'] for r in bad]}: {bad[0]}"


def _bench_line(env_extra):
    import json
    import subprocess
    env = dict(os.environ, **env_extra)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--oversubscribe", "--layers", "1", "--steps", "1", "--warmup", "1",
           "--frames", "17", "--height", "128", "--width", "192", "--no-variants", "--full"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    return json.loads(lines[0])


def test_bench_single_clip_self_validation():
    """bench.py --gpus N validates its own single-clip (configs[2]) measurement: every rank's decoded frames are compared, by per-frame
    checksums of the raw bits, with the frames of rank 0's one-GPU result of the same clip, and the line carries `single_clip.bit_identical`
    (+ `single_clip_failed` when it is not True).  Exercised here on the debug path (2 ranks as 2 processes on this box's one GPU, gloo
    wires): a clean run reads True; with one bit flipped in rank 1's last frame (DOVE_BENCH_STRONG_FAULT=corrupt:1) the same run reads
    False, names the frame and flags the line.  Shard axis: /root/reference/inference_script.py:249-279, 690-703."""
    d = _bench_line({})
    sc = d["single_clip"]
    print(f"[bench single_clip] clean: bit_identical {sc['bit_identical']} frames per rank {sc['frames_decoded_per_rank']}")
    assert sc["bit_identical"] is True and sc["mismatched_frames"] == [] and "single_clip_failed" not in d, sc
    assert sum(sc["frames_decoded_per_rank"]) == 17 and min(sc["frames_decoded_per_rank"]) > 0
    d = _bench_line({"DOVE_BENCH_STRONG_FAULT": "corrupt:1"})
    sc = d["single_clip"]
    print(f"[bench single_clip] one flipped bit on rank 1: bit_identical {sc['bit_identical']} mismatched frames {sc['mismatched_frames']}")
    assert sc["bit_identical"] is False and sc["mismatched_frames"] == [16] and d.get("single_clip_failed") is True, sc


# ---- BASELINE configs[2] at its REAL size: 33x720x1280, 8 ranks (as 8 processes on the one GPU), full-width VAE, 2-layer DiT -------------
RF, RH, RW = 33, 720, 1280
HALO_L0_128 = 2 * 128 * RH * RW * 2          # 471 859 200 B: the 2-frame halo of a 128-channel conv at full resolution ("472 MB")
HALO_L0_256 = 2 * 256 * RH * RW * 2          # 943 718 400 B: up_blocks.3's first conv reads the 256-channel upsampled tensor ("944 MB")


def _real_inputs(t):
    g = torch.Generator().manual_seed(5)
    video = (torch.rand(1, 3, RF, RH, RW, generator=g) * 2 - 1).to(torch.bfloat16)
    noise = torch.randn(1, 16, 1 + (RF - 1) // 4, RH // 8, RW // 8, generator=g)
    text = torch.randn(226, t["text_embed_dim"], generator=g).to(torch.bfloat16)
    return video, noise, text


def _real_pipe(dev):
    from dove_amd import config
    from dove_amd.pipeline import CogVideoXPipeline
    v, t, s = config.default_configs()                  # the CogVideoX1.5-5B VAE and DiT width; two DiT layers keep 8 processes light
    t["num_layers"] = 2
    return CogVideoXPipeline.from_config(v, t, s, seed=21, device=dev, init_device=dev), t


def _real_worker(rank, world, port, q, ref_path):
    import faulthandler
    faulthandler.dump_traceback_later(560, exit=True)
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dove_amd import dist as ddist
        pipe, t = _real_pipe(dev)
        video, noise, text = (x.to(dev) for x in _real_inputs(t))
        passes = []
        import time
        for _ in range(2):      # pass 1 records the halo plan (blocking receives), pass 2 runs on pre-posted receives only
            torch.cuda.synchronize()
            t0 = time.time()
            mine = ddist.process_video_sharded(pipe, video, empty_prompt_embedding=text, posterior_noise=noise, gather="none")
            torch.cuda.synchronize()
            passes.append(dict(out=mine, s=time.time() - t0, enc=dict(pipe.vae.last_halo_stats_encode), dec=dict(pipe.vae.last_halo_stats_decode)))
        nf = torch.tensor([0 if mine is None else mine.shape[2]])
        counts = [torch.zeros(1, dtype=torch.long) for _ in range(world)]
        dist.all_gather(counts, nf)
        s0 = int(sum(int(x) for x in counts[:rank]))
        ref = torch.load(ref_path)[:, :, s0:s0 + int(nf)].to(dev)
        eq = [bool(p["out"] is not None and torch.equal(p["out"], ref)) for p in passes]
        d = (passes[1]["out"].float() - ref.float()).abs()
        q.put(dict(rank=rank, frames=int(nf), first=s0, equal=eq, max_diff=float(d.max()), n_diff=int((d > 0).sum()),
                   seconds=[p["s"] for p in passes], enc=[p["enc"] for p in passes], dec=[p["dec"] for p in passes],
                   peak_gb=torch.cuda.max_memory_allocated() / 1e9))
    except BaseException:
        import traceback
        q.put(dict(rank=rank, error=traceback.format_exc()))
        os._exit(1)
    dist.barrier()
    dist.destroy_process_group()


def test_process_video_sharded_real_size_8_ranks(tmp_path):
    """configs[2] - 33x720x1280, frame-chunk = 4, 8 ranks - at production size on the HIP kernels (8 processes on this box's one GPU,
    gloo with host-staged wires): every rank's decoded frames (5,4,4,4,4,4,4,4) are BIT-IDENTICAL to the single-process result, on the
    recording pass and on the pre-posted pass; the halo messages are the ones SURVEY.md 8(e) counts (six 472 MB halos in the encoder's
    full-resolution block, eight of 472 MB + one of 944 MB in the decoder's); the second pass fetches EVERY halo from a receive posted
    before the stage started (no blocking receive left).  Shard axis: /root/reference/inference_script.py:249-279, 690-703."""
    import socket
    import time

    import torch.multiprocessing as mp
    from dove_amd.inference import process_video
    dev = torch.device("cuda", 0)
    pipe, t = _real_pipe(dev)
    video, noise, text = (x.to(dev) for x in _real_inputs(t))
    ref = process_video(pipe, video, empty_prompt_embedding=text, posterior_noise=noise)
    assert ref.shape == (1, 3, RF, RH, RW) and bool(torch.isfinite(ref).all())
    ref_path = str(tmp_path / "ref.pt")
    torch.save(ref.cpu(), ref_path)
    del pipe, ref, video, noise, text
    torch.cuda.empty_cache()
    world = 8
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_real_worker, args=(r, world, port, q, ref_path), daemon=True) for r in range(world)]
    t0 = time.time()
    for p in procs:
        p.start()
    res, t_end = [], time.time() + 580
    try:
        while time.time() < t_end and any(p.is_alive() for p in procs):
            while not q.empty():
                res.append(q.get())
            if any("error" in r for r in res):
                break
            time.sleep(0.2)
        while not q.empty():
            res.append(q.get())
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
            p.join(5)
    errs = [r for r in res if "error" in r]
    assert not errs, f"rank {errs[0]['rank']} failed:\n{errs[0]['error']}"
    assert len(res) == world and all(p.exitcode == 0 for p in procs), f"rank exit codes {[p.exitcode for p in procs]}"
    res.sort(key=lambda r: r["rank"])
    print(f"[configs2 real size x8] {time.time() - t0:.0f} s; per rank: " + " | ".join(
        f"r{r['rank']}: frames {r['frames']} eq {r['equal']} pass s {r['seconds'][0]:.1f}/{r['seconds'][1]:.1f} peak {r['peak_gb']:.1f} GB "
        f"enc MB {r['enc'][1]['bytes_sent'] / 1e6:.0f} dec MB {r['dec'][1]['bytes_sent'] / 1e6:.0f}" for r in res))
    assert [r["frames"] for r in res] == [5, 4, 4, 4, 4, 4, 4, 4]
    bad = [r for r in res if not all(r["equal"])]
    assert not bad, f"ranks {[r['rank'] for r in bad]} differ from the single-process result: {bad[0]['max_diff']} ({bad[0]['n_diff']} px)"
    for r in res:
        for stage, n128, n256 in (("enc", 6, 0), ("dec", 8, 1)):
            for k in (0, 1):
                st = r[stage][k]
                if r["rank"] < world - 1:       # every rank but the last hands the halo of each causal conv to its successor
                    assert st["messages"].count(HALO_L0_128) == n128 and st["messages"].count(HALO_L0_256) == n256, (r["rank"], stage, st["messages"])
                    assert st["bytes_sent"] == sum(st["messages"]) == res[0][stage][k]["bytes_sent"]
                else:
                    assert st["bytes_sent"] == 0
            n_halos = len(res[0][stage][0]["messages"])                # one per causal conv of the stage
            if r["rank"] > 0:
                assert r[stage][0]["recv_blocking"] == n_halos and r[stage][0]["recv_preposted"] == 0, (r["rank"], stage, r[stage][0])
                assert r[stage][1]["recv_blocking"] == 0 and r[stage][1]["recv_preposted"] == n_halos, (r["rank"], stage, r[stage][1])
            else:
                assert r[stage][0]["recv_blocking"] == r[stage][1]["recv_preposted"] == 0


# ---- the 42-layer DiT of configs[2] at its real sequence length, 8 ranks (the whole operator at real size keeps a 2-layer DiT: 8 x (11 GB of
# 42-layer weights + 17-20 GB of VAE working set) = 240 GB of this one GPU's 288 GB leaves no margin; the DiT alone is 8 x ~14 GB) --------------
def _dit42_worker(rank, world, port, q, ref_path):
    import faulthandler
    faulthandler.dump_traceback_later(560, exit=True)
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import time
        from dove_amd import config, dist as ddist, weights
        from dove_amd.rope import prepare_rotary_positional_embeddings
        from dove_amd.transformer import CogVideoXTransformer3DModel
        v, t, s = config.default_configs()
        assert t["num_layers"] == 42
        tr = CogVideoXTransformer3DModel(t, weights.LazyStateDict(weights.dit_param_shapes(t), 21, dev), dev)
        hidden, text = _dit42_inputs(t)
        rope = prepare_rotary_positional_embeddings(height=RH, width=RW, num_frames=hidden.shape[0], transformer_config=tr.config,
                                                    vae_scale_factor_spatial=8, device=dev)
        torch.cuda.synchronize()
        t0 = time.time()
        out = ddist.dit_forward_ulysses(tr, hidden.to(dev), text.to(dev), 399, rope)
        torch.cuda.synchronize()
        dt = time.time() - t0
        ref = torch.load(ref_path).to(dev)
        d = (out.float() - ref.float()).abs()
        q.put(dict(rank=rank, equal=bool(torch.equal(out, ref)), max_diff=float(d.max()), n_diff=int((d > 0).sum()), seconds=dt,
                   finite=bool(torch.isfinite(out).all()), peak_gb=torch.cuda.max_memory_allocated() / 1e9))
    except BaseException:
        import traceback
        q.put(dict(rank=rank, error=traceback.format_exc()))
        os._exit(1)
    dist.barrier()
    dist.destroy_process_group()


def _dit42_inputs(t):
    g = torch.Generator().manual_seed(9)
    hidden = torch.randn(10, 16, RH // 8, RW // 8, generator=g).to(torch.bfloat16)      # 9 latent frames + the first-frame copy: N = 18 000 + 226
    text = (torch.randn(226, t["text_embed_dim"], generator=g) * 0.15).to(torch.bfloat16)
    return hidden, text


def test_dit_sharded_42_layers_real_size_8_ranks(tmp_path):
    """The DiT half of configs[2] at FULL depth and the real sequence length: 42 layers, N = 18 226 tokens, 8 ranks (8 processes on this box's one
    GPU, gloo with host-staged wires) - rows of the residual stream sharded for every row-local operator, 6 heads per rank for attention, one
    all-to-all each way per layer (`dove_amd.dist.dit_forward_ulysses`): every rank's velocity is BIT-IDENTICAL to the single-process forward
    (which runs the bounded heads on the pipelined attention kernel and the GEMM row tails on their own kernel - per row and per head the same
    arithmetic whatever the sharding).  Shard axis of the reference: /root/reference/inference_script.py:249-279, 690-703; the op: :483-489."""
    import socket
    import time

    import torch.multiprocessing as mp
    from dove_amd import config, weights
    from dove_amd.rope import prepare_rotary_positional_embeddings
    from dove_amd.transformer import CogVideoXTransformer3DModel
    dev = torch.device("cuda", 0)
    v, t, s = config.default_configs()
    tr = CogVideoXTransformer3DModel(t, weights.LazyStateDict(weights.dit_param_shapes(t), 21, dev), dev)
    hidden, text = _dit42_inputs(t)
    rope = prepare_rotary_positional_embeddings(height=RH, width=RW, num_frames=hidden.shape[0], transformer_config=tr.config,
                                                vae_scale_factor_spatial=8, device=dev)
    ref = tr._forward_one(hidden.to(dev), text.to(dev), 399, rope)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref).all())
    ref_path = str(tmp_path / "ref_dit.pt")
    torch.save(ref.cpu(), ref_path)
    del tr, ref
    torch.cuda.empty_cache()
    world = 8
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dit42_worker, args=(r, world, port, q, ref_path), daemon=True) for r in range(world)]
    t0 = time.time()
    for p in procs:
        p.start()
    res, t_end = [], time.time() + 580
    try:
        while time.time() < t_end and any(p.is_alive() for p in procs):
            while not q.empty():
                res.append(q.get())
            if any("error" in r for r in res):
                break
            time.sleep(0.2)
        while not q.empty():
            res.append(q.get())
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
            p.join(5)
    errs = [r for r in res if "error" in r]
    assert not errs, f"rank {errs[0]['rank']} failed:\n{errs[0]['error']}"
    assert len(res) == world and all(p.exitcode == 0 for p in procs), f"rank exit codes {[p.exitcode for p in procs]}"
    res.sort(key=lambda r: r["rank"])
    print(f"[dit42 x8 real size] {time.time() - t0:.0f} s; per rank: " + " | ".join(
        f"r{r['rank']}: eq {r['equal']} {r['seconds']:.1f} s peak {r['peak_gb']:.1f} GB" for r in res))
    assert all(r["finite"] for r in res)
    bad = [r for r in res if not r["equal"]]
    assert not bad, f"ranks {[r['rank'] for r in bad]} differ from the single-process forward: max |d| {bad[0]['max_diff']} ({bad[0]['n_diff']} values)"
