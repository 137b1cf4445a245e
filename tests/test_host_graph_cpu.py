"""CPU check of the HOST graphs (no HIP involved): dove_amd's VAE / DiT / process_video orchestration with
dove_amd.ops replaced by the torch emulation of the operators (tests/emu_ops.py) must reproduce the oracle.
This pins frame-batching + conv caches, SpatialNorm frame maps, upsample/downsample geometry, weight packing,
AdaLN chunk regrouping, row classes, patchify order and the scheduler before any GPU time is spent."""
import os

import pytest
import torch

import emu_ops
from dove_amd import config, weights
from dove_amd.inference import process_video, run_clip
from dove_amd.pipeline import CogVideoXPipeline
from oracle import dit as odit
from oracle.vae import OracleVAE


def psnr(a, b):
    mse = ((a.float() - b.float()) ** 2).flatten(2).mean(dim=-1) if a.dim() > 2 else ((a.float() - b.float()) ** 2).mean()
    return float((10 * torch.log10(1.0 / (mse + 1e-8))).mean())


@pytest.fixture()
def tiny(monkeypatch):
    emu_ops.install(monkeypatch)
    v, t, s = config.tiny_configs()
    pipe = CogVideoXPipeline.from_config(v, t, s, seed=7, device="cpu")
    wv = weights.random_state_dict(weights.vae_param_shapes(v), 7)
    wt = weights.random_state_dict(weights.dit_param_shapes(t), 7)
    return pipe, (v, t, s), wv, wt


def rel(a, b):
    return float((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12))


@pytest.mark.parametrize("F,H,W", [(9, 32, 48), (17, 32, 32), (1, 32, 32), (5, 48, 32)])
def test_vae_encode_decode_vs_oracle(tiny, F, H, W):
    pipe, (v, t, s), wv, wt = tiny
    torch.manual_seed(0)
    x = torch.randn(1, 3, F, H, W).clamp(-1, 1)
    ov = OracleVAE(v, wv)
    p_ref = ov.encode(x)
    p = pipe.vae.encode(x.to(torch.bfloat16)).latent_dist.parameters
    assert p.shape == p_ref.shape
    assert rel(p, p_ref) < 0.06
    z = torch.randn(1, 16, p.shape[2], H // 8, W // 8)
    d_ref = ov.decode(z)
    d = pipe.vae.decode(z.to(torch.bfloat16)).sample
    assert d.shape == d_ref.shape
    if F % 8 == 1:
        assert d.shape == (1, 3, F, H, W)
    assert rel(d, d_ref) < 0.06


def test_dit_vs_oracle(tiny):
    pipe, (v, t, s), wv, wt = tiny
    torch.manual_seed(1)
    hidden = torch.randn(1, 4, 16, 8, 12)
    text = torch.randn(1, 226, t["text_embed_dim"])
    rope = odit.rope_3d(64, 2, 4, 6)
    ts = torch.tensor([399])
    ref = odit.OracleDiT(t, wt).forward(hidden, text, ts, rope)
    got = pipe.transformer(hidden_states=hidden.to(torch.bfloat16), encoder_hidden_states=text.to(torch.bfloat16),
                           timestep=ts, image_rotary_emb=rope, return_dict=False)[0]
    assert got.shape == ref.shape
    assert rel(got, ref) < 0.05


def test_rope_tables_match_oracle():
    from dove_amd.rope import get_3d_rotary_pos_embed
    c, s = get_3d_rotary_pos_embed(64, None, (45, 80), 5, grid_type="slice", max_size=(45, 80))
    rc, rs = odit.rope_3d(64, 5, 45, 80)
    assert c.shape == (18000, 64) and torch.equal(c, rc) and torch.equal(s, rs)


def test_scheduler_constants():
    from dove_amd.scheduler import CogVideoXDPMScheduler
    _, _, s = config.default_configs()
    sch = CogVideoXDPMScheduler.from_config(s, timestep_spacing="trailing")
    assert torch.allclose(sch.alphas_cumprod, odit.alphas_cumprod(s))
    assert abs(float(sch.alphas_cumprod[399]) - 0.3935440575) < 1e-6
    t = torch.tensor([399])
    assert sch._coeffs(t, torch.bfloat16) == (0.625, 0.78125)                # bf16 cast before sqrt (8a row 9)
    a, b = sch._coeffs(t, torch.float32)
    assert abs(a - 0.6273309) < 1e-6 and abs(b - 0.7787528) < 1e-6
    s3 = dict(s, snr_shift_scale=3.0)
    assert abs(float(CogVideoXDPMScheduler(**s3).alphas_cumprod[399]) - 0.17861523) < 1e-6


def test_process_video_vs_oracle(tiny, golden_dir):
    pipe, (v, t, s), wv, wt = tiny
    torch.manual_seed(2)
    F, H, W = 9, 32, 48
    video = torch.rand(1, 3, F, H, W) * 2 - 1
    noise = torch.randn(1, 16, 3, H // 8, W // 8)
    text = torch.randn(226, t["text_embed_dim"]).to(torch.bfloat16)
    got = process_video(pipe, video, empty_prompt_embedding=text, posterior_noise=noise)
    ref32 = odit.process_video(OracleVAE(v, wv), odit.OracleDiT(t, wt), s, video, text.float()[None], noise)
    refbf = odit.process_video(OracleVAE(v, wv, torch.bfloat16), odit.OracleDiT(t, wt, torch.bfloat16), s, video,
                               text[None], noise)
    assert got.shape == ref32.shape == (1, 3, F, H, W)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    p_got, p_bf = psnr(got, ref32), psnr(refbf.float(), ref32)
    # the fused-kernel rounding points must be at least as close to fp32 as the reference's bf16 path (minus 0.05 dB)
    assert p_got >= p_bf - 0.05, (p_got, p_bf)
    assert p_got > 30.0, p_got


def test_run_clip_chunks_cover_and_match_single_calls(tiny):
    pipe, (v, t, s), wv, wt = tiny
    torch.manual_seed(3)
    video = torch.rand(1, 3, 33, 16, 48) * 2 - 1
    text = torch.randn(226, t["text_embed_dim"]).to(torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    out, wc = run_clip(pipe, video, chunk_len=17, overlap_t=8, tile_size_hw=(16, 32), overlap_hw=(0, 16), empty_prompt_embedding=text, generator=g)
    from dove_amd import tiling
    tiling.check_coverage(wc)
    assert out.shape == video.shape and float(out.min()) >= 0 and float(out.max()) <= 1


def test_tokenizer_path_is_loud(tiny):
    pipe = tiny[0]
    with pytest.raises(NotImplementedError):
        process_video(pipe, torch.zeros(1, 3, 1, 16, 16), prompt="a cat")


def test_ops_fail_loudly_without_gpu():
    """No CPU fallback in the product: real ops refuse host tensors."""
    from dove_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.avgpool_time(torch.zeros(2, 4, 4, 32, dtype=torch.bfloat16))


def test_vae_tiling_vs_oracle(monkeypatch):
    """enable_tiling(): tile loop, in-place neighbour blending and crops reproduce the oracle's tiled_encode/tiled_decode."""
    emu_ops.install(monkeypatch)
    v, t, s = config.tiny_configs()
    v["sample_height"], v["sample_width"] = 96, 160          # tiles 48x80 px (latent 6x10), strides 40x64
    pipe = CogVideoXPipeline.from_config(v, t, s, seed=9, device="cpu")
    ov = OracleVAE(v, weights.random_state_dict(weights.vae_param_shapes(v), 9))
    torch.manual_seed(4)
    x = torch.randn(1, 3, 17, 120, 192).clamp(-1, 1)        # 17 frames = two frame-batches: the per-tile conv caches are used
    pipe.vae.enable_tiling()
    pipe.vae.enable_slicing()
    assert pipe.vae.tile_batching                            # 3 x 3 tiles in 4 shape classes (4, 2, 2, 1 tiles) = 4 batched passes
    p = pipe.vae.encode(x.to(torch.bfloat16)).latent_dist.parameters
    p_ref = ov.encode(x, tiling=True)
    assert p.shape == p_ref.shape == (1, 32, 5, 15, 24)
    assert rel(p, p_ref) < 0.06
    assert rel(p_ref, ov.encode(x)) > 0.2                    # tiling really changes the numbers (GroupNorm scope)
    z = torch.randn(1, 16, 5, 15, 24)
    d = pipe.vae.decode(z.to(torch.bfloat16)).sample
    d_ref = ov.decode(z, tiling=True)
    assert d.shape == d_ref.shape == (1, 3, 17, 120, 192)
    assert rel(d, d_ref) < 0.06
    # one tile at a time (the round-3 loop) gives the same bits: batching only changes how many tiles share a launch
    pipe.vae.tile_batching = False
    assert torch.equal(p, pipe.vae.encode(x.to(torch.bfloat16)).latent_dist.parameters)
    assert torch.equal(d, pipe.vae.decode(z.to(torch.bfloat16)).sample)
    pipe.vae.tile_batching = True
    pipe.vae.tile_batch_max = 3                              # a class of 4 tiles then runs as batches of 3 + 1: same bits again
    assert torch.equal(p, pipe.vae.encode(x.to(torch.bfloat16)).latent_dist.parameters)
    # below the tile threshold the tiled flag is a no-op, like diffusers
    small = torch.randn(1, 3, 5, 48, 80).clamp(-1, 1)
    assert rel(pipe.vae.encode(small.to(torch.bfloat16)).latent_dist.parameters, ov.encode(small)) < 0.06


def test_vae_single_frame_batches_vs_oracle(monkeypatch):
    """Frame-batches of ONE frame: every batch after the first is shorter than the causal convs' two-frame halo, so each cache entry is
    the previous entry slid by one frame (`_cconv`'s short-batch branch) - per instance when tiles run as one batch."""
    emu_ops.install(monkeypatch)
    v, t, s = config.tiny_configs()
    v["num_sample_frames_batch_size"] = v["num_latent_frames_batch_size"] = 1
    pipe = CogVideoXPipeline.from_config(v, t, s, seed=7, device="cpu")
    ov = OracleVAE(v, weights.random_state_dict(weights.vae_param_shapes(v), 7))
    torch.manual_seed(5)
    for T in (1, 2, 3):
        z = torch.randn(1, 16, T, 4, 6)
        d, d_ref = pipe.vae.decode(z.to(torch.bfloat16)).sample, ov.decode(z)
        assert d.shape == d_ref.shape
        assert rel(d, d_ref) < 0.06, T
    x = torch.randn(1, 3, 3, 32, 48).clamp(-1, 1)
    p, p_ref = pipe.vae.encode(x.to(torch.bfloat16)).latent_dist.parameters, ov.encode(x)
    assert p.shape == p_ref.shape
    assert rel(p, p_ref) < 0.06
    # the same short batches inside spatial tiles: a batch of tiles slides every instance's window like the tile-by-tile loop does
    v["sample_height"], v["sample_width"] = 32, 48
    pipe = CogVideoXPipeline.from_config(v, t, s, seed=7, device="cpu")
    pipe.vae.enable_tiling()
    z = torch.randn(1, 16, 3, 6, 9).to(torch.bfloat16)
    assert pipe.vae.tile_batching
    d = pipe.vae.decode(z).sample
    pipe.vae.tile_batching = False
    assert torch.equal(d, pipe.vae.decode(z).sample)


def test_prepost_roundtrip_cpu(monkeypatch, tmp_path):
    """preprocess_frames / postprocess_frames / frame I/O glue (emulated ops): shapes, pads, the reference's x4 crop quirk."""
    emu_ops.install(monkeypatch)
    from dove_amd import prepost
    import numpy as np
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (8, 45, 80, 3), generator=g, dtype=torch.uint8)
    np.save(tmp_path / "clip.npy", frames.numpy())
    loaded = prepost.load_frames(str(tmp_path / "clip.npy"))
    assert torch.equal(loaded, frames)
    video, pf, ph, pw, orig = prepost.preprocess_frames(loaded, upscale=4, dtype=torch.float32, device="cpu")
    assert (pf, ph, pw) == (1, 3, 0) and orig == (8, 45, 80, 3)
    assert video.shape == (1, 3, 9, 192, 320) and float(video.min()) >= -1 and float(video.max()) <= 1
    out = prepost.postprocess_frames((video * 0.5 + 0.5), pf, ph, pw)
    assert out.shape == (8, 180, 320, 3) and out.dtype == torch.uint8
    # --upscale_mode: the torch route (the reference's own pad / F.interpolate / normalise, ref :220-233, :672-676) == the operator on
    # "bilinear"; "bicubic" is the other mode the reference's `align_corners=False` call accepts
    alt = prepost.preprocess_frames_torch(loaded, pf, ph, pw, 4, "bilinear", torch.float32)[None]
    assert alt.shape == video.shape and float((alt - video).abs().max()) < 1e-5
    cub, a1, b1, c1, _ = prepost.preprocess_frames(loaded, upscale=4, dtype=torch.float32, device="cpu", upscale_mode="bicubic")
    assert cub.shape == video.shape and (a1, b1, c1) == (pf, ph, pw) and float((cub - video).abs().max()) > 1e-3
    assert torch.equal(cub[0, :, 8], cub[0, :, 7])                 # frame padding repeats the last frame before the resize
    with pytest.raises(ValueError):
        prepost.preprocess_frames(loaded, upscale=4, dtype=torch.float32, device="cpu", upscale_mode="nearest")   # as in the reference: align_corners
    # identity check at the LR sample positions is not exact (bilinear), but constant frames must survive exactly
    const = torch.full((3, 16, 16, 3), 200, dtype=torch.uint8)
    v, a, b, c, _ = prepost.preprocess_frames(const, upscale=2, dtype=torch.float32, device="cpu")
    back = prepost.postprocess_frames(v * 0.5 + 0.5, a, b, c, crop_scale=2)
    assert back.shape == (3, 32, 32, 3) and int(back.float().mean().round()) in (199, 200)
    prepost.save_frames_as_png(back, str(tmp_path / "png"))
    assert torch.equal(prepost.load_frames(str(tmp_path / "png")), back)
    with pytest.raises(ValueError, match="H.264"):
        prepost.load_frames("clip.mp4")


def _write_checkpoint(root, v, t, s, wv, wt):
    """A CogVideoX1.5/DOVE-style directory (finetune/scripts/prepare_sft_ckpt.py layout): vae single file, transformer
    sharded with an index json (fp32 shards), scheduler config."""
    import json
    from safetensors.torch import save_file
    for d in ("vae", "transformer", "scheduler"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    json.dump(v, open(os.path.join(root, "vae", "config.json"), "w"))
    json.dump(t, open(os.path.join(root, "transformer", "config.json"), "w"))
    json.dump(dict(s, _class_name="CogVideoXDPMScheduler"), open(os.path.join(root, "scheduler", "scheduler_config.json"), "w"))
    save_file({k: x.contiguous() for k, x in wv.items()}, os.path.join(root, "vae", "diffusion_pytorch_model.safetensors"))
    keys = list(wt)
    half = len(keys) // 2
    shards = {"diffusion_pytorch_model-00001-of-00002.safetensors": keys[:half],
              "diffusion_pytorch_model-00002-of-00002.safetensors": keys[half:]}
    wmap = {}
    for fn, ks in shards.items():
        save_file({k: wt[k].contiguous() for k in ks}, os.path.join(root, "transformer", fn))
        wmap.update({k: fn for k in ks})
    json.dump({"metadata": {}, "weight_map": wmap}, open(os.path.join(root, "transformer", "diffusion_pytorch_model.safetensors.index.json"), "w"))


def test_from_pretrained_and_lora_fuse(monkeypatch, tmp_path):
    """Checkpoint loader (key/shape strict) + LoRA load/fuse (ref :613-621) on a synthetic checkpoint directory."""
    emu_ops.install(monkeypatch)
    from safetensors.torch import save_file
    v, t, s = config.tiny_configs()
    wv = weights.random_state_dict(weights.vae_param_shapes(v), 31)
    wt = weights.random_state_dict(weights.dit_param_shapes(t), 31)
    _write_checkpoint(str(tmp_path / "ckpt"), v, t, s, wv, wt)
    pipe = CogVideoXPipeline.from_pretrained(str(tmp_path / "ckpt"), torch_dtype=torch.bfloat16, device="cpu")
    ref = CogVideoXPipeline.from_config(v, t, s, seed=31, device="cpu")
    assert torch.equal(pipe.transformer.blocks[1]["qkv"].w, ref.transformer.blocks[1]["qkv"].w)
    assert torch.equal(pipe.vae.pc["decoder.conv_in"].w, ref.vae.pc["decoder.conv_in"].w)
    assert abs(float(pipe.scheduler.alphas_cumprod[399]) - 0.3935440575) < 1e-6
    # text_encoder/ and tokenizer/ are only opened by the first non-empty prompt (the documented runs use the shipped empty-prompt
    # embedding): a checkpoint whose T5 directory is unreadable still loads, and says what is wrong when a prompt needs it
    os.makedirs(tmp_path / "ckpt" / "text_encoder")
    os.makedirs(tmp_path / "ckpt" / "tokenizer")
    lazy = CogVideoXPipeline.from_pretrained(str(tmp_path / "ckpt"), torch_dtype=torch.bfloat16, device="cpu")
    assert not lazy.text_encoder.loaded and not lazy.tokenizer.loaded
    with pytest.raises(Exception):
        lazy.tokenizer("a prompt", return_tensors="pt")
    # strictness: a checkpoint with a missing tensor or a wrong shape must fail loudly
    import json
    wt_bad = {k: x for k, x in wt.items() if k != "proj_out.bias"}
    _write_checkpoint(str(tmp_path / "bad1"), v, t, s, wv, wt_bad)
    with pytest.raises(RuntimeError, match="mismatch"):
        weights.load_component(str(tmp_path / "bad1" / "transformer"), weights.dit_param_shapes)
    wt_bad2 = dict(wt)
    wt_bad2["proj_out.bias"] = torch.zeros(7)
    _write_checkpoint(str(tmp_path / "bad2"), v, t, s, wv, wt_bad2)
    with pytest.raises(RuntimeError, match="shape"):
        weights.load_component(str(tmp_path / "bad2" / "transformer"), weights.dit_param_shapes)
    # LoRA: rank-4 adapter on block 0 to_q and block 1 to_out.0, alpha/r = 0.5 stored in the metadata
    D = t["num_attention_heads"] * t["attention_head_dim"]
    g = torch.Generator().manual_seed(5)
    lora = {}
    for mod in ("transformer_blocks.0.attn1.to_q", "transformer_blocks.1.attn1.to_out.0"):
        lora[f"transformer.{mod}.lora_A.weight"] = torch.randn(4, D, generator=g) * 0.1
        lora[f"transformer.{mod}.lora_B.weight"] = torch.randn(D, 4, generator=g) * 0.1
    os.makedirs(tmp_path / "lora")
    save_file(lora, str(tmp_path / "lora" / "pytorch_lora_weights.safetensors"),
              metadata={"lora_adapter_metadata": json.dumps({"r": 4, "lora_alpha": 2})})
    pipe.load_lora_weights(str(tmp_path / "lora"), weight_name="pytorch_lora_weights.safetensors", adapter_name="test_1")
    pipe.fuse_lora(components=["transformer"], lora_scale=1.0)
    wt2 = dict(wt)
    for mod in ("transformer_blocks.0.attn1.to_q", "transformer_blocks.1.attn1.to_out.0"):
        wt2[mod + ".weight"] = wt[mod + ".weight"] + 0.5 * lora[f"transformer.{mod}.lora_B.weight"] @ lora[f"transformer.{mod}.lora_A.weight"]
    torch.manual_seed(1)
    hidden = torch.randn(1, 4, 16, 8, 12)
    text = torch.randn(1, 226, t["text_embed_dim"])
    rope = odit.rope_3d(64, 2, 4, 6)
    ts = torch.tensor([399])
    want = odit.OracleDiT(t, wt2).forward(hidden, text, ts, rope)
    base = odit.OracleDiT(t, wt).forward(hidden, text, ts, rope)
    got = pipe.transformer(hidden_states=hidden.to(torch.bfloat16), encoder_hidden_states=text.to(torch.bfloat16), timestep=ts,
                           image_rotary_emb=rope, return_dict=False)[0]
    assert rel(got, want) < 0.05 and rel(base, want) > 2 * rel(got, want)     # the adapter really changed the output
    with pytest.raises(RuntimeError, match="before load_lora_weights"):
        pipe.fuse_lora()


def test_dit_mxfp8_host_path(monkeypatch):
    """linear_precision="mxfp8": the four big linears of every block go through mx_quant + linear_mx with the same epilogue
    wiring (bias, GELU, gated residual, in-place residual stream) as the bf16 path.  With the operators emulated the result
    must sit at MXFP8 distance from the bf16 graph (quantisation noise only: a mis-wired gate or residual would be O(1))."""
    emu_ops.install(monkeypatch)
    from dove_amd.transformer import CogVideoXTransformer3DModel
    v, t, s = config.tiny_configs()
    wt = weights.random_state_dict(weights.dit_param_shapes(t), 41)
    torch.manual_seed(3)
    hidden = torch.randn(1, 4, 16, 8, 12).to(torch.bfloat16)
    text = torch.randn(1, 226, t["text_embed_dim"]).to(torch.bfloat16)
    rope = odit.rope_3d(64, 2, 4, 6)
    ts = torch.tensor([399])
    outs = {}
    for prec in ("bf16", "mxfp8", "mxfp8+attn"):
        tr = CogVideoXTransformer3DModel(t, wt, "cpu", linear_precision=prec.split("+")[0],
                                         attention_precision="mxfp8" if prec.endswith("attn") else "bf16")
        outs[prec] = tr(hidden_states=hidden, encoder_hidden_states=text, timestep=ts, image_rotary_emb=rope, return_dict=False)[0].float()
    want = odit.OracleDiT(t, wt).forward(hidden.float(), text.float(), ts, rope)
    e_bf, e_mx, e_mxa = rel(outs["bf16"], want), rel(outs["mxfp8"], want), rel(outs["mxfp8+attn"], want)
    print(f"tiny DiT rel-max-err vs fp32 oracle: bf16 graph {e_bf:.4f}, mxfp8 linears {e_mx:.4f}, + mxfp8 attention {e_mxa:.4f}")
    assert e_bf < 0.03 and e_mx < 0.15 and e_mxa < 0.2
    with pytest.raises(ValueError):
        CogVideoXTransformer3DModel(t, wt, "cpu", linear_precision="fp4")
    with pytest.raises(ValueError):
        CogVideoXTransformer3DModel(t, wt, "cpu", attention_precision="fp4")
