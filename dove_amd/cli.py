"""Command-line driver mirroring the reference's ``python inference_script.py ...`` (ref :506-778) on the HIP path.

Every flag of the reference's parser (ref :507-554) is accepted: ``--input_dir --input_json --gt_dir --eval_metrics --model_path
--lora_path --output_path --fps --dtype --seed --upscale_mode --upscale --noise_step --sr_noise_step --is_cpu_offload --is_vae_st
--png_save --save_format --tile_size_hw --overlap_hw --chunk_len --overlap_t``; ``--color_fix {none,wavelet,adain}`` (not a flag of the reference's script: its
``finetune/scripts/color_fix_util.py`` on the GPU, dove_amd.colorfix) fixes every output frame against the clip's upscaled input.  ``--fps`` / ``--save_format`` describe the mp4
container the reference writes with imageio - frame files carry neither, so they are accepted and reported (with ``--y4m_save`` they are the
frame rate and chroma layout of the ``<clip>.y4m`` written: YUV4MPEG2, dove_amd.y4m / dove_amd.stream); ``--is_cpu_offload``
calls ``pipe.enable_sequential_cpu_offload()`` like the reference (a no-op with 288 GB of HBM); ``--eval_metrics`` knows the metrics of
``dove_amd.metrics.REGISTRY``, computed on the GPU from the uint8 frames written to disk against ``--gt_dir/<clip>``, as the reference's
``eval_metrics.py`` scores the saved files; the per-clip values go to ``metrics_<names>.json`` in ``--output_path`` (the reference's
structure, ref :755-776); the registry's metrics that need weights take them from ``--metric_weights DIR`` (``--help`` lists the files); without it they, and always the other metrics of pyiqa, are refused; ``--dtype`` other than bfloat16 is refused.  Inputs are PNG folders,
``.npy`` clips (uint8 [F,H,W,3]) or ``.y4m`` files because H.264 decoding (decord) is outside the accelerated path; outputs are PNG
folders, ``.npy`` or ``.y4m`` (``--y4m_save``; streamed chunk by chunk when ``--chunk_len > 0``), or - encoded on the GPU, dove_amd.jpeg - ``.jpg`` folders
(``--jpg_save``) or one Motion-JPEG ``.avi`` per clip at ``--fps`` (``--avi_save``), at ``--jpeg_quality`` and the subsampling of ``--save_format``.  ``--random_init`` builds the CogVideoX1.5-5B architecture with synthetic weights (no checkpoint is
available offline).  ``--eval_psnr_dir`` computes plain PSNR (10*log10(1/MSE), per-frame mean) on the CPU against ground-truth folders; with it,
``psnr`` in ``--eval_metrics`` is that value and the other metrics use ``--gt_dir`` (or those folders without ``--gt_dir``)."""
from __future__ import annotations

import argparse
import os

import torch


def add_model_arguments(ap):
    """The model and SR flags, shared with ``python -m dove_amd.stream``."""
    ap.add_argument("--model_path", type=str, default=None)
    ap.add_argument("--lora_path", type=str, default=None, help="LoRA weights to fuse into the transformer (ref :613-621)")
    ap.add_argument("--random_init", action="store_true")
    ap.add_argument("--fps", type=int, default=16, help="frame rate of the Y4M file (--y4m_save) or the Motion-JPEG AVI (--avi_save; ref :521); PNG / JPEG / .npy frame files carry none")
    ap.add_argument("--dtype", type=str, default="bfloat16")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--upscale_mode", type=str, default="bilinear", help="ref :527, :672; 'bilinear' is the fused HIP kernel, others run torch's interpolate")
    ap.add_argument("--upscale", type=int, default=4)
    ap.add_argument("--is_cpu_offload", action="store_true", help="ref :533, :637-641: enable_sequential_cpu_offload() (a no-op here)")
    ap.add_argument("--save_format", type=str, default="yuv444p",
                    help="pixel format of the Y4M file (--y4m_save): yuv444p, yuv422p or yuv420p (ref :541); chroma subsampling of "
                         "--jpg_save / --avi_save: yuv444p (4:4:4) or yuv420p (4:2:0); unused otherwise")
    ap.add_argument("--noise_step", type=int, default=0)
    ap.add_argument("--sr_noise_step", type=int, default=399)
    ap.add_argument("--is_vae_st", action="store_true")
    ap.add_argument("--tile_size_hw", type=int, nargs=2, default=(0, 0))
    ap.add_argument("--overlap_hw", type=int, nargs=2, default=(32, 32))
    ap.add_argument("--chunk_len", type=int, default=0)
    ap.add_argument("--overlap_t", type=int, default=8)
    ap.add_argument("--color_fix", type=str, default="none", choices=("none", "wavelet", "adain"),
                    help="colour-fix every output frame against the clip's upscaled input on the GPU (dove_amd.colorfix; the reference's "
                         "color_fix_util); saved and scored frames are the fixed ones")
    ap.add_argument("--yuv_matrix", type=str, default="bt601", choices=("bt601", "bt709"),
                    help="colour matrix of .y4m input and output (Y4M does not carry one; bt601 is what swscale assumes for RGB)")
    ap.add_argument("--yuv_range", type=str, default=None, choices=("limited", "full"),
                    help="range of .y4m output, and of .y4m input in place of its XCOLORRANGE tag (default: the tag / limited)")
    ap.add_argument("--num_layers", type=int, default=None, help="debug (with --random_init): fewer DiT layers than the 42 of CogVideoX1.5-5B")
    ap.add_argument("--prompt_embedding", type=str,
                    default="pretrained_models/prompt_embeddings/e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855.safetensors")


def check_dtype(args):
    if args.dtype != "bfloat16":
        raise ValueError(f"--dtype {args.dtype}: the HIP path computes in bfloat16 (the reference's default, ref :525); float16 / float32 "
                         "are not implemented (INTEGRATION.md, 'dtype')")


def check_eval_metrics(metrics, metric_weights: str, has_gt: bool) -> None:
    """Refuse what ``--eval_metrics`` cannot be computed from, before a model is built: a name outside ``metrics.REGISTRY``, a metric that
    needs weights without ``--metric_weights`` or without its main file there, a full-reference metric without ground truth."""
    from .metrics import FR, NETWORK, NR, REGISTRY, metric_names, name_list
    weighted = metric_names(NETWORK, NR)
    known = metric_names(FR) + (weighted if metric_weights else ())
    flag = ",".join(metrics)
    if any(m not in known for m in metrics):
        raise NotImplementedError(f"--eval_metrics {flag}: only {name_list(repr(m) for m in known)} are computed here; " +
                                  ("the other pyiqa metrics are outside the path" if metric_weights else
                                   "the other pyiqa metrics need network weights and are outside the path "
                                   f"(--metric_weights DIR adds {name_list(weighted)})"))
    for m in metrics:
        spec = REGISTRY[m]
        if spec.probe is not None and not spec.probe(metric_weights):   # as create_metric(m) without weights: not a metric here
            raise NotImplementedError(f"--eval_metrics {m}: {metric_weights} holds none of the files of {m} ({', '.join(spec.patterns)}); "
                                      f"{m} is computed only from files you supply (INTEGRATION.md {spec.section})")
    if any(m not in metric_names(NR) for m in metrics) and not has_gt:
        raise ValueError(f"--eval_metrics {flag} needs --gt_dir")


def build_pipe(args):
    """The pipeline the flags of ``add_model_arguments`` describe, seeded and on the device -> (pipe, empty-prompt embedding)."""
    from safetensors.torch import load_file

    from .pipeline import CogVideoXPipeline
    from .scheduler import CogVideoXDPMScheduler

    check_dtype(args)
    torch.manual_seed(args.seed)
    emb = load_file(args.prompt_embedding)["prompt_embedding"] if os.path.exists(args.prompt_embedding) else None
    if emb is None:
        raise FileNotFoundError(f"empty-prompt embedding not found at {args.prompt_embedding} (the reference ships it; ref :668-676)")
    if args.random_init or not args.model_path:
        from . import config
        v, t, s = config.default_configs()
        if args.num_layers:
            t["num_layers"] = args.num_layers
        pipe = CogVideoXPipeline.from_config(v, t, s, device="cuda", init_device="cuda")
    else:
        pipe = CogVideoXPipeline.from_pretrained(args.model_path, torch_dtype=torch.bfloat16)
    if args.lora_path:
        print(f"Loading LoRA weights from {args.lora_path}")
        pipe.load_lora_weights(args.lora_path, weight_name="pytorch_lora_weights.safetensors", adapter_name="test_1")
        pipe.fuse_lora(components=["transformer"], lora_scale=1.0)
    pipe.scheduler = CogVideoXDPMScheduler.from_config(pipe.scheduler.config, timestep_spacing="trailing")
    if args.is_cpu_offload:
        pipe.enable_sequential_cpu_offload()
    else:
        pipe.to("cuda")
    return pipe, emb


def _y4m_writer(path, frames_shape, args, chroma):
    from . import stream, y4m
    Ho, Wo = stream.output_size(frames_shape[1], frames_shape[2], args.upscale)
    return y4m.Y4MWriter(path, Wo, Ho, args.fps, chroma, args.yuv_range == "full")


def _stream_clip(pipe, emb, args, name, prompt, frames, path, chroma, color_fix, need_frames):
    """--y4m_save with --chunk_len > 0: the clip goes through ``stream.sr_stream`` chunk by chunk (one chunk of SR output on the device).
    Returns the frames decoded from the file written when they are scored, else None."""
    from . import prepost, stream, tiling
    F, H, W, _ = frames.shape
    pad_f, pad_h, pad_w = tiling.match_padding(F, H, W)
    shape = (1, 3, F + pad_f, (H + pad_h) * args.upscale, (W + pad_w) * args.upscale)
    items = tiling.plan(shape, args.chunk_len, args.overlap_t, tuple(args.tile_size_hw), tuple(args.overlap_hw))
    print(f"Process video: {name} | Prompt: {prompt} | Frame: {shape[2]} (ori: {F}; pad: {pad_f}) | Target Resolution: "
          f"{shape[3]}, {shape[4]} | Chunk Num: {len(items)}")
    with _y4m_writer(path, frames.shape, args, chroma) as writer:
        stream.sr_stream(pipe, stream.FrameSource(frames), writer, upscale=args.upscale, upscale_mode=args.upscale_mode,
                         chunk_len=args.chunk_len, overlap_t=args.overlap_t, tile_size_hw=tuple(args.tile_size_hw),
                         overlap_hw=tuple(args.overlap_hw), noise_step=args.noise_step, sr_noise_step=args.sr_noise_step, prompt=prompt,
                         empty_prompt_embedding=emb, color_fix=color_fix, yuv_matrix=args.yuv_matrix, log=lambda msg: None)
    return prepost.load_frames(path, yuv_matrix=args.yuv_matrix) if need_frames else None


def _save_clip_y4m(out, video, pads, args, path, chroma, color_fix, need_frames):
    """--y4m_save of a clip stitched in memory: the whole clip is converted at once (fused with the crop and the uint8 step unless a
    colour fix runs first)."""
    from . import prepost, yuv
    pad_f, pad_h, pad_w = pads
    fmt = yuv.YuvFormat(chroma, args.yuv_matrix, args.yuv_range or "limited")
    _, _, F, H, W = out.shape
    crop = (F - pad_f, H - pad_h * 4, W - pad_w * 4)
    if color_fix:
        payload = yuv.rgb_to_yuv(prepost.postprocess_frames(out, pad_f, pad_h, pad_w, color_fix=color_fix, source=video), fmt)
    else:
        payload = yuv.rgb_to_yuv(out, fmt, crop=crop)
    from . import y4m
    with y4m.Y4MWriter(path, crop[2], crop[1], args.fps, chroma, args.yuv_range == "full") as writer:
        writer.write(payload.cpu())
    return prepost.load_frames(path, yuv_matrix=args.yuv_matrix) if need_frames else None


def jpeg_subsampling(save_format: str) -> str:
    """--save_format -> the subsampling of --jpg_save / --avi_save; refused only where a JPEG is written."""
    table = {"yuv444p": "444", "yuv420p": "420"}
    if save_format not in table:
        raise ValueError(f"--save_format {save_format}: --jpg_save / --avi_save write yuv444p (4:4:4) or yuv420p (4:2:0); 4:2:2 JPEG is not "
                         "built")
    return table[save_format]


def build_parser() -> argparse.ArgumentParser:
    from . import metrics as M
    ap = argparse.ArgumentParser(description="VSR using DOVE on MI355X (dove_amd)")
    ap.add_argument("--input_dir", type=str, required=True)
    ap.add_argument("--input_json", type=str, default=None, help="{clip name: prompt}; clips without an entry use the empty prompt (ref :590-594, :676)")
    ap.add_argument("--output_path", type=str, default="./results")
    ap.add_argument("--gt_dir", type=str, default=None, help="ground-truth folders / .npy / .y4m clips for --eval_metrics (ref :511)")
    ap.add_argument("--eval_metrics", type=str, default="",
                    help=f"any of '{','.join(M.metric_names(M.FR))}' (ref :513), on the GPU; with --metric_weights also "
                         f"'{','.join(M.metric_names(M.NETWORK))}' and the no-reference '{','.join(M.metric_names(M.NR))}' (which need no "
                         "--gt_dir); the other network metrics of pyiqa are not provided")
    ap.add_argument("--metric_weights", type=str, default="", help=f"directory with the files of {M.weights_help()}")
    ap.add_argument("--png_save", action="store_true")
    ap.add_argument("--png_encoder", type=str, default="pil", choices=("pil", "gpu"),
                    help="who writes the --png_save files: PIL on the host, or the GPU encoder (dove_amd.png)")
    ap.add_argument("--y4m_save", action="store_true",
                    help="write <clip>.y4m (YUV4MPEG2) with --fps and --save_format; with --chunk_len > 0 it is streamed chunk by chunk")
    ap.add_argument("--jpg_save", action="store_true", help="write <clip>/000.jpg, ... (baseline JPEG encoded on the GPU, dove_amd.jpeg)")
    ap.add_argument("--avi_save", action="store_true",
                    help="write <clip>.avi (Motion-JPEG in RIFF AVI 1.0 at --fps; the frames are encoded on the GPU, dove_amd.jpeg / dove_amd.avi)")
    ap.add_argument("--jpeg_quality", type=int, default=95, help="libjpeg quality 1..100 of --jpg_save / --avi_save")
    ap.add_argument("--eval_psnr_dir", type=str, default=None)
    add_model_arguments(ap)
    return ap


def main(argv=None):
    from . import eval_metrics
    args = build_parser().parse_args(argv)
    check_dtype(args)
    metrics = [m.strip().lower() for m in args.eval_metrics.split(",") if m.strip()]
    check_eval_metrics(metrics, args.metric_weights, bool(args.gt_dir or args.eval_psnr_dir))
    # with --eval_psnr_dir, PSNR stays on that flag's CPU path (against its folders, as before); the rest runs on the GPU against
    # --gt_dir (or the --eval_psnr_dir folders when --gt_dir is not given)
    gpu_metrics = [m for m in metrics if not (m == "psnr" and args.eval_psnr_dir)]
    metric_weights = eval_metrics.load_weights(metrics, args.metric_weights)
    metrics_gt = args.gt_dir or args.eval_psnr_dir
    y4m_chroma = None
    forms = [f for f in ("png_save", "y4m_save", "jpg_save", "avi_save") if getattr(args, f)]
    if len(forms) > 1 and forms != ["png_save", "y4m_save"]:
        raise ValueError(" and ".join("--" + f for f in forms) + ": choose one output form")
    jpeg_sub = None
    if args.jpg_save or args.avi_save:
        if not 1 <= args.jpeg_quality <= 100:
            raise ValueError(f"--jpeg_quality {args.jpeg_quality} is not in 1..100")
        jpeg_sub = jpeg_subsampling(args.save_format)
    if args.y4m_save:
        if args.png_save:
            raise ValueError("--y4m_save and --png_save: choose one output form")
        from . import yuv
        y4m_chroma = yuv.save_format_to_chroma(args.save_format)      # refused only where a Y4M file is written

    from . import prepost, tiling
    from .inference import run_clip

    pipe, emb = build_pipe(args)
    if args.y4m_save:
        print(f"[dove_amd] clips are written as .y4m (YUV4MPEG2, {args.save_format}, {args.fps} fps, {args.yuv_matrix} / "
              f"{args.yuv_range or 'limited'}); --eval_metrics score the frames decoded from that file")
    elif args.jpg_save or args.avi_save:
        print(f"[dove_amd] clips are written as " + (f"Motion-JPEG .avi at {args.fps} fps" if args.avi_save else ".jpg folders") +
              f" (baseline JPEG, quality {args.jpeg_quality}, {args.save_format}); --eval_metrics score the frames before JPEG coding")
    elif not args.png_save:
        print(f"[dove_amd] clips are written as .npy frame arrays (uint8 [F,H,W,3]); --fps {args.fps} / --save_format {args.save_format} "
              "apply to the reference's mp4 writer only")
    if args.is_vae_st:
        pipe.vae.enable_slicing()
        pipe.vae.enable_tiling()
    color_fix = None if args.color_fix == "none" else args.color_fix
    if color_fix:
        print(f"[dove_amd] --color_fix {color_fix}: output frames are colour-fixed against the upscaled input "
              f"(--upscale_mode {args.upscale_mode}, x{args.upscale}) before they are saved and scored")
    overlap_t = args.overlap_t if args.chunk_len > 0 else 0
    os.makedirs(args.output_path, exist_ok=True)
    names = sorted(n for n in os.listdir(args.input_dir)
                   if n.lower().endswith((".npy", ".y4m")) or os.path.isdir(os.path.join(args.input_dir, n)))
    if not names:
        raise ValueError(f"No clips (.npy, .y4m or PNG folders) found in {args.input_dir}")
    yuv_in = {"yuv_matrix": args.yuv_matrix, "yuv_range": args.yuv_range}    # how .y4m clips (input and ground truth) are read
    need_frames = bool(metrics or args.eval_psnr_dir)
    prompts = {}
    if args.input_json is not None:
        import json
        with open(args.input_json) as f:
            prompts = json.load(f)
    psnrs = {}
    scores = {m: [] for m in metrics}                                     # per clip, in clip order (ref :647-656, :755-776)
    for name in names:
        prompt = prompts.get(name, "")
        frames = prepost.load_frames(os.path.join(args.input_dir, name), **yuv_in)
        stem = name[:-4] if name.lower().endswith((".npy", ".y4m")) else name
        if args.y4m_save and args.chunk_len > 0:
            frames_out = _stream_clip(pipe, emb, args, name, prompt, frames, os.path.join(args.output_path, stem + ".y4m"), y4m_chroma,
                                      color_fix, need_frames)
        else:
            video, pad_f, pad_h, pad_w, orig = prepost.preprocess_frames(frames, args.upscale, upscale_mode=args.upscale_mode)
            plan = dict(chunk_len=args.chunk_len, overlap_t=overlap_t, tile_size_hw=tuple(args.tile_size_hw), overlap_hw=tuple(args.overlap_hw))
            print(f"Process video: {name} | Prompt: {prompt} | Frame: {video.shape[2]} (ori: {orig[0]}; pad: {pad_f}) | Target Resolution: "
                  f"{video.shape[3]}, {video.shape[4]} | Chunk Num: {len(tiling.plan(video.shape, **plan))}")
            out, wc = run_clip(pipe, video, prompt=prompt, noise_step=args.noise_step, sr_noise_step=args.sr_noise_step,
                               empty_prompt_embedding=emb, out_device=video.device, out_dtype=torch.bfloat16, **plan)
            tiling.check_coverage(wc)
            if args.y4m_save:
                frames_out = _save_clip_y4m(out, video, (pad_f, pad_h, pad_w), args, os.path.join(args.output_path, stem + ".y4m"),
                                            y4m_chroma, color_fix, need_frames)
            elif color_fix:
                frames_out = prepost.postprocess_frames(out, pad_f, pad_h, pad_w, color_fix=color_fix, source=video)
            else:
                frames_out = prepost.postprocess_frames(out, pad_f, pad_h, pad_w)   # the reference crops pad*4 (ref :731)
        if args.y4m_save:
            pass
        elif args.png_save:
            prepost.save_frames_as_png(frames_out, os.path.join(args.output_path, stem), encoder=args.png_encoder)
        elif args.jpg_save:
            prepost.save_frames_as_jpeg(frames_out, os.path.join(args.output_path, stem), args.jpeg_quality, jpeg_sub)
        elif args.avi_save:
            from . import jpeg
            jpeg.save_avi(frames_out, os.path.join(args.output_path, stem + ".avi"), fps=args.fps, quality=args.jpeg_quality,
                          subsampling=jpeg_sub)
        else:
            import numpy as np
            np.save(os.path.join(args.output_path, stem + ".npy"), frames_out.cpu().numpy())
        if args.eval_psnr_dir:
            gt = prepost.load_frames(os.path.join(args.eval_psnr_dir, name), **yuv_in).float() / 255
            pr = frames_out.cpu().float() / 255
            mse = ((gt - pr) ** 2).flatten(1).mean(1)
            psnrs[name] = float((10 * torch.log10(1.0 / (mse + 1e-8))).mean())
            print(f"[{name}] PSNR={psnrs[name]:.4f}")
        if gpu_metrics:
            from .metrics import clip_metrics, nr_clip_metrics
            if metrics_gt:
                gt = prepost.load_frames(os.path.join(metrics_gt, name), **yuv_in)
                vals = clip_metrics(frames_out, gt, gpu_metrics, weights=metric_weights)
            else:                                                         # only no-reference metrics were asked for (checked above)
                vals = nr_clip_metrics(frames_out, gpu_metrics, metric_weights)
            for m in gpu_metrics:
                print(f"[{name}] {m.upper()}={vals[m]:.4f}")
        for m in metrics:
            scores[m].append(vals[m] if m in gpu_metrics else psnrs[name])
    if psnrs:
        print(f"=== Overall Average PSNR: {sum(psnrs.values()) / len(psnrs):.4f} ===")
    if metrics:
        import json
        average = {m: sum(v) / len(v) for m, v in scores.items()}
        for m in gpu_metrics:
            print(f"=== Overall Average {m.upper()}: {average[m]:.4f} ===")
        with open(os.path.join(args.output_path, eval_metrics.output_name(metrics)), "w") as f:
            json.dump({"per_sample": scores, "average": average, "count": len(names)}, f, indent=2)
    print("All videos processed.")


if __name__ == "__main__":
    main()
