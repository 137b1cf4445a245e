"""ctypes binding of libdove_hip.so (include/dove_hip.h).  No CPU fallback: every op raises if the
library is missing or the call fails -- the product path never routes through torch math or the oracle."""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdove_hip.so")
_lib = None

F32, BF16, U8 = 0, 1, 2
METRIC_PSNR, METRIC_SSIM, METRIC_RGB_TO_Y = 1, 2, 4           # dove_fr_metrics flags
COLORFIX_WAVELET, COLORFIX_ADAIN, COLORFIX_CLAMP = 1, 2, 1    # dove_color_fix modes / flag
YUV_444, YUV_422, YUV_420, YUV_MONO = 0, 1, 2, 3              # dove_yuv_format.chroma
YUV_SITING_LEFT, YUV_SITING_CENTRE = 0, 1                     # dove_yuv_format.siting_h
VIDEO_RGB_U8, VIDEO_YUV = 0, 1                                # dove_video_params.in_format / out_format
RESIZE_BILINEAR, RESIZE_BICUBIC, RESIZE_AREA = 0, 1, 2        # dove_resize_f32 modes
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3        # dove_conv2d_f32 activations


class ConvDesc(C.Structure):
    """dove_conv_desc (include/dove_hip.h).  ``struct_size`` is filled in on construction: the library refuses a descriptor whose
    size is not the one it was built with (a stale binding would otherwise have its missing tail fields read from stray memory)."""
    _fields_ = [
        ("struct_size", C.c_uint), ("reserved", C.c_uint),
        ("x", C.c_void_p), ("cache", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p),
        ("resid", C.c_void_p), ("gate", C.c_void_p), ("out", C.c_void_p),
        ("t_in", C.c_int), ("h_in", C.c_int), ("w_in", C.c_int), ("cin", C.c_int),
        ("t_out", C.c_int), ("h_out", C.c_int), ("w_out", C.c_int), ("cout_pad", C.c_int), ("cout_store", C.c_int),
        ("kt", C.c_int), ("kh", C.c_int), ("kw", C.c_int), ("stride", C.c_int), ("pad_h", C.c_int), ("pad_w", C.c_int),
        ("up", C.c_int), ("tmode", C.c_int), ("act", C.c_int),
        ("ldo", C.c_longlong), ("ldr", C.c_longlong), ("gate_split", C.c_longlong),
        ("gn_partial", C.c_void_p), ("out_f32", C.c_int),
        ("nb", C.c_int), ("cache_stride", C.c_longlong), ("w_first", C.c_void_p), ("w_sub", C.c_void_p),
        ("w_pair", C.c_void_p), ("tdup", C.c_int), ("reserved2", C.c_int),
    ]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(ConvDesc)


class ModelConfig(C.Structure):
    """dove_model_config (include/dove_hip.h): the fields of vae/config.json and transformer/config.json the graph needs."""
    _fields_ = [(n, C.c_int) for n in ("vae_in_channels", "vae_out_channels", "vae_latent_channels", "vae_num_blocks")] + \
               [("vae_block_out_channels", C.c_int * 8)] + \
               [(n, C.c_int) for n in ("vae_layers_per_block", "vae_temporal_compression", "vae_enc_batch", "vae_dec_batch")] + \
               [("vae_norm_eps", C.c_float), ("vae_scaling_factor", C.c_float)] + \
               [(n, C.c_int) for n in ("dit_heads", "dit_head_dim", "dit_num_layers", "dit_in_channels", "dit_out_channels", "dit_patch",
                                       "dit_patch_t", "dit_text_dim", "dit_time_embed_dim", "dit_max_text", "dit_flip_sin_to_cos")] + \
               [("dit_norm_eps", C.c_float), ("dit_freq_shift", C.c_float)]


class ImageView(C.Structure):
    """dove_image_view (include/dove_hip.h): a strided 4-D view, element (n, c, y, x) at data + n*sn + c*sc + y*sh + x*sw elements."""
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int), ("reserved", C.c_int),
                ("sn", C.c_longlong), ("sc", C.c_longlong), ("sh", C.c_longlong), ("sw", C.c_longlong)]


class MusiqScale(C.Structure):
    """dove_musiq_scale (include/dove_hip.h): one scale's image size, leading zero padding and whether it is resized."""
    _fields_ = [(n, C.c_int) for n in ("rh", "rw", "pad_top", "pad_left", "resized", "reserved")]


class YuvFormat(C.Structure):
    """dove_yuv_format (include/dove_hip.h): a fixed-point 3x3 matrix (rint(c * 65536)), the offsets, the chroma layout and siting."""
    _fields_ = [("coef", C.c_int * 9), ("offset", C.c_int * 3), ("chroma", C.c_int), ("siting_h", C.c_int)]


class DitAux(C.Structure):
    _fields_ = [("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p), ("timestep_proj", C.c_void_p)]


VIDEO_AUX_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(DitAux))   # dove_video_aux_fn


class VideoParams(C.Structure):
    """dove_video_params (include/dove_hip.h): one whole-video session.  ``struct_size`` is filled in on construction, like ConvDesc."""
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_uint),
                ("width", C.c_int), ("height", C.c_int), ("upscale", C.c_int),
                ("chunk_len", C.c_int), ("overlap_t", C.c_int), ("tile_h", C.c_int), ("tile_w", C.c_int), ("overlap_h", C.c_int),
                ("overlap_w", C.c_int), ("color_fix", C.c_int), ("in_format", C.c_int), ("out_format", C.c_int),
                ("in_yuv", YuvFormat), ("out_yuv", YuvFormat),
                ("text", C.c_void_p), ("text_len", C.c_int), ("timestep", C.c_int),
                ("sqrt_alpha", C.c_float), ("sqrt_one_minus_alpha", C.c_float),
                ("noise_step", C.c_int), ("noise_sqrt_alpha", C.c_float), ("noise_sqrt_one_minus_alpha", C.c_float),
                ("max_frames", C.c_int), ("max_push", C.c_int), ("seed", C.c_ulonglong),
                ("aux_fn", VIDEO_AUX_FN), ("aux_user", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(VideoParams)


class Conv2dF32Args(C.Structure):
    """dove_conv2d_f32_args (include/dove_hip.h).  ``struct_size`` is filled in on construction, like ConvDesc."""
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_uint),
                ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p), ("out", C.c_void_p),
                ("n", C.c_int), ("h", C.c_int), ("w_in", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("kh", C.c_int), ("kw", C.c_int),
                ("stride", C.c_int), ("act", C.c_int), ("out_mul", C.c_float), ("ldx", C.c_longlong), ("ldo", C.c_longlong)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(Conv2dF32Args)


class ConvnetConvF32Args(C.Structure):
    """dove_convnet_conv_f32_args (include/dove_hip.h).  ``struct_size`` is filled in on construction, like ConvDesc."""
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_uint),
                ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
                ("n", C.c_int), ("h", C.c_int), ("w_in", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("kh", C.c_int), ("kw", C.c_int),
                ("stride", C.c_int), ("pad_h", C.c_int), ("pad_w", C.c_int), ("relu", C.c_int), ("reserved2", C.c_int),
                ("ldx", C.c_longlong), ("ldo", C.c_longlong)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(ConvnetConvF32Args)


class ResnetConvF32Args(C.Structure):
    """dove_resnet_conv_f32_args (include/dove_hip.h).  ``struct_size`` is filled in on construction, like ConvDesc."""
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_uint),
                ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p),
                ("n", C.c_int), ("h", C.c_int), ("w_in", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("k", C.c_int),
                ("stride", C.c_int), ("pool", C.c_int), ("relu", C.c_int), ("reserved2", C.c_int),
                ("ldx", C.c_longlong), ("ldr", C.c_longlong), ("ldo", C.c_longlong)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(ResnetConvF32Args)


class PreNoise(C.Structure):
    """dove_pre_noise: `--noise_step` of the graph-level dove_sr_clip."""
    _fields_ = [("eps", C.c_void_p), ("eps_dtype", C.c_int), ("sqrt_alpha", C.c_float), ("sqrt_one_minus_alpha", C.c_float)]


# dove_set_option keys (include/dove_hip.h)
OPT_VAE_TILING, OPT_VAE_SAMPLE_HEIGHT, OPT_VAE_SAMPLE_WIDTH, OPT_DIT_LINEAR_MXFP8, OPT_DIT_ATTN_MXFP8, OPT_WEIGHT_SUMS, OPT_VAE_STREAMS = 1, 2, 3, 4, 5, 6, 7
STAT_HALO_PREPOSTED, STAT_HALO_BLOCKING, STAT_HALO_SENT, STAT_HALO_COMMUNICATORS = 100, 101, 102, 103


_VP, _I, _LL, _F = C.c_void_p, C.c_int, C.c_longlong, C.c_float
_ULL, _PI, _PLL = C.c_ulonglong, C.POINTER(C.c_int), C.POINTER(C.c_longlong)
XFER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)   # dove_xfer_fn
GROUP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)                                  # dove_group_fn

# name -> argtypes; the symbol list doubles as the export check in tests/test_abi.py
SIGNATURES = {
    "dove_conv_igemm_bf16": [C.POINTER(ConvDesc), _VP],
    "dove_groupnorm_stats_bf16": [_VP, _LL, _LL, _I, _F, _VP, _I, _VP, _VP],
    "dove_groupnorm_finalize_partials": [_VP, _LL, C.c_double, _F, _VP, _VP, _VP],
    "dove_groupnorm_stats_nb_bf16": [_VP, _I, _LL, _LL, _I, _F, _VP, _I, _VP, _VP],
    "dove_groupnorm_finalize_partials_nb": [_VP, _LL, _I, C.c_double, _F, _VP, C.c_size_t, _VP, _VP],
    "dove_groupnorm_apply_nb_bf16": [_VP, _VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _I, _VP, _I, _I, _I, _I, C.POINTER(C.c_int), _VP],
    "dove_avgpool_time_nb_bf16": [_VP, _I, _I, _LL, _VP, _VP],
    "dove_groupnorm_sums_bf16": [_VP, _LL, _LL, _I, _VP, _I, _VP, _VP],
    "dove_groupnorm_finalize_sums": [_VP, C.c_double, _F, _VP, _VP],
    "dove_groupnorm_sums_from_partials": [_VP, _LL, _VP, _VP, _VP],
    "dove_groupnorm_apply_bf16": [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _I, _VP, _I, _I, _I, C.POINTER(C.c_int), _VP],
    "dove_layernorm_modulate_bf16": [_VP, _VP, _LL, _I, _F, _VP, _VP, _VP, _LL, _VP],
    "dove_qkv_post_bf16": [_VP, _LL, _LL, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _F, _F, _VP, _VP, _VP, _I, _VP, _VP],
    "dove_vt_quad_swap_bf16": [_VP, _LL, _LL, _VP],
    "dove_ulysses_place_bf16": [_VP, _VP, _VP, C.POINTER(C.c_longlong), _I, _I, _LL, _LL, _VP, _VP, _VP, _VP, _VP],
    "dove_cl_im2col3x3_from_ncthw": [_VP, _I, _I, _I, _I, _I, _I, _F, _F, _VP, _VP],
    "dove_conv_out_gather": [_VP, _LL, _I, _I, _I, _I, _VP, _F, _F, _F, _F, _VP, _I, _VP],
    "dove_attention_fwd_bf16": [_VP, _VP, _VP, _VP, _LL, _LL, _I, _I, _LL, _VP, _VP],
    "dove_qkv_post_mxfp8": [_VP, _LL, _LL, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _F, _F, _VP, _VP, _VP, _VP, _VP],
    "dove_attention_fwd_mxfp8": [_VP, _VP, _VP, _VP, _VP, _LL, _LL, _I, _I, _LL, _VP],
    "dove_cl_from_ncthw": [_VP, _I, _I, _LL, _I, _F, _F, _VP, _VP],
    "dove_ncthw_from_cl": [_VP, _LL, _I, _LL, _F, _F, _F, _F, _VP, _I, _VP],
    "dove_avgpool_time_bf16": [_VP, _I, _LL, _VP, _VP],
    "dove_posterior_sample": [_VP, _LL, _I, _LL, _VP, _I, _VP, _I, _VP],
    "dove_axpby": [_VP, _VP, _VP, _I, _LL, _F, _F, _VP],
    "dove_patchify": [_VP, _I, _I, _I, _I, _I, _I, _I, _VP, _LL, _VP],
    "dove_unpatchify": [_VP, _LL, _I, _I, _I, _I, _I, _I, _VP, _I, _VP],
    "dove_gemv_bf16": [_VP, _VP, _VP, _I, _I, _I, _VP, _VP],
    "dove_blend_edge_bf16": [_VP, _VP, _I, _I, _I, _I, _I, _I, _I, _I, _VP],
    "dove_preprocess_u8": [_VP, _I, _I, _I, _I, _I, _I, _I, _VP, _I, _VP],
    "dove_postprocess_u8": [_VP, _I, _I, _I, _I, _I, _I, _I, _VP, _VP],
    "dove_rmsnorm_bf16": [_VP, _VP, _LL, _I, _F, _VP, _VP],
    "dove_gated_gelu_bf16": [_VP, _VP, _LL, _I, _VP],
    "dove_attention_bias_bf16": [_VP, _VP, _VP, _LL, _VP, _VP, _LL, _I, _I, _I, _VP],
    "dove_mx_quant_bf16": [_VP, _LL, _I, _VP, _VP, _VP],
    "dove_create": [_I, C.POINTER(ModelConfig), C.POINTER(_VP)],
    "dove_set_weight": [_VP, C.c_char_p, _VP, C.POINTER(C.c_longlong), _I, _I],
    "dove_finalize_weights": [_VP],
    "dove_set_workspace": [_VP, _VP, C.c_size_t],
    "dove_vae_encode": [_VP, _VP, _I, _I, _I, _I, _VP, _I, _VP],
    "dove_dit_forward": [_VP, _VP, _I, _I, _I, _I, _VP, _I, _I, C.POINTER(DitAux), _VP, _I, _VP],
    "dove_vae_decode": [_VP, _VP, _I, _I, _I, _I, _F, _I, _VP, _I, _VP],
    "dove_sr_clip": [_VP, _VP, _I, _I, _I, _I, _VP, _I, _VP, _I, _I, _F, _F, C.POINTER(DitAux), C.POINTER(PreNoise), _VP, _I, _VP],
    "dove_set_option": [_VP, _I, _LL],
    "dove_comm_unique_id": [_VP],
    "dove_comm_init": [_VP, _VP, _I, _I],
    "dove_comm_init_custom": [_VP, _I, _I, XFER_FN, XFER_FN, _VP],
    "dove_comm_set_group": [_VP, GROUP_FN, GROUP_FN],
    "dove_shard_frames": [_VP, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "dove_conv_out_gather_cl": [_VP, _LL, _I, _I, _I, _I, _VP, _VP, _I, _VP],
    "dove_tile_gather_bf16": [_VP, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), _I, _VP, _VP],
    "dove_linear_mxfp8": [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _LL, _I, _I, _LL, _LL, _LL, _I, _VP],
    "dove_fr_metrics": [C.POINTER(ImageView), C.POINTER(ImageView), _I, _I, _I, _I, _I, _VP, C.c_size_t, _VP, _VP],
    "dove_color_fix": [C.POINTER(ImageView), _F, _F, C.POINTER(ImageView), _F, _F, _I, _I, _I, _I, _I, C.POINTER(ImageView), _VP,
                       C.c_size_t, _VP],
    "dove_rgb_to_yuv_u8": [C.POINTER(ImageView), _I, _I, _I, C.POINTER(YuvFormat), _VP, _VP],
    "dove_yuv_to_rgb_u8": [_VP, _I, _I, _I, C.POINTER(YuvFormat), _VP, _VP],
    # whole videos from C: the host planner returns counts (>= 0) where it fills a list, so its restype is the same int
    "dove_plan_padding": [_I, _I, _I, _PI, _PI, _PI],
    "dove_plan_output_size": [_I, _I, _I, _PI, _PI],
    "dove_plan_temporal_chunks": [_I, _I, _I, _PI, _I],
    "dove_plan_spatial_tiles": [_I, _I, _I, _I, _I, _I, _PI, _I],
    "dove_plan_valid_region": [_PI, _I, _I, _I, _I, _I, _I, _PI, _PI],
    "dove_plan_pieces": [_I, _I, _I, _I, _I, _I, _I, _I, _I, _PI, _PI, _PI, _I],
    "dove_plan_check_coverage": [_PI, _I, _I, _I, _I],
    "dove_chunk_planner_create": [_I, _I, C.POINTER(_VP)],
    "dove_chunk_planner_next": [_VP, _LL, _I, _PLL, _PLL, _PI],
    "dove_philox_u32": [_VP, _LL, _ULL, _ULL, _ULL, _VP],
    "dove_randn": [_VP, _I, _LL, _ULL, _ULL, _ULL, _VP],
    # degradation synthesis: sigma / scale / quality are host arrays
    "dove_blur2d_f32": [_VP, _I, _I, _I, _VP, _I, _I, _VP, _VP],
    "dove_resize_f32": [_VP, _I, _I, _I, _I, _I, _I, _VP, _VP],
    "dove_add_gaussian_noise_f32": [_VP, _I, _I, _I, C.POINTER(C.c_float), _I, _ULL, _ULL, _LL, _VP, _VP],
    "dove_add_poisson_noise_f32": [_VP, _I, _I, _I, C.POINTER(C.c_float), _I, _ULL, _ULL, _LL, _VP, C.c_size_t, _VP, _VP],
    "dove_jpeg_roundtrip": [_VP, _I, _I, _I, _PI, _VP, C.c_size_t, _VP, _VP],
    "dove_vcodec_roundtrip": [_VP, _I, _I, _I, _LL, _I, _VP, C.c_size_t, _VP, _VP, _VP, _VP],
    "dove_vcodec_roundtrip_tools": [_VP, _I, _I, _I, _LL, _I, _I, _VP, C.c_size_t, _VP, _VP, _VP, _VP],
    "dove_motion_search_u8": [_VP, _VP, _I, _I, _I, _I, _I, _VP, _VP, _VP],
    "dove_stitch": [_VP, _I, _I, _I, _PI, _VP, _I, _I, _I, _I, _I, _I, _VP],
    "dove_video_open": [_VP, C.POINTER(VideoParams), C.POINTER(_VP)],
    "dove_video_info": [_VP, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _PI, _PI, _PI],
    "dove_video_push": [_VP, _VP, _I, _VP],
    "dove_video_end_of_input": [_VP],
    "dove_video_need": [_VP, _PLL, _PI],
    "dove_video_step": [_VP, _VP, C.c_size_t, _PI, _PI, _VP],
    # optical flow (csrc/flow.hip, csrc/conv_f32.hip): fp32 channels-last operators with pixel strides, and the warping error
    "dove_conv2d_f32": [C.POINTER(Conv2dF32Args), _VP],
    "dove_instance_norm_f32": [_VP, _I, _I, _I, _I, _VP, _I, _F, _VP, C.c_size_t, _VP, _VP],
    "dove_corr_volume_f32": [_VP, _VP, _I, _I, _I, _I, _F, _VP, _VP],
    "dove_avgpool2_f32": [_VP, _LL, _I, _I, _VP, _VP],
    "dove_corr_lookup_f32": [_VP, _VP, _VP, _VP, _VP, _LL, _I, _I, _I, _I, _VP, _VP],
    "dove_gru_gate_f32": [_VP, _LL, _VP, _LL, _I, _I, _LL, _VP, _VP],
    "dove_gru_update_f32": [_VP, _LL, _VP, _LL, _VP, _LL, _I, _LL, _VP],
    "dove_add_f32": [_VP, _LL, _VP, _LL, _VP, _LL, _I, _LL, _I, _VP],
    "dove_convex_upsample_f32": [_VP, _LL, _VP, _I, _I, _I, _VP, _VP],
    "dove_flow_warp_error": [_VP, _VP, _I, _VP, _VP, _I, _I, _I, _VP, C.c_size_t, _VP, _VP, _VP, _VP],
    # perceptual metrics (csrc/percep.hip, csrc/conv_f32.hip): the fp32 trunk operators and the fp64 heads of LPIPS and DISTS; mean / std are host arrays
    "dove_convnet_conv_f32": [C.POINTER(ConvnetConvF32Args), _VP],
    "dove_percep_prep_f32": [C.POINTER(ImageView), _I, _I, _I, _I, _F, _F, C.POINTER(C.c_float), C.POINTER(C.c_float), _VP, _VP],
    "dove_maxpool_f32": [_VP, _LL, _I, _I, _I, _I, _I, _I, _VP, _LL, _VP],
    "dove_l2pool_f32": [_VP, _LL, _I, _I, _I, _I, _VP, _LL, _VP],
    "dove_lpips_layer": [_VP, _VP, _LL, _VP, _I, _I, _I, _I, _VP, C.c_size_t, _VP, _VP],
    "dove_dists_layer": [_VP, _VP, _LL, _VP, _VP, _I, _I, _I, _I, _VP, C.c_size_t, _VP, _VP],
    # NIQE (csrc/niqe.hip): features and stats on the device in fp64; the distance is host code on host pointers
    "dove_niqe_features": [C.POINTER(ImageView), _I, _I, _I, _I, _VP, C.c_size_t, _VP, _VP, _VP],
    "dove_niqe_stats": [_VP, _I, _I, _VP, _VP, _VP, _VP],
    "dove_niqe_distance": [_VP, _VP, _VP, _VP, _VP],
    # CLIP-IQA (csrc/clipiqa.hip, csrc/conv_f32.hip): the fp32 ResNet operators, the attention pool and the score in fp64
    "dove_resnet_conv_f32": [C.POINTER(ResnetConvF32Args), _VP],
    "dove_avgpool_cl_f32": [_VP, _LL, _I, _I, _I, _I, _VP, _LL, _VP],
    "dove_clip_attnpool_f32": [_VP, _LL, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP, _VP],
    "dove_clipiqa_score": [_VP, _VP, _I, _I, _I, C.c_double, _VP, _VP],
    # MUSIQ (csrc/musiq.hip): the patch gather, GroupNorm, LayerNorm, embeddings, fp32 attention, GELU and the fp64 head
    "dove_musiq_patches_f32": [C.POINTER(ImageView), _I, _I, _I, _I, C.POINTER(MusiqScale), _VP, _I, _I, _I, _VP, _VP],
    "dove_musiq_groupnorm_f32": [_VP, _VP, _VP, _VP, _VP, _VP, _LL, _I, _I, C.c_double, _I, _I, _VP, _VP],
    "dove_layernorm_f32": [_VP, _LL, _LL, _I, _VP, _VP, C.c_double, _VP, _LL, _VP],
    "dove_musiq_embed_f32": [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP],
    "dove_mha_f32": [_VP, _VP, _VP, _LL, _I, _I, _I, _F, _VP, _LL, _VP],
    "dove_gelu_f32": [_VP, _LL, _VP, _VP],
    "dove_musiq_score": [_VP, _LL, _VP, _VP, _I, _I, _I, _VP, _VP],
    # FasterVQA / FAST-VQA (csrc/swin3d.hip): the fragment gather, 3-D window partition and its inverse, patch merging, window attention, fp64 head
    "dove_vqa_fragments_f32": [C.POINTER(ImageView), _I, _I, _I, _VP, _I, _VP, _I, _I, _I, _I, _I, C.POINTER(C.c_double), C.POINTER(C.c_double),
                               _I, _VP, _VP],
    "dove_swin3d_window_gather_f32": [_VP, _I, _PI, _I, _PI, _PI, _VP, _VP],
    "dove_swin3d_window_scatter_f32": [_VP, _VP, _I, _PI, _I, _PI, _PI, _VP, _VP],
    "dove_swin3d_patch_merge_f32": [_VP, _LL, _I, _I, _I, _VP, _VP],
    "dove_swin3d_window_attention_f32": [_VP, _VP, _VP, _LL, _LL, _I, _I, _F, _VP, _VP, _I, _VP, _VP, _VP, _I, _VP, _LL, _VP],
    "dove_vqa_head_f64": [_VP, _LL, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _VP, _VP],
    # DOVER's aesthetic branch (csrc/convnext3d.hip): the depthwise 3 x 7 x 7 conv and the resized view
    "dove_dwconv3d_f32": [_VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP],
    "dove_vqa_resized_view_f32": [C.POINTER(ImageView), _I, _I, _I, _VP, _I, _VP, _VP, _I, _VP, _VP, _I, _I, _I, C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), _I, _VP, _VP],
    # MANIQA (csrc/maniqa.hip): the batched strided GEMM, row softmax, 2-D window attention, crop gather, cls / positions, scale-add-transpose
    # and the fp64 weighted head
    "dove_bmm_f32": [_VP, _LL, _LL, _VP, _LL, _LL, _VP, _VP, _LL, _LL, _VP, _LL, _LL, _I, _I, _I, _I, _F, _I, _VP],
    "dove_softmax_rows_f32": [_VP, _LL, _LL, _I, _VP, _LL, _VP],
    "dove_window_attention_f32": [_VP, _VP, _VP, _LL, _LL, _I, _I, _I, _F, _VP, _I, _VP, _VP, _I, _VP, _LL, _VP],
    "dove_maniqa_crops_f32": [C.POINTER(ImageView), _I, _I, _I, _I, _VP, _I, _I, _I, _VP, _VP],
    "dove_maniqa_tokens_f32": [_VP, _VP, _VP, _LL, _I, _I, _VP, _VP],
    "dove_mix_f32": [_VP, _LL, _LL, _VP, _LL, _LL, _F, _I, _I, _I, _I, _VP, _LL, _LL, _VP],
    "dove_maniqa_score": [_VP, _LL, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    # PNG encoder (csrc/png.hip): whole files on the device, and its deflate stage on a plain buffer
    "dove_png_encode": [C.POINTER(ImageView), _I, _I, _I, _I, _VP, C.c_size_t, _VP, _VP, _VP],
    "dove_zlib_huffman": [_VP, _LL, _LL, _VP, C.c_size_t, _VP, _VP, _VP],
    # JPEG encoder (csrc/jpeg.hip): whole baseline JFIF files on the device
    "dove_jpeg_encode": [C.POINTER(ImageView), _I, _I, _I, C.POINTER(C.c_int), _I, _VP, C.c_size_t, _VP, _VP, _VP],
}
PLAIN = {"dove_last_error": (C.c_char_p, []), "dove_abi_version": (C.c_int, []), "dove_comm_destroy": (None, [C.c_void_p]),
         "dove_conv_gn_partial_rows": (C.c_longlong, [C.POINTER(ConvDesc)]),
         "dove_conv_kernel_name": (C.c_char_p, [C.POINTER(ConvDesc)]),
         "dove_conv_partial_launches": (C.c_int, [C.POINTER(ConvDesc)]),
         "dove_attention_head_paths": (C.c_int, [C.POINTER(C.c_float), _I, C.POINTER(C.c_int)]),
         "dove_attention_path_name": (C.c_char_p, [_I]),
         "dove_device_info": (C.c_int, [_I, C.c_char_p, _I, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
         "dove_destroy": (None, [_VP]),
         "dove_vae_decode_num_frames": (C.c_int, [_VP, _I]),
         "dove_get_option": (C.c_longlong, [_VP, _I]),
         "dove_comm_useful_ranks": (C.c_int, [_VP, _I, _I]),
         "dove_workspace_bytes": (C.c_size_t, [_VP, _I, _I, _I]),
         "dove_workspace_high_water": (C.c_size_t, [_VP]),
         "dove_fr_metrics_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
         "dove_color_fix_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I]),
         "dove_yuv_frame_bytes": (C.c_size_t, [_I, _I, _I]),
         "dove_poisson_noise_workspace_bytes": (C.c_size_t, [_I]),
         "dove_jpeg_roundtrip_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
         "dove_vcodec_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I]),
         "dove_vcodec_tools_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
         "dove_chunk_planner_need": (C.c_longlong, [_VP]),
         "dove_chunk_planner_destroy": (None, [_VP]),
         "dove_video_workspace_bytes": (C.c_size_t, [_VP, C.POINTER(VideoParams)]),
         "dove_video_close": (None, [_VP]),
         "dove_instance_norm_f32_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I]),
         "dove_flow_warp_error_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
         "dove_convnet_conv_f32_kernel_name": (C.c_char_p, [C.POINTER(ConvnetConvF32Args)]),
         "dove_lpips_layer_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
         "dove_dists_layer_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I]),
         "dove_niqe_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
         "dove_resnet_conv_f32_kernel_name": (C.c_char_p, [C.POINTER(ResnetConvF32Args)]),
         "dove_clip_attnpool_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
         "dove_mha_f32_tiles": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
         "dove_swin3d_attention_tiles": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
         "dove_dwconv3d_tile": (None, [_I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
         "dove_bmm_f32_tiles": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
         "dove_bmm_f32_kernel_name": (C.c_char_p, [_I]),
         "dove_window_attention_tiles": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
         "dove_png_segment_rows": (C.c_int, [_I, _I]),
         "dove_png_bound": (C.c_size_t, [_I, _I, _I]),
         "dove_png_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I]),
         "dove_zlib_huffman_bound": (C.c_size_t, [_LL, _LL]),
         "dove_zlib_huffman_workspace_bytes": (C.c_size_t, [_LL, _LL]),
         "dove_jpeg_restart_mcus": (C.c_int, []),
         "dove_jpeg_bound": (C.c_size_t, [_I, _I, _I]),
         "dove_jpeg_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I])}


def kernel_source_sha256() -> str:
    """sha256 over the kernel sources (csrc/*.hip, csrc/*.h, include/dove_hip.h; names and bytes, sorted): what a measurement of the kernels
    is a measurement OF.  tools/pmc_bench_traffic.py stores it in profiles/pmc_traffic.json and bench.py replays that summary only when it
    equals the tree's - a PMC pass taken on other kernel code (round 4: the MFMA-shape move) can no longer be replayed as this build's."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h")))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "dove_hip.h"))
    for fn in files:
        h.update(os.path.basename(fn).encode() + b"\0")
        with open(fn, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    return h.hexdigest()


def load():
    """Load libdove_hip.so (built by ``__graft_entry__.build()`` / dove_amd/csrc/build.sh)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(dove_amd has no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, argt in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argt
        fn.restype = C.c_int
    for name, (res, argt) in PLAIN.items():
        fn = getattr(lib, name)
        fn.argtypes = argt
        fn.restype = res
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {load().dove_last_error().decode()}")


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def dt_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"dove_amd supports float32 / bfloat16 boundary tensors, got {t.dtype}")


def require_cuda(*tensors):
    cur = None
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("dove_amd ops need tensors on the HIP device (`cuda`); there is no CPU path")
        if t is not None:
            # kernels launch on the CURRENT device's stream (stream_ptr) and the library keeps per-device state keyed by
            # hipGetDevice(): a tensor of another GPU would be dereferenced there
            if cur is None:
                cur = torch.cuda.current_device()
            if t.device.index != cur:
                raise RuntimeError(f"dove_amd op called with a tensor on cuda:{t.device.index} while cuda:{cur} is current; "
                                   "wrap the call in torch.cuda.device(tensor.device)")
        if t is not None and not t.is_contiguous():
            raise RuntimeError("dove_amd ops need contiguous tensors")
