/* libdove_hip.so -- C ABI of the MI355X-native (gfx950) operator library behind DOVE's one-step video-SR path.
 *
 * The reference (zhengchen1999/DOVE) has no FFI of its own: `inference_script.py::process_video`
 * (/root/reference/inference_script.py:394-503) drives a diffusers `CogVideoXPipeline`, and every FLOP is a
 * torch operator invoked inside diffusers modules.  The entry points below are what those modules would bind
 * instead of the torch operators -- each one cites the reference call site whose arithmetic it carries
 * (the module names are diffusers'; SURVEY.md App. A restates them).  INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions
 *  - plain C: raw device pointers, sizes, a `hipStream_t` passed as `void*`; no torch / C++ types.
 *  - every function returns 0 on success, a negative DOVE_E* code otherwise; `dove_last_error()` holds the message
 *    (thread-local).  No exceptions cross the ABI.
 *  - all tensor memory is owned by the caller; launches are asynchronous on the given stream.
 *  - activations: channels-last bf16 ([T,H,W,C] for the VAE, [N,C] token-major for the DiT); statistics,
 *    biases, norm affine parameters and modulation vectors are fp32.
 */
#ifndef DOVE_HIP_H
#define DOVE_HIP_H

#include <stddef.h> /* size_t */

#ifdef __cplusplus
extern "C" {
#endif

#define DOVE_ABI_VERSION 15

/* dtype codes for boundary tensors */
#define DOVE_F32 0
#define DOVE_BF16 1

const char* dove_last_error(void);
int dove_abi_version(void);
/* name / CU count / total memory of HIP device `dev`; name_len bytes available in `name` */
int dove_device_info(int dev, char* name, int name_len, int* cu_count, long long* total_mem);

/* Implicit-GEMM convolution / linear layer (bf16 in, fp32 accumulate on MFMA, bf16 out).
 * Carries: CogVideoXCausalConv3d, Downsample3D / Upsample3D convs, resnet 1x1x1 shortcut, SpatialNorm conv_y/conv_b
 * (vae.encode / decode_latents, /root/reference/inference_script.py:408,500) and every nn.Linear of
 * CogVideoXTransformer3DModel (/root/reference/inference_script.py:483-489).
 *   x      [t_in, h_in, w_in, cin]      cin multiple of 32 (zero-padded channels)
 *   cache  [kt-1, h_in, w_in, cin] or NULL: temporal front halo = last frames of the previous frame-batch's
 *          input (diffusers `conv_cache`); NULL replicates frame 0.
 *   w      [kt*kh*kw][cout_pad][cin]    packed, cout_pad multiple of 32, padding rows zero
 *   out    [t_out, h_out, w_out, ldo]   channels [0, cout_store) written (cout_store multiple of 4)
 *   input row for output row oh and tap dh: (oh*stride + dh - pad_h) >> up   (`up`=1 folds a nearest x2 upsample)
 *   tmode (kt==1 only): 0 t_in=t, 1 t_in=t>>1, 2 t_in = t==0 ? 0 : 1+((t-1)>>1)   (Upsample3D time doubling)
 *   epilogue: v = acc + bias; act==1: gelu(tanh); resid: v = resid + (gate ? gate[class][c] * v : v), where
 *   class = (flat output pixel index < gate_split) ? 0 : 1 and gate is [2][cout_pad] fp32 (AdaLN-Zero gates). */
typedef struct dove_conv_desc {
  /* = sizeof(dove_conv_desc) of the header the CALLER was built against.  The descriptor is caller-allocated and grows with the
   * ABI (gn_partial at 2, out_f32 at 8): a binding written against an older header would hand over a shorter struct and the new
   * fields would be read from whatever follows it.  Every entry point that takes a descriptor rejects a size other than its own. */
  unsigned int struct_size;
  unsigned int reserved; /* 0 */
  const void* x;
  const void* cache;
  const void* w;
  const float* bias;
  const void* resid;
  const float* gate;
  void* out;
  int t_in, h_in, w_in, cin;
  int t_out, h_out, w_out, cout_pad, cout_store;
  int kt, kh, kw, stride, pad_h, pad_w, up, tmode, act;
  long long ldo, ldr, gate_split;
  /* optional fused GroupNorm(32) statistics of `out` (the nn.GroupNorm that consumes this conv's output in
   * CogVideoXResnetBlock3D / CogVideoXSpatialNorm3D): fp32 [dove_conv_gn_partial_rows(d)][32][2] partial (sum, sum of
   * squares) per group over the bf16-rounded stored values; reduce with dove_groupnorm_finalize_partials.  Only the
   * kernels for which dove_conv_gn_partial_rows() > 0 produce them; anything else with gn_partial != NULL is an error. */
  float* gn_partial;
  /* != 0: `out` is float [..][ldo] and receives the un-rounded fp32 accumulators (+ bias): partial sums another kernel finishes
   * (dove_conv_out_gather).  Only for plain convs (no act / resid) that dispatch to igemm_fast_kernel; an error otherwise. */
  int out_f32;
  /* nb > 1 (ABI 12): `nb` INDEPENDENT instances of this conv in one launch, laid out back to back along the frame axis -
   * x [nb * t_in, h_in, w_in, cin], out / resid [nb * t_out, ...], gn_partial instance-major (dove_conv_gn_partial_rows(d) / nb rows
   * each).  t_in / t_out stay PER-INSTANCE counts: causal temporal taps, the conv cache and tmode are evaluated inside an instance
   * (instance b's first frames read ITS cache frames, cache + b * cache_stride).  The spatial tiles of diffusers' tiled_encode /
   * tiled_decode (`--is_vae_st`, /root/reference/inference_script.py:642-645) are such instances: each tile sees zero padding at its
   * own border and keeps its own conv cache and GroupNorm scope, so same-shaped tiles run as ONE launch instead of one per tile.
   * Results are those of nb separate calls.  0 / 1 = one instance.  Not combined with gate. */
  int nb;
  /* elements between two instances' cache frames; 0 = (kt-1) * h_in * w_in * cin (a dense [nb][kt-1][h][w][cin] array).  A cache that is
   * a view of the previous frame-batch's input [nb][t_prev][h][w][cin] passes t_prev * h_in * w_in * cin. */
  long long cache_stride;
  /* optional (ABI 12), kt == 3 only: [2][kh*kw][cout_pad][cin] = the temporal weight sums w[0] + w[1] and w[0] + w[1] + w[2] (tap blocks of
   * `w`), formed in fp32 and rounded to bf16 ONCE at pack time.  Without a conv cache (cache == NULL: the first frame-batch of a clip, tile
   * or chunk) CogVideoXCausalConv3d pads the front with the REPLICATED first frame, so output frame 0 is (w0 + w1 + w2) x0 and output frame 1
   * is (w0 + w1) x0 + w2 x1: one and two temporal taps instead of three (3 % of the causal-conv MACs of a 33-frame clip).  Used by
   * conv3x3_halo4x_kernel when cache == NULL; ignored otherwise (NULL: three taps for every frame).  The sums differ from the three separate
   * products by one bf16 rounding of the summed weight - inside the operator tolerance, but a caller that needs the un-summed arithmetic
   * leaves the field NULL. */
  const void* w_first;
  /* optional (ABI 12), up == 1 with a 3x3 (kt == 1) kernel: [4 phases][2x2 taps][cout_pad][cin] = the SUB-PIXEL form of the upsample-fused conv.
   * A nearest x2 upsample followed by a 3x3 conv is, for output phase (py, px) = (oy & 1, ox & 1), a 2x2 conv on the low-res input:
   *   out[2y + py][2x + px] = sum_{a,b in {0,1}} w_sub[2 py + px][2 a + b] . in[y + py - 1 + a][x + px - 1 + b]   (zero outside the frame),
   *   w_sub[2 py + px][2 a + b] = sum of w[dh][dw] over the dh with (py + dh + 1) / 2 == py + a and the dw with (px + dw + 1) / 2 == px + b
   * (integer division), formed in fp32 and rounded to bf16 ONCE at pack time - 4 / 9 of the MACs of Upsample3D's conv.  Used when the low-res grid
   * is at least 16 x 32; NULL = the direct form (upsample folded into the addressing, all 9 taps). */
  const void* w_sub;
  /* optional (ABI 13), kt == 3 only: the caller DECLARES that the input frames of every instance come in bit-identical pairs - the frames
   * CogVideoXUpsample3D's time doubling produces (F.interpolate(scale_factor=2) along t, the first frame kept single when the frame-batch has an
   * odd length; decode_latents, /root/reference/inference_script.py:500), carried unchanged through the per-pixel SpatialNorm + SiLU to the
   * first causal conv of the next up-block.
   *   tdup == 1: pairs (0,1), (2,3), ... ; a conv cache, if any, holds an equal pair too (it is the end of the previous batch's input)
   *   tdup == 2: frame 0 single, pairs (1,2), (3,4), ... ; cache must be NULL (the head of a clip)
   * Two of the three causal taps of every output frame then read the same bits: the launch runs TWO temporal groups per frame instead of
   * three - (w0 + w1) x[t-1] + w2 x[t]  or  w0 x[t-2] + (w1 + w2) x[t]  by frame parity (frames whose three taps all read one frame: one
   * group on w_first's w0 + w1 + w2) - two thirds of the MACs.  w_pair = [2][kh*kw][cout_pad][cin]: the sums w[0] + w[1] and w[1] + w[2]
   * (tap blocks of `w`), formed in fp32 and rounded to bf16 ONCE at pack time, like w_first (which a cache-less launch needs as well).
   * Used by conv3x3_halo4x_kernel; every other kernel ignores the declaration and computes the three taps (the same function of equal frames up
   * to the rounding of the summed weights).  0 / NULL: no declaration. */
  const void* w_pair;
  int tdup;
  int reserved2; /* 0 */
} dove_conv_desc;
int dove_conv_igemm_bf16(const dove_conv_desc* d, void* stream);
/* name of the kernel this call dispatches to (one of igemm_kernel, igemm_fast_kernel, conv3x3_halo4x_kernel, gemm8p_kernel,
 * smallk_kernel) - for reporting (bench.py's per-kernel roofline) and for tests that pin which production shape
 * runs where; the rule is a pure function of the descriptor (no environment switches) */
const char* dove_conv_kernel_name(const dove_conv_desc* d);
/* Partial-tile launches a call makes besides its main launch (reporting / tests; ABI 15): 1 = the last 16 x 32 tile column is walked in
 * 32 x 16 tiles by a second launch - taken when the image ends within the first half of that column (W % 32 in 1..16) AND the two launches
 * need fewer rounds of the persistent grid than one launch (the 240 x 360 tiles of the tiled VAE).  Outputs and fused GroupNorm partial
 * sums do not depend on it (bit-identical). */
int dove_conv_partial_launches(const dove_conv_desc* d);
/* rows of gn_partial this call would write, 0 if its kernel does not fuse the statistics (caller then runs
 * dove_groupnorm_stats_bf16 on the output as before) */
long long dove_conv_gn_partial_rows(const dove_conv_desc* d);
/* stats [32][2] (mean, rstd) from partial [rows][32][2] (deterministic two-level fp64 combine).  count = elements per
 * group = npix * C/32; ws >= 256*64 DOUBLES (128 KiB, 8-byte aligned) of scratch: both levels are fp64. */
int dove_groupnorm_finalize_partials(const float* partial, long long rows, double count, float eps, void* ws, float* stats,
                                     void* stream);

/* nn.GroupNorm(32, C, eps) statistics over one frame-batch [npix, C] (diffusers CogVideoXResnetBlock3D norm1/norm2,
 * encoder.norm_out, and the norm_layer inside CogVideoXSpatialNorm3D).  stats = [32][2] (mean, rstd) fp32.
 * frame_pix = H*W of one frame (npix = frames * frame_pix; 0: treat the tensor as one frame): partial sums are formed per
 * (frame, fixed share of the frame), so a batch split into pieces of whole frames reduces to the same statistics.
 * partial_ws: >= ws_blocks*64 floats of scratch; ws_blocks >= frames * min(256, blocks a frame needs) - 4096 rows never constrain a
 * 9-frame batch; a scratch too small for the call is an ERROR (a lowered block count would make the sums depend on how many frames
 * share the call, which the split-invariance above forbids). */
int dove_groupnorm_stats_bf16(const void* x, long long npix, long long frame_pix, int C, float eps, void* partial_ws, int ws_blocks,
                              float* stats, void* stream);
/* Distributed form (dove_amd.dist, frame-batch split over a rank pair): raw per-group (sum, sum of squares) of one piece
 * as fp64 [32][2] - the ranks add their pieces' sums (and element counts) and call the finalize below, which is the same
 * fp64 mean / rstd arithmetic the single-call form ends with. */
int dove_groupnorm_sums_bf16(const void* x, long long npix, long long frame_pix, int C, void* partial_ws, int ws_blocks, double* sums,
                             void* stream);
/* count <= 0: sums has 65 entries and sums[64] is the element count (the message two ranks of a split frame-batch exchange and add) */
int dove_groupnorm_finalize_sums(const double* sums, double count, float eps, float* stats, void* stream);
/* the same raw sums from the partial rows a conv epilogue wrote (dove_conv_desc.gn_partial): no pass over the tensor */
int dove_groupnorm_sums_from_partials(const float* partial, long long rows, void* ws, double* sums, void* stream);
/* y = silu?( GN(x) [ * yb[z][0:C] + yb[z][C:2C] ] ): GroupNorm apply, optional SpatialNorm3D conditioning from the
 * [Tz,hz,wz,2C] table conv_y(zq)||conv_b(zq) on the latent grid (z = (tmap[t], h>>sshift, w>>sshift), i.e. the
 * nearest-neighbour resize of zq), optional SiLU. */
int dove_groupnorm_apply_bf16(const void* x, void* y, int T, int H, int W, int C, const float* stats,
                              const float* gamma, const float* beta, int silu, const void* yb, int hz, int wz,
                              int sshift, const int* tmap, void* stream);

/* ---- batched forms (ABI 12): `nb` independent instances back to back along the frame axis, each with its own GroupNorm scope - the
 * same-shaped spatial tiles of AutoencoderKLCogVideoX.tiled_encode / tiled_decode (`--is_vae_st`, /root/reference/inference_script.py:
 * 642-645) in ONE launch per operator instead of one per tile (dove_conv_desc.nb is the conv's form).  Each returns what nb separate
 * calls of the un-suffixed function would: the partial sums are keyed by (instance, frame, share of the frame) as before.
 *   stats_nb:             x [nb][npix][C] (npix = pixels of ONE instance, frame_pix of one frame) -> stats [nb][32][2];
 *                         partial_ws >= nb * frames * min(256, ceil(frame_pix / (8192 / (C/8)))) rows of 64 floats (an error otherwise)
 *   finalize_partials_nb: partial [nb][rows][32][2] (dove_conv_desc.gn_partial of a conv with nb instances; rows = rows of ONE
 *                         instance) -> stats [nb][32][2]; ws >= nb * 128 KiB when rows > 1024
 *   apply_nb:             x, y [nb * T, H, W, C], stats [nb][32][2], yb [nb * Tz, hz, wz, 2C], tmap [T] = frame map of ONE instance
 *   avgpool_time_nb:      x [nb][T][frame] -> y [nb][To][frame] */
int dove_groupnorm_stats_nb_bf16(const void* x, int nb, long long npix, long long frame_pix, int C, float eps, void* partial_ws,
                                 int ws_blocks, float* stats, void* stream);
int dove_groupnorm_finalize_partials_nb(const float* partial, long long rows, int nb, double count, float eps, void* ws, size_t ws_bytes,
                                        float* stats, void* stream);
int dove_groupnorm_apply_nb_bf16(const void* x, void* y, int nb, int T, int H, int W, int C, const float* stats, const float* gamma,
                                 const float* beta, int silu, const void* yb, int Tz, int hz, int wz, int sshift, const int* tmap,
                                 void* stream);
int dove_avgpool_time_nb_bf16(const void* x, int nb, int T, long long frame_elems, void* y, void* stream);

/* CogVideoXLayerNormZero / norm_final / AdaLayerNorm: y = LN(x)*gamma+beta, then *(1+scale)+shift with
 * mod = [2 row classes][shift|scale][D] fp32 (rows < split: class 0 = text); mod NULL -> plain LayerNorm. */
int dove_layernorm_modulate_bf16(const void* x, void* y, long long rows, int D, float eps, const float* gamma,
                                 const float* beta, const float* mod, long long split, void* stream);

/* Attention pre-processing of the fused QKV projection [N, 3*heads*64]: per-head LayerNorm(64) on q,k
 * (attn1.norm_q / norm_k), interleaved-pair RoPE on rows >= text_len (apply_rotary_emb), q *= qscale,
 * head-major outputs Qh,Kh [heads][Npad][64] and Vt [heads][64][Npad] (pad must be pre-zeroed).
 * v_order: key order of the Vt rows.  0 = natural.  1 = quad-swapped, what dove_attention_fwd_bf16 reads (Npad % 16 == 0): every
 * 16 consecutive keys are stored [0-3, 8-11, 4-7, 12-15] - the order in which the QK^T MFMA leaves the probabilities in a lane,
 * so that P needs no cross-lane exchange before the PV MFMA.  dove_vt_quad_swap_bf16 converts rows [rows][Npad] between the two
 * orders in place (an involution; for hosts that assemble Vt from natural-order pieces, e.g. after an all-to-all). */
/* norm2 (may be NULL): float [heads][2], receives max over the N rows of |q row|^2 and |k row|^2 of every head, taken from the STORED
 * (bf16-rounded, rotated, scaled) values - what dove_attention_fwd_bf16 needs to bound its scores.  The array is cleared and filled
 * on the stream; a host that shards the rows takes the element-wise maximum of the ranks' arrays (exact, so the sharded result
 * stays bit-identical). */
int dove_qkv_post_bf16(const void* qkv, long long N, long long Npad, int heads, int head_dim, int text_len,
                       const float* gq, const float* bq, const float* gk, const float* bk, const float* cosT,
                       const float* sinT, float qscale, float eps, void* Qh, void* Kh, void* Vt, int v_order, float* norm2, void* stream);
int dove_vt_quad_swap_bf16(void* Vt, long long rows, long long Npad, void* stream);
/* Receive side of the Q' / K' / V^T all-to-all of the sequence/head-parallel DiT (dove_amd.dist; not in the reference: one clip over
 * several GPUs): rq, rk = per source rank i the block [hloc][counts[i]][64], rv = [hloc][64][counts[i]] (natural key order), blocks in
 * rank order -> Qh, Kh [hloc][Npad][64] and Vt [hloc][64][Npad] quad-swapped with zero pad columns: the operands of
 * dove_attention_fwd_bf16 for this rank's hloc heads over all N = sum(counts) rows.  counts is a HOST array of `world` entries. */
/* norm2_out (may be NULL; ABI 12): float [hloc][2].  When given, every source block carries ONE extra row per head (rq, rk: [hloc][counts[i] + 1][64])
 * / column (rv: [hloc][64][counts[i] + 1]) behind its rows, and the extra row of the K block starts with two floats: that rank's
 * (max |q row|^2, max |k row|^2) of the head over ITS rows (dove_qkv_post_bf16's norm2).  norm2_out = their maximum over the ranks = what one
 * GPU computes over all rows, exactly - the attention's score bound rides in the all-to-all payload instead of a collective of its own. */
int dove_ulysses_place_bf16(const void* rq, const void* rk, const void* rv, const long long* counts, int world, int hloc, long long N,
                            long long Npad, void* Qh, void* Kh, void* Vt, float* norm2_out, void* stream);

/* F.scaled_dot_product_attention (no mask, non-causal) on the operands above, Vt in QUAD-SWAPPED key order; Qh carries
 * scale*log2(e).  O [N][ldo] token-major, head h at columns [64h, 64h+64).
 * norm2 (may be NULL; IN/OUT since ABI 14): float [heads][2] = max squared row norms of this call's Qh / Kh heads (dove_qkv_post_bf16).
 * Every head whose two numbers are finite runs on the software-pipelined kernel WITHOUT a softmax shift (shift-invariance: 2^s itself, the
 * constant cancels in O / l; -13 % kernel time against the running maximum at N = 18 226).  That is exact to rounding while a row's sum
 * l = sum_j 2^s_ij stays in [2^-80, 2^100] - guaranteed when the Cauchy-Schwarz bound b = 1.01 sqrt(norm2[h][0] norm2[h][1]) <= 80, and
 * checked per row otherwise: a head with a row outside the window is marked norm2[h][0] = NaN and recomputed, whole, with the running
 * maximum inside the same call.  Heads with a non-finite entry on entry and calls with norm2 == NULL use the running maximum.  On return
 * (stream order) norm2 therefore tells which kernel produced each head (dove_attention_head_paths).  The values only select the path: a
 * stale array costs time, never correctness (ABI <= 13 used b as the shift itself and needed it to describe THESE Qh / Kh). */
int dove_attention_fwd_bf16(const void* Qh, const void* Kh, const void* Vt, void* O, long long N, long long Npad,
                            int heads, int head_dim, long long ldo, float* norm2, void* stream);
/* Which kernel produced each head of a dove_attention_fwd_bf16 call: norm2_host = HOST copy of that call's norm2 taken after it completed
 * (NULL: the call had none); path[h] = 1 "attn_pipe_kernel" (no shift), 0 "attn_fwd_kernel" (running maximum).  Pure host function.
 * dove_attention_path_name(path) names them. */
int dove_attention_head_paths(const float* norm2_host, int heads, int* path);
const char* dove_attention_path_name(int path);

/* layout glue at the [B,C,T,H,W] boundary (B = 1) */
int dove_cl_from_ncthw(const void* x, int dtype, int C, long long npix, int Cp, float scale, float shift, void* y,
                       void* stream);
int dove_ncthw_from_cl(const void* x, long long ld, int C, long long npix, float scale, float shift, float lo,
                       float hi, void* y, int dtype, void* stream);
/* encoder.conv_in (3 -> 128 channels, 3x3x3) with the spatial taps moved into the input channels: [C][T][H][W] -> [T][H][W][Cp] bf16,
 * y[..][(dy*3+dx)*C + c] = x[c][t][h+dy-1][w+dx-1] * scale + shift (0 outside the frame; channels >= 9C zero).  The conv then is a (3,1,1)
 * conv on 27 real input channels (weights re-laid the same way) instead of a 3x3x3 conv on 3 real channels padded to 32. */
int dove_cl_im2col3x3_from_ncthw(const void* x, int dtype, int C, int T, int H, int W, int Cp, float scale, float shift, void* y,
                                 void* stream);
/* decoder.conv_out (128 -> 3 channels, 3x3x3) split by spatial tap: a (3,1,1) conv with 27 (padded 32) output channels
 * P[t][y][x][(dy*3+dx)*C + c] = sum_{kt,ci} x[t+kt-2][y][x][ci] w[c][ci][kt][dy][dx] (dove_conv_igemm_bf16 with out_f32 = 1: K = 3*Cin
 * instead of 27*Cin per staged pixel, and no 32/3 padding waste on the MFMAs) followed by this gather:
 * y[c][t][oy][ox] = clamp(bf16(bias[c] + sum_{dy,dx} P[t][oy+dy-1][ox+dx-1][(dy*3+dx)*C + c]) * scale + shift, lo, hi), zero padding at
 * the frame border; the bf16 rounding is the conv's own output rounding in the reference. */
int dove_conv_out_gather(const float* p, long long ldp, int T, int H, int W, int C, const float* bias, float scale, float shift, float lo,
                         float hi, void* y, int dtype, void* stream);
/* CogVideoXDownsample3D temporal average pool (odd T keeps the first frame) */
int dove_avgpool_time_bf16(const void* x, int T, long long frame_elems, void* y, void* stream);
/* DiagonalGaussianDistribution.sample(): out[c] = mean + exp(0.5*clamp(logvar,-30,20)) * noise  (ref :409) */
int dove_posterior_sample(const void* moments, long long ld, int latent_channels, long long npix, const void* noise,
                          int noise_dtype, void* out, int out_dtype, void* stream);
/* out = a*x + b*y : CogVideoXDPMScheduler.get_velocity / add_noise (ref :457,491-493) */
int dove_axpby(const void* x, const void* y, void* out, int dtype, long long n, float a, float b, void* stream);
/* CogVideoXPatchEmbed gather / transformer un-patchify between [T,C,h,w] and tokens [Nv][C*pt*p*p] */
int dove_patchify(const void* x, int dtype, int T, int C, int H, int W, int pt, int p, void* tokens, long long ld,
                  void* stream);
int dove_unpatchify(const void* tokens, long long ld, int T, int C, int H, int W, int pt, int p, void* y, int dtype,
                    void* stream);
/* The same gather for a SPATIAL TILE of diffusers' tiled_decode (`--is_vae_st`, /root/reference/inference_script.py:642-645): the tile is
 * cross-faded with its neighbours in the channels-last layout before the clip changes layout, so the result stays channels-last:
 * y[t][oy][ox][c] = bf16(bias[c] + sum ...) for c < C, 0 for C <= c < ldy; bf16 [T,H,W,ldy], C <= ldy <= 32, ldy % 4 == 0; no range map.
 * T may be nb x frames (tile-major batch): frames are independent.  (ABI 15) */
int dove_conv_out_gather_cl(const float* p, long long ldp, int T, int H, int W, int C, const float* bias, void* y, int ldy, void* stream);
/* Spatial tiles of diffusers' tiled_encode / tiled_decode as ONE tile-major batch (dove_conv_desc.nb): out [nb][nt][th][tw][C] <-
 * x [T][H][W][C] bf16 channels-last, frames [t0, t0 + nt), tile n at (oy[n], ox[n]) (HOST arrays, nb <= 64), C % 8 == 0.
 * im2col_cin > 0: x is the im2col'ed clip of dove_cl_im2col3x3_from_ncthw with C = im2col_cin input channels; the channels of taps that
 * reach outside the TILE are zeroed at the tile's border pixels (each tile sees zero padding at its own border), so that the batch equals
 * the im2col of the cropped tiles bit for bit and encoder.conv_in runs in its (3,1,1) form inside tiles too.  (ABI 15) */
int dove_tile_gather_bf16(const void* x, int H, int W, int C, int t0, int nt, int th, int tw, int nb, const int* oy, const int* ox,
                          int im2col_cin, void* out, void* stream);
/* AutoencoderKLCogVideoX.blend_v / blend_h of the spatial-tiling path (`enable_tiling`, ref :644-645): in-place linear
 * cross-fade of the first `extent` rows (axis 0) / columns (axis 1) of tile b with the last ones of its neighbour a;
 * channels-last tiles [T,H,W,ld], ld multiple of 4. */
int dove_blend_edge_bf16(const void* a, void* b, int T, int Ha, int Wa, int Hb, int Wb, int ld, int extent, int axis,
                         void* stream);
/* Script-level pre/post-processing of /root/reference/inference_script.py on the GPU:
 * preprocess: frames [F0,H0,W0,3] u8 -> [3, F0+pad_f, (H0+pad_h)*up, (W0+pad_w)*up] in [-1,1]: pad F by repeating the last frame,
 *   pad H/W with zeros bottom/right (ref :220-232), bilinear x`up` with align_corners=False (ref :672), x/255*2-1 (ref :674).
 * postprocess: video [3,F,H,W] in [0,1] -> frames [Fo,Ho,Wo,3] u8 = trunc(clamp(x*255,0,255)), cropping the padding
 *   (ref :238-246, :124). */
int dove_preprocess_u8(const void* frames, int F0, int H0, int W0, int pad_f, int pad_h, int pad_w, int upscale, void* out,
                       int out_dtype, void* stream);
int dove_postprocess_u8(const void* video, int dtype, int F, int H, int W, int Fo, int Ho, int Wo, void* out, void* stream);

/* Full-reference metrics of the reference's evaluation step (eval_metrics.py; pyiqa 'psnr' and 'ssim' defaults; INTEGRATION.md 'Metrics'):
 * per image n of a batch, out[n][0] = PSNR in dB and out[n][1] = SSIM (fp64, device memory; NaN for a metric not asked for).
 * Each input is a strided view: element (n, c, y, x) is at data + n*sn + c*sc + y*sh + x*sw elements, so [F,H,W,3] u8 frames, [3,F,H,W]
 * decoder output and border / resolution crops (a pointer offset plus a smaller h x w) are read in place.  dtype: DOVE_F32, DOVE_BF16, or
 * DOVE_U8 (read as value / 255).  flags: DOVE_METRIC_PSNR and/or DOVE_METRIC_SSIM, optionally DOVE_METRIC_RGB_TO_Y (eval_metrics.py
 * --test_y_channel: y = 0.257 r + 0.504 g + 0.098 b + 0.0625 before both metrics; needs channels == 3).  channels: 1 or 3; SSIM needs
 * h, w >= 11.  ws: device scratch of dove_fr_metrics_workspace_bytes(n, h, w) bytes.  Deterministic: two calls give identical bits. */
#define DOVE_U8 2
#define DOVE_METRIC_PSNR 1
#define DOVE_METRIC_SSIM 2
#define DOVE_METRIC_RGB_TO_Y 4
typedef struct dove_image_view {
  const void* data;
  int dtype;
  int reserved;
  long long sn, sc, sh, sw;
} dove_image_view;
size_t dove_fr_metrics_workspace_bytes(int n, int h, int w);
int dove_fr_metrics(const dove_image_view* pred, const dove_image_view* ref, int n, int channels, int h, int w, int flags, void* ws,
                    size_t ws_bytes, double* out, void* stream);
/* Colour fix of restored frames against their upscaled input (the reference's finetune/scripts/color_fix_util.py):
 * content (the SR result) keeps its detail and takes the colour of style (the upscaled low-quality input).  content, style and out are
 * strided [n,3,h,w] views as above, every frame on its own; input dtypes DOVE_F32 / DOVE_BF16 / DOVE_U8 (read as value / 255), each
 * followed by the affine  v = scale * raw + bias  (a [-1,1] clip is read as 0.5 x + 0.5 without a copy).
 *   DOVE_COLORFIX_WAVELET: out = content + low5(style - content), low5 = five 3x3 [1,2,1]x[1,2,1]/16 blurs of dilation 1, 2, 4, 8, 16,
 *     each on its replicate-padded input (= wavelet_reconstruction: (content - low5(content)) + low5(style)); any h, w >= 1.
 *   DOVE_COLORFIX_ADAIN: out = (content - mean_c) / std_c * std_s + mean_s per frame and channel, std = sqrt(unbiased var + 1e-5)
 *     (= adaptive_instance_normalization); needs h * w >= 2.
 * out dtype DOVE_F32 / DOVE_BF16: the fp32 result (clamped to [0,1] with DOVE_COLORFIX_CLAMP); DOVE_U8: trunc(clamp(x,0,1) * 255), the rule
 * of dove_postprocess_u8, so out may be the final [F,H,W,3] frames.  out may be the very view given as content or style (same pointer,
 * strides and dtype), not a shifted or differently strided window onto one of them.  ws: device scratch of
 * dove_color_fix_workspace_bytes(mode, n, h, w) bytes.  fp32 arithmetic (adain: fp64 statistics); two calls give identical bits. */
#define DOVE_COLORFIX_WAVELET 1
#define DOVE_COLORFIX_ADAIN 2
#define DOVE_COLORFIX_CLAMP 1
size_t dove_color_fix_workspace_bytes(int mode, int n, int h, int w);
int dove_color_fix(const dove_image_view* content, float c_scale, float c_bias, const dove_image_view* style, float s_scale, float s_bias,
                   int n, int h, int w, int mode, int flags, const dove_image_view* out, void* ws, size_t ws_bytes, void* stream);
/* 8-bit RGB <-> planar YUV for YUV4MPEG2 video I/O (tests/yuv_ref.py is the bit-exact definition).  Integer fixed
 * point with 16 fractional bits: the caller passes the 3x3 matrix as rint(c * 65536) and the offsets (16 or 0, 128, 128); a result is
 * rounded once (+ half before the final arithmetic shift) and clamped to 0..255.  A frame payload is the Y plane [h,w], then U, then V
 * (DOVE_YUV_444: [h,w]; DOVE_YUV_422: [h, ceil(w/2)]; DOVE_YUV_420: [ceil(h/2), ceil(w/2)]; DOVE_YUV_MONO: none), contiguous and
 * dove_yuv_frame_bytes long (0 for a bad argument) - what follows "FRAME\n" in a Y4M stream.
 * rgb_to_yuv: rgb is a strided [n,3,h,w] view as above (u8 frames [F,H,W,3], or [3,F,H,W] f32 / bf16 decoder output in [0,1] and crops
 *   of it); a float sample is first quantised as dove_postprocess_u8 does, trunc(clamp(x*255,0,255)).  offset[] is added to Y, U, V.
 *   422 chroma: [1 2 1]/4 at even x (left co-sited); 420: mean of the 2x2 block (centre-sited, C420jpeg); edges replicate; the filter
 *   runs on the un-rounded products.  out: n payloads.
 * yuv_to_rgb: yuv holds n payloads; offset[] is subtracted from Y, U, V; out is [n,h,w,3] u8.  Chroma is upsampled bilinearly with
 *   integer weights (sum 4 per axis, neighbours clamped) and enters the matrix product still scaled: 420 vertical 3:1 towards the nearer
 *   sample; 420 horizontal 3:1 when siting_h is DOVE_YUV_SITING_CENTRE (C420jpeg), else 4:0 at even x and 2:2 at odd x (C420mpeg2,
 *   C420paldv), as 422 always is.  DOVE_YUV_MONO gives grey RGB. */
#define DOVE_YUV_444 0
#define DOVE_YUV_422 1
#define DOVE_YUV_420 2
#define DOVE_YUV_MONO 3
#define DOVE_YUV_SITING_LEFT 0
#define DOVE_YUV_SITING_CENTRE 1
typedef struct dove_yuv_format {
  int coef[9];   /* row-major 3x3: rows Y, U, V (forward) or R, G, B (inverse) */
  int offset[3];
  int chroma;    /* DOVE_YUV_444 / 422 / 420 / MONO */
  int siting_h;  /* DOVE_YUV_SITING_*: read by yuv_to_rgb for DOVE_YUV_420 only */
} dove_yuv_format;
size_t dove_yuv_frame_bytes(int h, int w, int chroma);
int dove_rgb_to_yuv_u8(const dove_image_view* rgb, int n, int h, int w, const dove_yuv_format* fmt, void* out, void* stream);
int dove_yuv_to_rgb_u8(const void* yuv, int n, int h, int w, const dove_yuv_format* fmt, void* out, void* stream);
/* M = 1 linear with optional SiLU on the input (time_embedding MLP, norm*.linear modulation vectors) */
int dove_gemv_bf16(const void* W, const float* bias, const float* x, int in_features, int out_features, int act_in,
                   float* y, void* stream);

/* ---- MXFP8 linears (BASELINE configs[4]: fp8 MFMA path of the DiT, PSNR-gated against the bf16 path) --------------------
 * OCP microscaling FP8: e4m3fn elements, one E8M0 (power-of-two) scale per 32 consecutive K elements of a row, for BOTH
 * operands of an nn.Linear of CogVideoXBlock (attn1.to_q/k/v fused, attn1.to_out.0, ff.net.0.proj, ff.net.2;
 * /root/reference/inference_script.py:483-489).  The scales are applied inside v_mfma_scale_f32_32x32x64_f8f6f4.
 * dove_mx_quant_bf16: x bf16 [rows][K] (K % 256 == 0) -> q u8 [rows][K] and scales u32 [K/256][rows][2]; word (c, r, h),
 *   byte u = E8M0 scale of row r's block 8c + 2u + h; scale = 2^ceil(log2(amax/448)) (no clipping), q = RNE_e4m3(x/scale).
 * dove_linear_mxfp8: out [M][ldo] bf16 = epilogue((xq.xs) (wq.ws)^T + bias) with the epilogue of dove_conv_igemm_bf16
 *   (act 1 = GELU(tanh); resid / gate [2][N] fp32 / gate_split as there); N % 256 == 0, K % 256 == 0. */
int dove_mx_quant_bf16(const void* x, long long rows, int K, void* q, void* scales, void* stream);
int dove_linear_mxfp8(const void* xq, const void* xs, const void* wq, const void* ws, const float* bias, const void* resid,
                      const float* gate, void* out, long long M, int N, int K, long long ldo, long long ldr, long long gate_split,
                      int act, void* stream);

/* MXFP8 attention (csrc/attention_mx.hip; same configs[4] variant): dove_qkv_post_bf16's pre-processing with e4m3 outputs -
 * Q8 [heads][Npad][64] = e4m3(q * qscale * 8) (fixed block scale 2^-3), K8 [heads][Npad][64] = e4m3(k) (scale 2^0),
 * V8t [heads][64][Npad] e4m3 with one E8M0 scale per (d, 32 consecutive keys): Vs u8 [heads][Npad/64][64][2].
 * Every row of the padded buffers is written (pad = zeros); Npad % 128 == 0.
 * dove_attention_fwd_mxfp8: softmax(Q K^T) V on those operands, probabilities quantised per (query, 64-key tile) in
 * registers; O as dove_attention_fwd_bf16. */
int dove_qkv_post_mxfp8(const void* qkv, long long N, long long Npad, int heads, int head_dim, int text_len,
                        const float* gq, const float* bq, const float* gk, const float* bk, const float* cosT,
                        const float* sinT, float qscale, float eps, void* Q8, void* K8, void* V8t, void* Vs,
                        void* stream);
int dove_attention_fwd_mxfp8(const void* Q8, const void* K8, const void* V8t, const void* Vs, void* O, long long N,
                             long long Npad, int heads, int head_dim, long long ldo, void* stream);

/* ---- T5 text encoder operators (non-empty prompts only: `pipe.text_encoder(ids)[0]`, /root/reference/inference_script.py:429-444;
 * transformers' T5EncoderModel of CogVideoX1.5: T5-v1.1-XXL, 24 blocks, d_model 4096, 64 heads x 64, gated-GELU d_ff 10240) ----
 * T5LayerNorm: y = weight * x * rsqrt(mean(x^2) + eps) (fp32 statistics; no mean subtraction, no bias) */
int dove_rmsnorm_bf16(const void* x, void* y, long long rows, int D, float eps, const float* weight, void* stream);
/* T5DenseGatedActDense: y [M][F] = gelu_new(x[:, :F]) * x[:, F:2F] on the fused wi_0 || wi_1 projection */
int dove_gated_gelu_bf16(const void* x, void* y, long long M, int F, void* stream);
/* T5Attention (encoder self-attention, no mask): out [N][ldo] = softmax(q k^T + bias[h]) v per head; q/k/v token-major with
 * row stride ld (views into the fused projection), head h at columns [64h, 64h+64); NO 1/sqrt(d) scaling; bias [H][N][N]
 * fp32 = relative_attention_bias gathered by bucket; N <= 1024 */
int dove_attention_bias_bf16(const void* q, const void* k, const void* v, long long ld, const float* bias, void* out, long long ldo,
                             int N, int heads, int head_dim, void* stream);

/* ---- graph-level entry points: a context owns packed weights + one workspace arena and runs whole stages ----
 * One context per (process, device); NOT thread-safe; calls are asynchronous on the given stream except where a host-side
 * table has to be uploaded (first call with a new shape / timestep).  Weight tensors passed to dove_set_weight are BORROWED until
 * dove_finalize_weights returns (it repacks them into library-owned memory: implicit-GEMM layout for every conv / linear,
 * fused QKV, SpatialNorm conv_y || conv_b, fp32 norm parameters).  Names are diffusers' state-dict names of
 * AutoencoderKLCogVideoX (`encoder.*`, `decoder.*`) and CogVideoXTransformer3DModel (everything else); SURVEY.md App. E. */
typedef struct dove_ctx dove_ctx;
typedef struct dove_model_config {
  /* vae/config.json */
  int vae_in_channels, vae_out_channels, vae_latent_channels, vae_num_blocks, vae_block_out_channels[8], vae_layers_per_block,
      vae_temporal_compression, vae_enc_batch /* num_sample_frames_batch_size */, vae_dec_batch /* num_latent_frames_batch_size */;
  float vae_norm_eps, vae_scaling_factor;
  /* transformer/config.json */
  int dit_heads, dit_head_dim, dit_num_layers, dit_in_channels, dit_out_channels, dit_patch, dit_patch_t, dit_text_dim,
      dit_time_embed_dim, dit_max_text, dit_flip_sin_to_cos;
  float dit_norm_eps, dit_freq_shift;
} dove_model_config;
/* optional precomputed inputs of the DiT (all device pointers, may be NULL): RoPE tables [Nv][64] fp32 as
 * `prepare_rotary_positional_embeddings` returns them (ref :364-392) and the bf16-rounded sinusoidal timestep projection [D] fp32;
 * NULL = computed inside (host libm + upload, cached per shape / timestep) */
typedef struct dove_dit_aux { const float* rope_cos; const float* rope_sin; const float* timestep_proj; } dove_dit_aux;
int dove_create(int hip_device, const dove_model_config* cfg, dove_ctx** out);
/* ---- one clip on several GPUs (BASELINE configs[2]) ----
 * One context per rank (process or thread, one GPU each).  With a communicator set,
 *  - dove_vae_encode / dove_vae_decode run only THIS rank's share of the frame-batches (diffusers' num_sample_frames_batch_size /
 *    num_latent_frames_batch_size batching): every CogVideoXCausalConv3d of the rank's first work item receives its conv_cache (the last
 *    kt-1 input frames the previous item would have left) from rank-1, and sends its own to rank+1 after the rank's last - point-to-point, in
 *    layer order, on the context's own receive / send streams (ABI 14): the transport callbacks are handed THOSE streams for halos, the
 *    caller's stream only waits on events (receives are pre-posted from the second call with a given stage and shape on).  With at most as many ranks as frame-batches the items are whole batches; with MORE ranks (ABI 12)
 *    batches are split into PAIRED PIECES on consecutive ranks - 8 ranks on a 33-frame clip decode 5,4,4,4,4,4,4,4 frames, BASELINE's
 *    "frame-chunk = 4" - and every GroupNorm of a piece swaps 65 doubles (per-group sum, sum of squares, element count) with its partner, so the
 *    statistics are the whole batch's.  Only the frames dove_shard_frames reports are written to the output buffer;
 *  - dove_dit_forward (ABI 12) shards ONE sample over the ranks: rows of the token-major residual stream for every row-local operator,
 *    heads for attention, one all-to-all of Q' / K' / V^T and one of the attention output per layer (the score bound rides in the K blocks);
 *    v_out is complete on every rank.  dit_heads must be a multiple of nranks;
 *  - dove_sr_clip (ABI 12) chains them: encode, gather of the posterior moments, the sharded DiT, decode - every rank passes the SAME clip,
 *    noise and text and gets ITS frames of video_out (dove_shard_frames(ctx, 1, T, ...)); gathering them is the caller's.
 * Every result is bit-identical to the single-GPU call (tests/test_graph_gpu.py plays 2 - 8 ranks as threads on one GPU).
 * dove_comm_init: RCCL transport (librccl opened at run time; the 128-byte id from dove_comm_unique_id on rank 0, distributed by the host;
 * every symmetric exchange is one ncclGroup; the halos of the two directions travel on two further communicators made with ncclCommSplit).
 * dove_comm_init_custom: any transport - send / recv of `bytes` device bytes to / from rank `peer`, ordered on `stream`, matched in order per
 * (source, destination) pair.  `stream` is the caller's for the symmetric exchanges and one of the context's two internal streams for
 * halos: a transport that hands data from the sender's stream to the receiver's must order the two itself (an event per message).  Because
 * a custom transport has no channels, halo receives are posted ahead only for work items whose GroupNorm partner is not rank - 1 (the pair
 * sums would share the halos' message order); under RCCL the halos have communicators of their own and are always posted ahead. */
typedef int (*dove_xfer_fn)(void* user, int peer, void* dev_ptr, size_t bytes, void* stream);
/* Bracket of ONE exchange (ABI 12).  The paired-piece VAE swaps 65 doubles with a partner per GroupNorm and the sharded DiT runs all-to-alls:
 * symmetric patterns in which every rank sends and receives.  A transport whose send rendezvous with the peer's receive (RCCL) must see the
 * calls of such an exchange as one group (dove_comm_init does this with ncclGroupStart / ncclGroupEnd); a custom transport either BUFFERS its
 * sends (then no bracket is needed: the library issues all sends of an exchange before its receives, and in a pair swap the lower rank
 * sends first) or provides the two callbacks here. */
typedef int (*dove_group_fn)(void* user, void* stream);
int dove_comm_set_group(dove_ctx* ctx, dove_group_fn begin, dove_group_fn end);
int dove_comm_unique_id(void* out128);
int dove_comm_init(dove_ctx* ctx, const void* nccl_unique_id, int rank, int nranks);
int dove_comm_init_custom(dove_ctx* ctx, int rank, int nranks, dove_xfer_fn send, dove_xfer_fn recv, void* user);
void dove_comm_destroy(dove_ctx* ctx);
/* stage 0 = dove_vae_encode (n = pixel frames F -> latent frames), stage 1 = dove_vae_decode (n = latent frames T -> pixel frames) */
int dove_shard_frames(dove_ctx* ctx, int stage, int n, int* first, int* count);
/* number of ranks that get work for this stage and clip length under the context's communicator (whole batches, or paired pieces when there
 * are more ranks than batches); on a single-rank context: the most ranks that could (two per splittable frame-batch) */
int dove_comm_useful_ranks(dove_ctx* ctx, int stage, int n);
void dove_destroy(dove_ctx* ctx);
/* ---- options of the graph level: the reference's switches that change what a stage computes ----
 * DOVE_OPT_VAE_TILING (value 0 / 1): pipe.vae.enable_tiling() (`--is_vae_st`, /root/reference/inference_script.py:643-645; every
 *   published number of the reference ran with it): dove_vae_encode / dove_vae_decode / dove_sr_clip run diffusers' spatial tiling
 *   whenever the clip is larger than one tile - tile = sample/2 px (sample/16 latents), strides 5/6 and 4/5 of it, linear
 *   cross-fade of the overlaps, every tile with its own GroupNorm scope and conv caches.  Not combined with a multi-rank context.
 * DOVE_OPT_VAE_SAMPLE_HEIGHT / _WIDTH (px): vae/config.json sample_height / sample_width (defaults 480 / 720).
 * DOVE_OPT_DIT_LINEAR_MXFP8 (0 / 1; BASELINE configs[4], not a reference option; never the headline dtype): attn1.to_q/k/v,
 *   attn1.to_out.0, ff.net.0.proj and ff.net.2 of every block in MXFP8.  Choose BEFORE dove_finalize_weights: the weights are
 *   quantised there and their bf16 copies dropped.
 * DOVE_OPT_DIT_ATTN_MXFP8 (0 / 1; same variant): attention on dove_qkv_post_mxfp8 / dove_attention_fwd_mxfp8; any time.
 * DOVE_OPT_WEIGHT_SUMS: see below.
 * Stage results with an option set are bit-identical to the Python facade with the same switch (tests/test_graph_gpu.py). */
#define DOVE_OPT_VAE_TILING 1
#define DOVE_OPT_VAE_SAMPLE_HEIGHT 2
#define DOVE_OPT_VAE_SAMPLE_WIDTH 3
#define DOVE_OPT_DIT_LINEAR_MXFP8 4
#define DOVE_OPT_DIT_ATTN_MXFP8 5
/* DOVE_OPT_WEIGHT_SUMS (0 / 1, default 1; any time): 0 = the VAE never hands the pack-time weight sums (dove_conv_desc.w_first / w_sub /
 * w_pair) to its convolutions - every launch computes the reference's per-tap arithmetic (+7.6 % conv MACs), for a caller who wants a
 * checkpoint validated without the one extra bf16 rounding of the summed weights.  The Python facade's switch: pipe.vae.weight_sums. */
#define DOVE_OPT_WEIGHT_SUMS 6
/* DOVE_OPT_VAE_STREAMS (1 / 2, default 2; any time; ABI 14): 2 = the frame-batches of an un-tiled, single-rank dove_vae_encode / dove_vae_decode
 * alternate between the caller's stream and one internal stream, ordered by one event per causal conv (the conv cache is the only dependency
 * between frame-batches); the caller's stream continues behind both when the stage returns.  Same kernels on the same inputs: bit-identical
 * to 1; +1.5 % per clip; the arena's high water grows by about a half (dove_workspace_bytes accounts for it).  The Python facade's switch:
 * pipe.vae.n_streams. */
#define DOVE_OPT_VAE_STREAMS 7
/* read-only counters of the LAST dove_vae_encode / dove_vae_decode of a multi-rank context (dove_get_option; ABI 14): halos this rank received
 * from receives posted before the stage's first kernel / posted where they were consumed (the first pass over a (stage, shape) records the
 * list, later passes pre-post it), halos sent; DOVE_STAT_HALO_COMMUNICATORS: 3 = RCCL with one communicator per halo direction + the main
 * one, 1 = RCCL without ncclCommSplit (one communicator, nothing pre-posted), 0 = custom transport / single rank. */
#define DOVE_STAT_HALO_PREPOSTED 100
#define DOVE_STAT_HALO_BLOCKING 101
#define DOVE_STAT_HALO_SENT 102
#define DOVE_STAT_HALO_COMMUNICATORS 103
int dove_set_option(dove_ctx* ctx, int option, long long value);
long long dove_get_option(dove_ctx* ctx, int option); /* -1: unknown option */
int dove_set_weight(dove_ctx* ctx, const char* name, const void* dev_ptr, const long long* shape, int ndim, int dtype);
int dove_finalize_weights(dove_ctx* ctx);
/* arena bytes a [3,F,H,W] clip needs (upper bound); dove_set_workspace(ctx, NULL, n) lets the library allocate, a non-NULL pointer
 * lends caller memory; with neither the first stage call allocates dove_workspace_bytes itself */
size_t dove_workspace_bytes(dove_ctx* ctx, int F, int H, int W);
int dove_set_workspace(dove_ctx* ctx, void* dev_ptr, size_t bytes);
size_t dove_workspace_high_water(dove_ctx* ctx);
/* pipe.vae.encode(x).latent_dist.parameters (ref :408): x [3][F][H][W] -> moments [2L][T][H/8][W/8]; T is the sum over the frame-batches
 * of what each leaves behind the temporal 2:1 stages = 1 + (F-1)/4 at the default vae_enc_batch of 8 (the counts of dove_shard_frames
 * (ctx, 0, F, ...) over the ranks add up to it) */
int dove_vae_encode(dove_ctx* ctx, const void* x, int dtype, int F, int H, int W, void* moments_out, int out_dtype, void* stream);
/* pipe.transformer(...)[0] for one sample (ref :483-489): hidden [T][C][h][w], text [L][text_dim] bf16 -> v [T][C][h][w] */
int dove_dit_forward(dove_ctx* ctx, const void* hidden, int dtype, int T, int h, int w, const void* text, int L, int timestep,
                     const dove_dit_aux* aux, void* v_out, int out_dtype, void* stream);
/* pipe.vae.decode(z * prescale).sample (ref :500-501; range01 != 0 fuses (x*0.5+0.5).clamp(0,1)): z [L][T][h][w] -> [3][F][8h][8w],
 * F = dove_vae_decode_num_frames(T) = 1 + 4(T-1) for the odd T of 8N+1-frame clips */
int dove_vae_decode_num_frames(dove_ctx* ctx, int T);
int dove_vae_decode(dove_ctx* ctx, const void* z, int dtype, int T, int h, int w, float prescale, int range01, void* video_out,
                    int out_dtype, void* stream);
/* `--noise_step n` (ref :449-457; 0 = off = NULL): the latent handed to the DiT is first noised,
 * latent <- sqrt_alpha * latent + sqrt_one_minus_alpha * eps with the scheduler's alpha_n (cast to the latent dtype first, like
 * diffusers' add_noise) and eps [T'][L][h][w] (the DiT's input layout, T' = T + T % patch_t) drawn by the caller. */
typedef struct dove_pre_noise { const void* eps; int eps_dtype; float sqrt_alpha, sqrt_one_minus_alpha; } dove_pre_noise;
/* process_video (ref :394-503) with the posterior noise injected and the scheduler's sqrt(alpha_t), sqrt(1 - alpha_t) (alpha cast
 * to bf16 first, like diffusers): video_in [3][F][H][W] in [-1,1] -> video_out [3][F][H][W] in [0,1]; pre_noise may be NULL */
int dove_sr_clip(dove_ctx* ctx, const void* video_in, int dtype, int F, int H, int W, const void* noise, int noise_dtype, const void* text,
                 int text_len, int timestep, float sqrt_alpha, float sqrt_one_minus_alpha, const dove_dit_aux* aux,
                 const dove_pre_noise* pre_noise, void* video_out, int out_dtype, void* stream);

/* ---- whole videos from C: the script around process_video (/root/reference/inference_script.py:192-361, :670-731) ----
 * Host planner: pure host functions (no GPU, no context), the integer logic of dove_amd/tiling.py and dove_amd.stream.ChunkPlanner.  Boxes are
 * six ints (t0, t1, h0, h1, w0, w1), half-open.  The functions that fill a list return the number of entries (>= 0) and write at most `cap`
 * of them (a NULL list only counts), or a negative DOVE_E* code with the reference's message in dove_last_error().
 *   dove_plan_padding:     preprocess_video_match(is_match=True) (ref :220-232): frames -> 8N+1 (repeat the last), H and W -> multiples of 16.
 *   dove_plan_output_size: (H + pad_h) * upscale - pad_h * 4, likewise W: the reference crops pad * 4 whatever --upscale is (ref :731).
 *   dove_plan_temporal_chunks: make_temporal_chunks (ref :255-279), chunks [n][2]; chunk_len 0 = one chunk; a short tail is merged into its
 *     predecessor; "chunk_len must be greater than overlap" otherwise.  A clip of <= overlap_t frames has NO chunk (0 is returned).
 *   dove_plan_spatial_tiles: make_spatial_tiles (ref :282-329), tiles [n][4] = (h0, h1, w0, w1); a zero tile size = one tile; the last row /
 *     column is merged; "Tile size must be greater than overlap" otherwise.
 *   dove_plan_valid_region: get_valid_tile_region (ref :332-361) of `piece` inside a clip of F x H x W: half of each interior overlap is
 *     dropped.  valid = the kept box in the piece's own coordinates, out = where it lands in the clip.
 *   dove_plan_pieces: the work list of ref :565-574, :682-683 (dove_amd.tiling.plan), chunk-major and tile-minor, overlaps zeroed on an untiled
 *     axis (chunk_len 0 / tile size (0, 0)): piece, valid and out boxes [n][6] each (any may be NULL).
 *   dove_plan_check_coverage: "every voxel written exactly once" (ref :724-729) for n out-boxes [n][6] in a domain of F x H x W, on the
 *     boxes themselves (no per-voxel counts): a hole fails with "Error: Lack of write in region !!!", else a double write with
 *     "Error: Write count > 1 in region !!!" - the reference's two messages, in the reference's order.
 *   dove_chunk_planner_*: make_temporal_chunks one chunk at a time, without the frame count up front.  need: frames that must be known
 *     (counted from the start of the stream) before next() may be called without eof = start + 2 * chunk_len - overlap_t; -1 for chunk_len 0
 *     (one chunk of the whole clip: needs the end of the stream).  next(known, eof): returns 1 and the chunk [t0, t1) with last != 0 when it is
 *     the final one, 0 when no chunk is left (a clip of <= overlap_t frames: none at all), negative when called too early. */
int dove_plan_padding(int F, int H, int W, int* pad_f, int* pad_h, int* pad_w);
int dove_plan_output_size(int H, int W, int upscale, int* out_h, int* out_w);
int dove_plan_temporal_chunks(int F, int chunk_len, int overlap_t, int* chunks, int cap);
int dove_plan_spatial_tiles(int H, int W, int tile_h, int tile_w, int overlap_h, int overlap_w, int* tiles, int cap);
int dove_plan_valid_region(const int* piece, int F, int H, int W, int overlap_t, int overlap_h, int overlap_w, int* valid, int* out);
int dove_plan_pieces(int F, int H, int W, int chunk_len, int overlap_t, int tile_h, int tile_w, int overlap_h, int overlap_w, int* pieces,
                     int* valid, int* out, int cap);
int dove_plan_check_coverage(const int* boxes, int n, int F, int H, int W);
typedef struct dove_chunk_planner dove_chunk_planner;
int dove_chunk_planner_create(int chunk_len, int overlap_t, dove_chunk_planner** out);
long long dove_chunk_planner_need(const dove_chunk_planner* p);
int dove_chunk_planner_next(dove_chunk_planner* p, long long known, int eof, long long* t0, long long* t1, int* last);
void dove_chunk_planner_destroy(dove_chunk_planner* p);

/* Counter-based normal generator (csrc/video.hip; tests/randn_ref.py is the definition in numpy): what a host without torch's generator
 * draws the VAE posterior noise from.  Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9,
 * 0xBB67AE85), key = (seed low, seed high), counter = (block low, block high, stream_id low, stream_id high).  The four output words
 * x0..x3 of block b are the elements 4b..4b+3 of the stream: element e is word e % 4 of block e / 4.  The call writes the n elements
 * [offset, offset + n) of stream (seed, stream_id), so any split of a tensor over calls gives the same values.
 *   dove_philox_u32: the raw words (uint32), exact.
 *   dove_randn: standard normals by two Box-Muller pairs per block:  u1 = (x0 + 1) 2^-32, u2 = x1 2^-32, r = sqrt(-2 ln u1),
 *     (z0, z1) = (r cos 2 pi u2, r sin 2 pi u2), and (z2, z3) likewise from (x2, x3).  fp32 arithmetic (u1 above 1/2 goes through
 *     log1p of the exact complement); INTEGRATION.md 1e gives the measured distance from the fp64 evaluation.  dtype DOVE_F32, or DOVE_BF16 =
 *     the round-to-nearest-even of that fp32 value.  Deterministic: the bits do not depend on the launch geometry or on the split. */
int dove_philox_u32(void* out, long long n, unsigned long long seed, unsigned long long stream_id, unsigned long long offset, void* stream);
int dove_randn(void* out, int dtype, long long n, unsigned long long seed, unsigned long long stream_id, unsigned long long offset,
               void* stream);

/* Degradation synthesis (csrc/degrade.hip; tests/degrade_ref.py is the definition in numpy): the operators of a
 * RealESRGAN-style low-quality pipeline - blur, resize, Gaussian / Poisson noise, JPEG - on frames x, out [n][h][w][3] fp32, contiguous, in
 * the 0..255 scale, not clipped between steps.  Every frame on its own; out must not alias x.  Per-frame parameters (sigma, scale, quality)
 * are HOST arrays of n entries.  Two calls give identical bits, and a clip split over calls gives the bits of one call.
 *   blur2d: cv2.filter2D(x, -1, kernel): correlation, anchor at the centre, BORDER_REFLECT_101 (dcb|abcd|cba).  kernel: device fp32 [k][k]
 *     (per_frame 0) or [n][k][k] (per_frame 1), k odd in 3..21; h, w > k / 2.  fp32 FMA, taps in row-major order.
 *   resize: -> out [n][oh][ow][3].  DOVE_RESIZE_BILINEAR / DOVE_RESIZE_BICUBIC: half-pixel centres, indices clamped at the border, cubic
 *     A = -0.75 (torch's F.interpolate with align_corners=False, antialias=False; OpenCV's INTER_LINEAR / INTER_CUBIC rule).
 *     DOVE_RESIZE_AREA: the pixel-area relation - output pixel i is the mean of the source span [i h / oh, (i + 1) h / oh) weighted by
 *     fractional coverage, separably per axis, enlarging or shrinking.  Source coordinates come from integers.  oh == h and ow == w: a copy.
 *   add_gaussian_noise: out = x + sigma[i] z, z = the dove_randn stream (seed, stream_id) at the row-major index of
 *     (frame0 + i, y, x, c) in [.][h][w][3] - gray: of (frame0 + i, y, x) in [.][h][w], one draw for the pixel's three channels.
 *   add_poisson_noise: per frame v = clip(rint(x), 0, 255) (gray: of 0.299 R + 0.587 G + 0.114 B in fp32, one value per pixel),
 *     U = 2^ceil(log2(number of distinct v in the frame)), out = x + scale[i] (Poisson(v U) / U - v).  The sampler is exact (inversion below
 *     rate 10, Hoermann's PTRS from there on, fp64); round r of element e (indexed as for the Gaussian noise) draws its two uniforms from the
 *     Philox block with counter (e low, e high, stream_id, r), so stream_id < 2^32.  ws: device scratch of
 *     dove_poisson_noise_workspace_bytes(n) bytes.
 *   jpeg_roundtrip: -> out [n][h][w][3] u8, what baseline JPEG at quality[i] (1..100) does to trunc(clip(x, 0, 255)): JFIF YCbCr, edge
 *     replication to whole 16 x 16 MCUs, 4:2:0 chroma (2x2 mean), 8x8 DCT, Annex-K tables under libjpeg's quality rule, dequantisation, IDCT, "fancy"
 *     3:1 chroma upsampling, RGB.  Integer fixed point throughout: tests/degrade_ref.py fixes every byte.  ws: device scratch of
 *     dove_jpeg_roundtrip_workspace_bytes(n, h, w) bytes. */
#define DOVE_RESIZE_BILINEAR 0
#define DOVE_RESIZE_BICUBIC 1
#define DOVE_RESIZE_AREA 2
int dove_blur2d_f32(const float* x, int n, int h, int w, const float* kernel, int k, int per_frame, float* out, void* stream);
int dove_resize_f32(const float* x, int n, int h, int w, int oh, int ow, int mode, float* out, void* stream);
int dove_add_gaussian_noise_f32(const float* x, int n, int h, int w, const float* sigma, int gray, unsigned long long seed,
                                unsigned long long stream_id, long long frame0, float* out, void* stream);
size_t dove_poisson_noise_workspace_bytes(int n);
int dove_add_poisson_noise_f32(const float* x, int n, int h, int w, const float* scale, int gray, unsigned long long seed,
                               unsigned long long stream_id, long long frame0, void* ws, size_t ws_bytes, float* out, void* stream);
size_t dove_jpeg_roundtrip_workspace_bytes(int n, int h, int w);
int dove_jpeg_roundtrip(const float* x, int n, int h, int w, const int* quality, void* ws, size_t ws_bytes, unsigned char* out,
                        void* stream);

/* The video-compression step of the degradation pipeline (tests/vcodec_ref.py fixes every byte): what a hybrid
 * motion-compensated transform codec does to the pixels, without a bitstream.  Not modelled: sub-pel motion, B frames, intra macroblocks in
 * P frames, the deblocking filter, entropy coding.
 *   vcodec_roundtrip: x [n][h][w][3] f32 on the 0..255 scale -> out [n][h][w][3] u8.  trunc(clip(x, 0, 255)), edge replication to whole
 *     16 x 16 macroblocks, BT.601 limited-range Y'CbCr 4:2:0 (dove_rgb_to_yuv_u8; back with centre siting).  Closed groups of gop frames
 *     (the last may be shorter): an I frame predicted as 128, then P frames predicted from the previous reconstructed frame by full-search
 *     integer motion (range 7, cost SAD + 4 (se_len(dx) + se_len(dy))) per macroblock, chroma at half the vector.  H.264 4x4 core transform
 *     and quantiser at one QP (0..51) per group, found per group by bisection against bitrate * frames under the integer bit-count model of
 *     the definition.  bitrate: bits per frame.  qp_out [ceil(n / gop)] i32 and bits_out [ceil(n / gop)] i64: device memory, the chosen QP
 *     and the bits of each group at it; either may be null.  The QP search runs on the device: no readback, no allocation; ws is device
 *     scratch of dove_vcodec_workspace_bytes(n, h, w, gop) bytes, 256-byte aligned.
 *   motion_search_u8: the motion search on its own.  cur, ref: [n][h][w] u8 planes, both edge-replicated (cur to whole macroblocks, ref to
 *     wherever a vector points).  Per macroblock of frame i the (dy, dx) in [-search, search]^2 (search 0..15) that minimises
 *     (SAD + lambda (se_len(dx) + se_len(dy)), |dy| + |dx|, dy, dx) in that order, prediction = ref[y + dy][x + dx]; se_len(v) is the
 *     signed Exp-Golomb length.  mv_out [n][ceil(h / 16)][ceil(w / 16)][2] i32 as (dy, dx); sad_out [n][..][..] i32, the winner's SAD. */
size_t dove_vcodec_workspace_bytes(int n, int h, int w, int gop);
int dove_vcodec_roundtrip(const float* x, int n, int h, int w, long long bitrate, int gop, void* ws, size_t ws_bytes, unsigned char* out,
                          int* qp_out, long long* bits_out, void* stream);
int dove_motion_search_u8(const unsigned char* cur, const unsigned char* ref, int n, int h, int w, int search, int lambda, int* mv_out,
                          int* sad_out, void* stream);

/* The round trip with an H.264 tool set (tests/vcodec_tools_ref.py fixes every byte).  tools is a mask of the bits below;
 * 0 gives the bytes, QPs and bits of dove_vcodec_roundtrip, unknown bits are refused.  Every other argument is dove_vcodec_roundtrip's; ws is
 * dove_vcodec_tools_workspace_bytes(n, h, w, gop, tools) bytes (with tools 0 the size of dove_vcodec_workspace_bytes).
 *   INTRA16: I frames are predicted per macroblock from the row above and the column to the left of the frame's unfiltered reconstruction
 *     (luma V / H / DC, chroma DC / H / V by SAD + 4 ue_len(index)), macroblocks in raster order: one launch per anti-diagonal.
 *   QPEL: a P macroblock's integer winner is refined in quarter samples (two steps of 9 candidates); luma by the 6-tap (1, -5, 20, 20, -5, 1)
 *     half samples and their averages, chroma bilinear in eighths; the vector costs its quarter-unit Exp-Golomb lengths.
 *   DEBLOCK: the H.264 edge filter at indexA = indexB = QP on every reconstructed frame before it is output and referenced: all vertical
 *     edges of a plane, then all horizontal ones (frame-wide, not the standard's macroblock interleave).
 * Still not modelled: B frames, intra macroblocks in P frames, Intra 4x4 and the plane mode, the Intra16x16 DC Hadamard, per-macroblock
 * QP, entropy coding. */
#define DOVE_VCODEC_INTRA16 1
#define DOVE_VCODEC_QPEL 2
#define DOVE_VCODEC_DEBLOCK 4
size_t dove_vcodec_tools_workspace_bytes(int n, int h, int w, int gop, int tools);
int dove_vcodec_roundtrip_tools(const float* x, int n, int h, int w, long long bitrate, int gop, int tools, void* ws, size_t ws_bytes,
                                unsigned char* out, int* qp_out, long long* bits_out, void* stream);

/* The stitch of ref :712-720 for one piece: the box `valid` (piece coordinates) of piece [3][f][h][w] is copied to the box of the same size at
 * (out_t0, out_h0, out_w0) of chunk [3][f_chunk][Hs][Ws]; both bf16, contiguous.  One launch, no write counts; 16-byte loads and stores when
 * both boxes allow (the box width, every row / frame / channel stride of both arrays and both box origins multiples of 8 elements, i.e.
 * 16-byte aligned), 2-byte otherwise.  Nothing outside the box is
 * written: the chunk buffer needs no clearing when dove_plan_check_coverage has accepted the boxes. */
int dove_stitch(const void* piece, int f, int h, int w, const int* valid, void* chunk, int f_chunk, int Hs, int Ws, int out_t0, int out_h0,
                int out_w0, void* stream);

/* The streaming whole-video session: what `python -m dove_amd.stream` does, as push / step calls on device buffers.  The host keeps the
 * I/O (the library touches no file); the session plans the chunks and tiles, draws the noise, runs dove_sr_clip per piece and stitches,
 * colour-fixes and converts each chunk's final frames.  Its output is byte-identical to the composition of the operator-level entry points
 * (tests/test_video_graph_gpu.py).  Bound to a single-rank context (a context with a communicator is refused); the context's options
 * (VAE tiling, MXFP8, weight sums, VAE streams) apply as they do to dove_sr_clip.  Not thread-safe; one session per context at a time.
 *   in_format / out_format: DOVE_VIDEO_RGB_U8 = frames [n][H][W][3] u8; DOVE_VIDEO_YUV = Y4M frame payloads of in_yuv / out_yuv
 *     (dove_yuv_frame_bytes each; in_yuv carries the inverse matrix, out_yuv the forward one).
 *   upscale: bilinear, dove_preprocess_u8.  color_fix: 0, DOVE_COLORFIX_WAVELET or DOVE_COLORFIX_ADAIN against the upscaled input.
 *   text [text_len][text_dim] bf16 on the device, borrowed until close.  timestep, sqrt_alpha, sqrt_one_minus_alpha as dove_sr_clip.
 *   noise_step != 0: the `--noise_step` pre-noising with noise_sqrt_alpha / noise_sqrt_one_minus_alpha (dove_pre_noise).
 *   seed: piece p (counted over the whole video, chunk-major and tile-minor) draws its posterior noise [L][T][h][w] fp32 as
 *     dove_randn(seed, stream 2p, offset 0) and its pre-noise eps [T'][L][h][w] fp32 as stream 2p + 1.
 *   max_frames: chunk_len 0 only (one piece of the whole clip: memory grows with it) - the most frames that will be pushed.
 *   max_push: the most frames one push adds beyond what dove_video_need asked for (0 = 64); sizes the input ring.
 *   aux_fn (may be NULL): called on the host before each piece with the DiT's grid - T' latent frames (after the patch_t pad) of h x w
 *     latents - to fill a dove_dit_aux for that piece (a host that has diffusers' own RoPE tables and timestep projection hands them over, as
 *     the aux argument of dove_sr_clip; the pointers must stay valid until the step's work has run).  NULL: computed inside the library.
 * Memory: the pieces run in the context's arena (dove_workspace_bytes of the largest piece); everything else is ONE device allocation of
 * dove_video_workspace_bytes made at open.  With chunk_len > 0 neither depends on the number of frames pushed.
 *   push: n frames / payloads in device memory, copied on `stream`; frames no later chunk needs are dropped after each step.
 *   need: *frames = input frames still missing before dove_video_step can run (0 = it can), *end_of_input = 1 when only the end of the input
 *     will do (chunk_len 0).  After dove_video_end_of_input both are 0.
 *   step: runs at most ONE temporal chunk on `stream`: yuv_to_rgb (YUV input) and preprocess; per spatial tile dove_randn, dove_sr_clip and
 *     dove_stitch; dove_color_fix of the chunk's final frames; dove_postprocess_u8 or dove_rgb_to_yuv_u8 with the padding cropped into `out`.
 *     *frames_written (known at once: it follows from the plan) frames of dove_video_info's out_frame_bytes each; *done = 1 after the last
 *     chunk.  out_bytes must hold max_step_frames frames or at least this step's.  A step refused for its arguments, its plan, its
 *     output size or by aux_fn changes nothing and may be repeated; a launch that fails afterwards ends the session (close it).  Fails with
 *     the reference's coverage messages when the plan leaves a hole (a clip of <= overlap_t frames has no chunk at all) or writes a voxel
 *     twice - inside a chunk, or at the seam of two chunks (an odd overlap_t keeps one frame on both sides: "Write count > 1"). */
#define DOVE_VIDEO_RGB_U8 0
#define DOVE_VIDEO_YUV 1
typedef int (*dove_video_aux_fn)(void* user, int T, int h, int w, dove_dit_aux* aux); /* 0 on success */
typedef struct dove_video_params {
  unsigned int struct_size; /* = sizeof(dove_video_params) of the caller's header, as dove_conv_desc */
  unsigned int reserved;    /* 0 */
  int width, height;        /* of the low-resolution input */
  int upscale;
  int chunk_len, overlap_t, tile_h, tile_w, overlap_h, overlap_w;
  int color_fix;
  int in_format, out_format;
  dove_yuv_format in_yuv, out_yuv;
  const void* text;
  int text_len;
  int timestep;
  float sqrt_alpha, sqrt_one_minus_alpha;
  int noise_step;
  float noise_sqrt_alpha, noise_sqrt_one_minus_alpha;
  int max_frames, max_push;
  unsigned long long seed;
  dove_video_aux_fn aux_fn;
  void* aux_user;
} dove_video_params;
typedef struct dove_video dove_video;
size_t dove_video_workspace_bytes(dove_ctx* ctx, const dove_video_params* params); /* 0: bad parameters (dove_last_error) */
int dove_video_open(dove_ctx* ctx, const dove_video_params* params, dove_video** out);
int dove_video_info(const dove_video* v, size_t* in_frame_bytes, size_t* out_frame_bytes, int* out_h, int* out_w, int* max_step_frames);
int dove_video_push(dove_video* v, const void* frames, int n, void* stream);
int dove_video_end_of_input(dove_video* v);
int dove_video_need(const dove_video* v, long long* frames, int* end_of_input);
int dove_video_step(dove_video* v, void* out, size_t out_bytes, int* frames_written, int* done, void* stream);
void dove_video_close(dove_video* v);

/* Optical flow (RAFT) and the warping error (csrc/flow.hip, the convs in csrc/conv_f32.hip).  Everything is fp32 on the f32-input MFMA or the fp32 / fp64
 * VALU; activations are channels-last [n][h][w][c] fp32 whose pixel stride (ldx, ldo, ld...) may exceed c, so an operator reads or fills a
 * channel slice of a wider buffer (pass the pointer of the slice's first channel).  Nothing outside a written slice is touched.  No call
 * uses atomics: two calls give identical bits, and the result for one image does not depend on what else is in the batch.
 *   conv2d_f32: zero padding k / 2, kh, kw in {1, 3, 5, 7}, stride 1 or 2; w is [kh][kw][cin][cout] fp32 (tap-major K, cout contiguous).
 *     out = out_mul * act(scale * (conv + bias) + shift); bias, scale / shift (per output channel) may be NULL.  Each output is one fp32 FMA
 *     chain in K order.  sigmoid and tanh are evaluated in fp64 and rounded once.
 *   instance_norm_f32: per (n, c) over h x w, biased variance, no affine: y = (x - mean) / sqrt(var + eps); relu != 0: y = max(y, 0);
 *     resid != NULL: y = max(resid + y, 0).  x, resid, out dense [n][h][w][c]; out may alias x.  Statistics in fp64 (256-pixel partials merged in
 *     order).  ws: device scratch of dove_instance_norm_f32_workspace_bytes.
 *   corr_volume_f32: out [n][h w][h w] = scale * sum_c fmap1[n][p][c] fmap2[n][q][c] (p the row), fmaps dense [n][h][w][c].
 *   avgpool2_f32: x [planes][h][w] -> out [planes][h / 2][w / 2], 2 x 2 means, odd sizes floored.
 *   corr_lookup_f32: levels l = 0..3 are [n h w][h >> l][w >> l] (the volume and its three pools).  For pixel p with centre (cx, cy) = coords[p ldc],
 *     coords[p ldc + 1] (add_grid != 0: plus the pixel's own (x, y)), out[p][l 81 + a 9 + b] is the bilinear sample (zeros outside, corners
 *     aligned) of plane p of level l at (cx / 2^l + a - 4, cy / 2^l + b - 4): the window's first index moves x, as the reference's CorrBlock does.
 *     out dense [n][h][w][324]; h, w >= 8.
 *   gru_gate_f32: rhx[p][c] = c < ch_h ? r[p][c] * hx[p][c] : hx[p][c] for c < ch (hx, rhx of pixel stride ld; r of ldr).
 *   gru_update_f32: hx[p][c] = (1 - z) hx[p][c] + z q for c < ch_h.
 *   add_f32: out = a + b over ch channels of npix pixels, relu != 0: max(., 0).  out may alias a or b.
 *   convex_upsample_f32: flow [n][h][w] pixels of stride ldf (x, y first), mask dense [n][h][w][576] with channel = tap 64 + i 8 + j ->
 *     out [n][2][8 h][8 w]: out[c][8 y + i][8 x + j] = sum_tap softmax_tap(mask) 8 flow[c] at the 3 x 3 neighbour `tap` (zero outside).
 *   flow_warp_error: n frame pairs.  img1, img2 [n][h][w][3] (DOVE_U8: value / 255; DOVE_F32: as is), flow_fw, flow_bw [n][2][h][w] fp32 (x, y).
 *     With s = (x, y) + flow_fw: b~ = bilinear(flow_bw, s), warp = bilinear(img2, s) (zeros outside, corners aligned);
 *     fb = |flow_fw + b~|^2 < 0.01 (|flow_fw|^2 + |b~|^2) + 0.5; inside = s within [0, w - 1] x [0, h - 1].
 *     out[n][2] fp64 = {sum over pixels with fb and inside of sum_c (img1 - warp)^2, the number of such pixels}.  warped (may be NULL):
 *     [n][h][w][3] fp32; mask (may be NULL): [n][h][w] u8, bit 0 = fb, bit 1 = inside.  ws: dove_flow_warp_error_workspace_bytes. */
#define DOVE_ACT_NONE 0
#define DOVE_ACT_RELU 1
#define DOVE_ACT_SIGMOID 2
#define DOVE_ACT_TANH 3
typedef struct dove_conv2d_f32_args {
  unsigned int struct_size; /* = sizeof(dove_conv2d_f32_args) of the caller's header, as dove_conv_desc */
  unsigned int reserved;    /* 0 */
  const float* x;           /* [n][h][w_in] pixels of stride ldx, cin channels read */
  const float* w;           /* [kh][kw][cin][cout] */
  const float* bias;        /* [cout] or NULL */
  const float* scale;       /* [cout] or NULL; with shift */
  const float* shift;
  float* out;               /* [n][ho][wo] pixels of stride ldo, cout channels written; ho = (h + 2 (kh / 2) - kh) / stride + 1 */
  int n, h, w_in, cin, cout, kh, kw, stride;
  int act;                  /* DOVE_ACT_* */
  float out_mul;            /* 1 for none */
  long long ldx, ldo;
} dove_conv2d_f32_args;
int dove_conv2d_f32(const dove_conv2d_f32_args* args, void* stream);
size_t dove_instance_norm_f32_workspace_bytes(int n, int h, int w, int c);
int dove_instance_norm_f32(const float* x, int n, int h, int w, int c, const float* resid, int relu, float eps, void* ws, size_t ws_bytes,
                           float* out, void* stream);
int dove_corr_volume_f32(const float* fmap1, const float* fmap2, int n, int h, int w, int c, float scale, float* out, void* stream);
int dove_avgpool2_f32(const float* x, long long planes, int h, int w, float* out, void* stream);
int dove_corr_lookup_f32(const float* level0, const float* level1, const float* level2, const float* level3, const float* coords,
                         long long ldc, int add_grid, int n, int h, int w, float* out, void* stream);
int dove_gru_gate_f32(const float* r, long long ldr, const float* hx, long long ld, int ch_h, int ch, long long npix, float* rhx,
                      void* stream);
int dove_gru_update_f32(const float* z, long long ldz, const float* q, long long ldq, float* hx, long long ld, int ch_h, long long npix,
                        void* stream);
int dove_add_f32(const float* a, long long lda, const float* b, long long ldb, float* out, long long ldo, int ch, long long npix, int relu,
                 void* stream);
int dove_convex_upsample_f32(const float* flow, long long ldf, const float* mask, int n, int h, int w, float* out, void* stream);
size_t dove_flow_warp_error_workspace_bytes(int n, int h, int w);
int dove_flow_warp_error(const void* img1, const void* img2, int dtype, const float* flow_fw, const float* flow_bw, int n, int h, int w,
                         void* ws, size_t ws_bytes, double* out, float* warped, unsigned char* mask, void* stream);

/* Perceptual metrics LPIPS and DISTS (csrc/percep.hip, the conv in csrc/conv_f32.hip): the operators of a VGG16 / AlexNet trunk in exact fp32 and the two
 * statistical heads in fp64.  Layouts and guarantees are those of the flow block: channels-last fp32 with pixel strides, no atomics, identical
 * bits on repetition, and an image's result independent of the rest of the batch.
 *   convnet_conv_f32: out = conv + bias, then max(., 0) if relu != 0.  kh, kw in 1..11, stride 1..4, pad_h < kh, pad_w < kw (zero padding),
 *     ho = (h + 2 pad_h - kh) / stride + 1 >= 1; w is [kh][kw][cin][cout] fp32.  Each output is one fp32 FMA chain in K order (tap-major, then
 *     channel), so on a shape dove_conv2d_f32 accepts the two give the same bits.  Two walks, chosen from the arguments alone and named by
 *     dove_convnet_conv_f32_kernel_name ("" for arguments the call would refuse; needs no device): "convnet3x3_f32_kernel" for 3 x 3, stride 1,
 *     pad 1, cin % 32 == 0, cout >= 128, cout % 4 == 0, ldx % 4 == 0 and 16-byte aligned x and w (a 128 x 128 tile, LDS double-buffered); "conv_f32_kernel"
 *     (the flow block's kernel) otherwise.
 *   percep_prep_f32: in is a strided view of n images of c in {1, 3} channels (DOVE_U8: value / 255; DOVE_F32: as is) -> out dense
 *     [n][h][w][3] = (fma(pre_mul, v, pre_add) - mean[ch]) / std[ch]; a one-channel image feeds all three.  mean, std: host arrays of 3.
 *   maxpool_f32: k x k window (1..4), stride s (1..4), no padding, ho = (h - k) / s + 1.  A NaN in a window is its result.
 *   l2pool_f32: out = sqrt(sum_taps g x^2 + 1e-12) with g the 3 x 3 outer product of (1/4, 1/2, 1/4), stride 2, zero padding 1,
 *     ho = (h - 1) / 2 + 1; summed in fp64, rounded once.
 *   lpips_layer: x, y [n][h][w] pixels of stride ld, c channels.  Per pixel in fp64: nx = sqrt(sum_c x^2), ny likewise,
 *     d = sum_c lin[c] (x / (nx + 1e-10) - y / (ny + 1e-10))^2; out[n] (fp64) += (sum over pixels of d) / (h w), one fp64 division.  Partials of 128 pixels, summed in a
 *     fixed tree by a second launch.  ws: dove_lpips_layer_workspace_bytes.
 *   dists_layer: per (n, c) in fp64 the means mx, my, the biased variances vx, vy and the covariance (1024-pixel two-pass partials merged in
 *     slice order), then out[n] (fp64) += sum_c alpha[c] (2 mx my + 1e-6) / (mx^2 + my^2 + 1e-6) + beta[c] (2 cov + 1e-6) / (vx + vy + 1e-6).
 *     alpha, beta: fp64 [c], already divided by the sum of all of them.  ws: dove_dists_layer_workspace_bytes.
 *   The workspace sizes are 0 for an empty batch. */
typedef struct dove_convnet_conv_f32_args {
  unsigned int struct_size; /* = sizeof(dove_convnet_conv_f32_args) of the caller's header, as dove_conv_desc */
  unsigned int reserved;    /* 0 */
  const float* x;           /* [n][h][w_in] pixels of stride ldx, cin channels read */
  const float* w;           /* [kh][kw][cin][cout] */
  const float* bias;        /* [cout] or NULL */
  float* out;               /* [n][ho][wo] pixels of stride ldo, cout channels written */
  int n, h, w_in, cin, cout, kh, kw, stride, pad_h, pad_w;
  int relu;
  int reserved2;            /* 0 */
  long long ldx, ldo;
} dove_convnet_conv_f32_args;
int dove_convnet_conv_f32(const dove_convnet_conv_f32_args* args, void* stream);
const char* dove_convnet_conv_f32_kernel_name(const dove_convnet_conv_f32_args* args);
int dove_percep_prep_f32(const dove_image_view* in, int n, int c, int h, int w, float pre_mul, float pre_add, const float* mean,
                         const float* std, float* out, void* stream);
int dove_maxpool_f32(const float* x, long long ldx, int n, int h, int w, int c, int k, int stride, float* out, long long ldo, void* stream);
int dove_l2pool_f32(const float* x, long long ldx, int n, int h, int w, int c, float* out, long long ldo, void* stream);
size_t dove_lpips_layer_workspace_bytes(int n, int h, int w);
int dove_lpips_layer(const float* x, const float* y, long long ld, const float* lin, int n, int h, int w, int c, void* ws, size_t ws_bytes,
                     double* out, void* stream);
size_t dove_dists_layer_workspace_bytes(int n, int h, int w, int c);
int dove_dists_layer(const float* x, const float* y, long long ld, const double* alpha, const double* beta, int n, int h, int w, int c, void* ws,
                     size_t ws_bytes, double* out, void* stream);

/* NIQE, the no-reference metric of the evaluation step (csrc/niqe.hip): pyiqa's 'niqe' with its defaults, all in fp64.
 *   niqe_features: img is a strided view of n images of c in {1, 3} channels, h, w >= 96 (DOVE_U8: value / 255; DOVE_F32 / DOVE_BF16: values in
 *     [0,1]).  The luma round(255 (0.299 R + 0.587 G + 0.114 B)) (round(255 v) for one channel) of the top-left (h/96)*96 x (w/96)*96 region is
 *     cut into B = (h/96) (w/96) blocks, row-major.  features [n][B][36]: the 18 AGGD features of each 96 x 96 block, then the 18 of the
 *     matching 48 x 48 block of the half-scale image; a product with an empty sign set has NaN features.  sharpness [n][B] (may be NULL): the
 *     block's mean local deviation at scale 1.  ws: device scratch of dove_niqe_workspace_bytes(n, h, w) bytes (0 for an empty batch or
 *     h, w < 96).  The first call on a device builds the Gamma tables on the host and uploads them (a blocking copy).
 *   niqe_stats: features [n][blocks][36] -> mu [n][36], the mean of each column over its non-NaN entries (NaN for none); cov [n][36][36], the
 *     covariance (divisor count - 1) over the blocks without a NaN (NaN for fewer than two); counts [n][2] (int) = {blocks without a NaN, blocks
 *     with at least one non-NaN feature}.
 *   niqe_distance: HOST code on HOST pointers, no device needed.  out = sqrt(d pinv((cov_a + cov_b) / 2) d^T), d = mu_a - mu_b, by a symmetric
 *     Jacobi eigen-solve; pinv drops singular values at or below 36 eps sigma_max.  A non-finite input gives NaN, not an error.
 *   No atomics: two calls give identical bits, and a frame's result does not depend on the rest of the batch. */
size_t dove_niqe_workspace_bytes(int n, int h, int w);
int dove_niqe_features(const dove_image_view* img, int n, int c, int h, int w, void* ws, size_t ws_bytes, double* features, double* sharpness,
                       void* stream);
int dove_niqe_stats(const double* features, int n, int blocks, double* mu, double* cov, int* counts, void* stream);
int dove_niqe_distance(const double* mu_a, const double* cov_a, const double* mu_b, const double* cov_b, double* out);

/* CLIP-IQA (csrc/clipiqa.hip, the conv in csrc/conv_f32.hip): the operators of CLIP RN50's ModifiedResNet in exact fp32, its attention pool and the
 * prompt-pair score in fp64.  Layouts and guarantees are those of the perceptual block: channels-last fp32 with pixel strides, weights
 * [k][k][cin][cout] (BatchNorm folded in by the host), no atomics, identical bits on repetition, an image's result independent of the batch.
 *   resnet_conv_f32: out = relu?((conv + bias) + residual).  k in {1, 3} with zero padding k / 2, stride in {1, 2}; pool in {1, 2}: with 2 the
 *     conv reads the 2 x 2 average ((a + b) + (c + d)) * 0.25f of its input (floor sizes; a, b the upper pixels), so ho = h / 2.  Each output
 *     is one fp32 FMA chain in K order (tap-major, then channel): the bits are dove_convnet_conv_f32's.  Four walks, chosen from the arguments
 *     alone and named by dove_resnet_conv_f32_kernel_name ("" for arguments the call would refuse; needs no device):
 *       "pointwise_f32_kernel": k 1, stride 1, cin % 32 == 0, cout % 4 == 0, ldx % 4 == 0, 16-byte aligned x and w (a 128 x 128 tile, 128 x 64
 *         for cout < 128, LDS double-buffered).  The only walk with pool 2 and with a residual: both are refused on any other.
 *       "convnet3x3_n64_f32_kernel": k 3, stride 1, cout in {32, 64} and the same alignment (a 128 x 64 tile).
 *       "convnet3x3_f32_kernel": k 3, stride 1, cout >= 128 and the same alignment (the perceptual block's kernel).
 *       "conv_f32_kernel" (the flow block's kernel): everything else, among it a k 1 conv with cin % 32 != 0.
 *     residual may be out (each element is read, then written, by one thread).
 *   avgpool_cl_f32: the 2 x 2, stride 2 average in the same summation order, ho = h / 2, wo = w / 2 (h, w >= 2).
 *   clip_attnpool_f32: x [n][h][w] pixels of stride ldx, 2048 channels -> out [n][1024] fp32, CLIP's AttentionPool2d without the positional
 *     embedding: tokens T = [mean over the h w positions; the positions], 32 heads of 64, only token 0 as the query.  wq, wk, wv [2048][2048]
 *     and wc [1024][2048] are the projections' weights as torch holds them ([out][in]), bq, bk, bv [2048], bc [1024].  Evaluated in fp64 as
 *     q = Wq T_0 + bq, s_t,h = (T_t . (Wk_h^T q_h) + q_h . bk_h) / 8, a = softmax over t, o_h = Wv_h (sum_t a_t,h T_t) + bv_h, out = Wc o + bc
 *     (standard attention in another rounding order), rounded once to fp32.  Token sums go through slices of 256 tokens merged in order.
 *     ws: dove_clip_attnpool_workspace_bytes (0 for an empty batch).
 *   clipiqa_score: emb [n][dim] fp32, text [2 pairs][dim] fp64, already L2-normalised, rows (positive, negative) per pair.  In fp64:
 *     f = emb / |emb|, l_j = logit_scale f . text_j, out[n] = mean over the pairs of 1 / (1 + exp(l_neg - l_pos)). */
typedef struct dove_resnet_conv_f32_args {
  unsigned int struct_size; /* = sizeof(dove_resnet_conv_f32_args) of the caller's header, as dove_conv_desc */
  unsigned int reserved;    /* 0 */
  const float* x;           /* [n][h][w_in] pixels of stride ldx, cin channels read */
  const float* w;           /* [k][k][cin][cout] */
  const float* bias;        /* [cout] or NULL */
  const float* residual;    /* [n][ho][wo] pixels of stride ldr, cout channels, or NULL */
  float* out;               /* [n][ho][wo] pixels of stride ldo, cout channels written */
  int n, h, w_in, cin, cout, k, stride, pool;
  int relu;
  int reserved2;            /* 0 */
  long long ldx, ldr, ldo;
} dove_resnet_conv_f32_args;
int dove_resnet_conv_f32(const dove_resnet_conv_f32_args* args, void* stream);
const char* dove_resnet_conv_f32_kernel_name(const dove_resnet_conv_f32_args* args);
int dove_avgpool_cl_f32(const float* x, long long ldx, int n, int h, int w, int c, float* out, long long ldo, void* stream);
size_t dove_clip_attnpool_workspace_bytes(int n, int h, int w);
int dove_clip_attnpool_f32(const float* x, long long ldx, int n, int h, int w, const float* wq, const float* bq, const float* wk,
                           const float* bk, const float* wv, const float* bv, const float* wc, const float* bc, void* ws, size_t ws_bytes,
                           float* out, void* stream);
int dove_clipiqa_score(const float* emb, const double* text, int n, int pairs, int dim, double logit_scale, double* out, void* stream);

/* MUSIQ (csrc/musiq.hip): what pyiqa's `musiq` needs beside the convs and GEMMs above (its 1 x 1 convs and Linears run on
 * dove_resnet_conv_f32 with tokens as pixels, its 3 x 3 conv too, its 7 x 7 stem conv on dove_convnet_conv_f32 with pad 0 over the 37 x 37 frame
 * that the gather writes).  Channels-last fp32, no atomics, identical bits on repetition, a frame's result independent of the batch.  None of
 * these needs a workspace.
 *   musiq_patches_f32: img is n frames [c][h][w] (c in {1, 3}; one channel is repeated; f32 / bf16 in [0,1] or u8 read as u / 255.0 in fp64, any
 *     strides) -> out [n tokens_per_frame][side][side][3].  tokens [tokens_per_frame][4] int32 on the device: (scale 0..2, patch row, patch
 *     column, spatial index); scales[3] on the host.  Token t's 32 x 32 patch lies at [before, before + 32)^2 of its side x side frame, 0
 *     around it.  Patch pixel (py, px) is pixel (32 row + py - pad_top, 32 column + px - pad_left) of the scale's rh x rw image and 0 outside
 *     it.  With v' = 2 v - 1: a scale with resized == 0 (rh == h, rw == w) gives (float)v'; a resized scale gives torch's bicubic of v'
 *     (A = -0.75, align_corners = False, source coordinate (h / rh) (y + 0.5) - 0.5, taps clamped at the border, no antialias), evaluated in
 *     fp64 from the source values, rows first, taps ascending, and rounded once to fp32.
 *   musiq_groupnorm_f32: x [maps][side][side][c] dense, 32 groups of c / 32 channels, statistics per map and group in fp64 in two passes (mean,
 *     then squared deviations; eight threads per group in a fixed order), biased variance.  out = relu?((x - mean) rstd gamma + beta [+ the same
 *     of y with gamma_y, beta_y]), the bracket evaluated in fp64 and rounded once.  pool != 0 (one operand only): out is [maps][side / 2]
 *     [side / 2][c], the 3 x 3 stride-2 max over those values with zero padding 0 before and 1 after.  out may be x when pool == 0.
 *   layernorm_f32: rows of dim values at stride ldx -> stride ldo: fp64 mean and biased variance in two passes, fixed order, one rounding.
 *   musiq_embed_f32: out [n][tokens_per_frame + 1][dim]: row 0 = cls, row 1 + t = (emb[f tokens_per_frame + t] + pos[spatial(t)]) +
 *     scale_emb[scale(t)], fp32.
 *   mha_f32: q, k, v: rows of stride ld, n frames of t rows each, head h in columns [64 h, 64 h + 64) (they may be slices of one QKV buffer);
 *     out the same with stride ldo.  softmax(scale q k^T) v per frame and head in fp32 on v_mfma_f32_32x32x2_f32, flash-style: Q tiles of 64
 *     rows, KV tiles of 32 keys (dove_mha_f32_tiles reports them), a running row maximum, row sums in a fixed order, accurate expf; no t x t
 *     matrix is stored.  Any t >= 1; ld, ldo multiples of 4 and 16-byte aligned pointers.
 *   gelu_f32: out = 0.5 x (1 + erff(x / sqrt 2)) in fp32, its own pass; out may be x.
 *   musiq_score: features n rows of dim at stride ld (the normalised token 0), w [k][dim], b [k] fp32 -> out[n] fp64: row = w f + b in fp64;
 *     k == 1: the row; k > 1 (the AVA head): sum_j (j + 1) softmax(row)_j.  k <= 64. */
typedef struct dove_musiq_scale {
  int rh, rw;            /* the scale's image */
  int pad_top, pad_left; /* zero padding in front of it: (32 ceil(rh / 32) - rh) / 2, likewise for rw */
  int resized;           /* 0: the original resolution, read as it is */
  int reserved;          /* 0 */
} dove_musiq_scale;
int dove_musiq_patches_f32(const dove_image_view* img, int n, int c, int h, int w, const dove_musiq_scale* scales, const int* tokens,
                           int tokens_per_frame, int before, int side, float* out, void* stream);
int dove_musiq_groupnorm_f32(const float* x, const float* gamma, const float* beta, const float* y, const float* gamma_y, const float* beta_y,
                             long long maps, int side, int c, double eps, int relu, int pool, float* out, void* stream);
int dove_layernorm_f32(const float* x, long long ldx, long long rows, int dim, const float* gamma, const float* beta, double eps, float* out,
                       long long ldo, void* stream);
int dove_musiq_embed_f32(const float* emb, const float* pos, const float* scale_emb, const float* cls, const int* tokens, int n,
                         int tokens_per_frame, int dim, float* out, void* stream);
int dove_mha_f32(const float* q, const float* k, const float* v, long long ld, int n, int t, int heads, float scale, float* out, long long ldo,
                 void* stream);
void dove_mha_f32_tiles(int* q_tile, int* kv_tile);
int dove_gelu_f32(const float* x, long long count, float* out, void* stream);
int dove_musiq_score(const float* features, long long ld, const float* w, const float* b, int n, int dim, int k, double* out, void* stream);

/* FasterVQA / FAST-VQA (csrc/swin3d.hip; tests/fastvqa_ref.py is the definition): what a Video Swin-T with gated relative
 * position bias needs beside dove_resnet_conv_f32's 1 x 1 walk (every Linear, tokens as pixels), dove_layernorm_f32 and dove_gelu_f32.  Token
 * maps are channels-last fp32 [b][d][h][w][c], dense; no atomics, identical bits on repetition, a sample's result independent of the batch.
 * None of these needs a workspace.
 *   vqa_fragments_f32: clip is frames_in frames [3][h][w] (f32 / bf16 in [0,1], or u8; any strides).  frames [t] int32 and offsets [gh][gw]
 *     [t_groups][2] int32 (row, column: the top-left source pixel of a fragment) are on the device; mean[3], std[3] on the host.  Output pixel
 *     (t, y, x) of the [t][gh fh][gw fw] canvas is pixel offsets[y / fh][x / fw][t / (t / t_groups)] + (y % fh, x % fw) of frame frames[t]; a
 *     coordinate or frame index outside the clip is clamped into it.  Value (X - mean_c) / std_c evaluated in fp64 and rounded once, with X the u8
 *     value itself, or 255.0 v otherwise.  cols == 0: out is the canvas [t][gh fh][gw fw][3].  cols != 0 (t even, canvas sides multiples of 4): out
 *     is [t / 2][gh fh / 4][gw fw / 4][96], the rows of the (2, 4, 4) stride-(2, 4, 4) patch embedding's GEMM, column c 32 + (t % 2) 16 + (y % 4) 4
 *     + x % 4 (a Conv3d weight [out][3][2][4][4] flattened); the embedding is then one k-ordered fp32 FMA chain of 96 terms per output.
 *   swin3d_window_gather_f32: x [b][dims] [c] -> out [b nW][N][c], N = window[0] window[1] window[2], nW the window count of the map padded to
 *     multiples of the window.  Slot n of window a is padded position p = a window + n per axis (both row-major over d, h, w) and holds map
 *     position (p + shift) % padded, torch.roll by -shift, or 0 where that is in the pad.  0 <= shift < window; c a multiple of 4.  The caller
 *     applies Video Swin's rule that an axis no longer than its window uses its own length as the window and shift 0.
 *   swin3d_window_scatter_f32: the inverse on the unpadded map, out = shortcut + windows; out may be shortcut.
 *   swin3d_patch_merge_f32: x [maps][h][w][c] -> out [maps][ceil(h / 2)][ceil(w / 2)][4 c]: chunk j of an output pixel is input pixel (2 h2 +
 *     (j & 1), 2 w2 + (j >> 1)), Swin's order (0,0), (1,0), (0,1), (1,1), or 0 outside the map.
 *   swin3d_window_attention_f32: q, k, v: rows of stride ld, `windows` windows of n rows each, head h in columns [32 h, 32 h + 32) (slices of
 *     one QKV buffer); out likewise with stride ldo.  Per window and head, in fp32 on v_mfma_f32_32x32x2_f32 with K and V of the window in LDS:
 *     s = (q . k) scale + T[index[query][key]][h] + (region[query] != region[key] ? -100 : 0), out = softmax(s) v.  index [n][n] int32 into
 *     tables of [table_rows][heads] (an entry outside [0, table_rows) is clamped); T = table_b where it is given and frag[query] != frag[key], else
 *     table_a.  frag and region are [id_windows][n] int32 and window a uses row a % id_windows (id_windows: the windows of one sample); either
 *     may be NULL (no gate / no mask).  The softmax is two-pass: the true row maximum over all keys first, then expf(s - max) (accurate expf), row
 *     sums in key order, no n x n matrix stored.  1 <= n <= 392 (dove_swin3d_attention_tiles reports the 32 x 32 tile and this limit); ld, ldo
 *     multiples of 4 and 16-byte aligned pointers.  The head's column of each table is kept in LDS beside K and V: 260 bytes per 32 tokens
 *     (rounded up) of n plus 4 bytes per table row must fit 160 KiB (n = 392 with two tables of 2535 rows needs 129 KiB).
 *   vqa_head_f64: features [clips][tokens] rows of dim at stride ld; w1 [hidden][dim], b1 [hidden], w2 [hidden], b2 [1] fp32 -> out[clips] fp64:
 *     the mean over a clip's tokens of w2 . gelu(w1 f + b1) + b2 in fp64 (exact erf), every sum in a fixed order.  hidden <= 256. */
int dove_vqa_fragments_f32(const dove_image_view* clip, int frames_in, int h, int w, const int* frames, int t, const int* offsets, int gh, int gw,
                           int fh, int fw, int t_groups, const double* mean, const double* std, int cols, float* out, void* stream);
int dove_swin3d_window_gather_f32(const float* x, int b, const int* dims, int c, const int* window, const int* shift, float* out, void* stream);
int dove_swin3d_window_scatter_f32(const float* windows, const float* shortcut, int b, const int* dims, int c, const int* window,
                                   const int* shift, float* out, void* stream);
int dove_swin3d_patch_merge_f32(const float* x, long long maps, int h, int w, int c, float* out, void* stream);
void dove_swin3d_attention_tiles(int* q_tile, int* kv_tile, int* max_n);
int dove_swin3d_window_attention_f32(const float* q, const float* k, const float* v, long long ld, long long windows, int n, int heads,
                                     float scale, const float* table_a, const float* table_b, int table_rows, const int* index, const int* frag,
                                     const int* region, int id_windows, float* out, long long ldo, void* stream);
int dove_vqa_head_f64(const float* features, long long ld, int clips, int tokens, int dim, const float* w1, const float* b1, int hidden,
                      const float* w2, const float* b2, double* out, void* stream);

/* DOVER's aesthetic branch (csrc/convnext3d.hip; tests/dover_ref.py is the definition): what an inflated ConvNeXt-Tiny needs
 * beside the operators above.  Maps are channels-last fp32 [b][d][h][w][c], dense; no atomics, identical bits on repetition, a sample's result
 * independent of the batch.  Neither needs a workspace.
 *   dwconv3d_f32: depthwise Conv3d, kernel (3,7,7), zero padding (1,3,3), stride 1.  weight is [3][7][7][c] (tap-major), bias [c]; c a multiple
 *     of 4; out must not overlap x; 16-byte aligned pointers.  Exact fp32: out = one fmaf chain from the bias over the taps in (kd, kh, kw)
 *     order, each ascending, tap (kd, kh, kw) reading x at (d + kd - 1, h + kh - 3, w + kw - 3); taps outside the map are skipped or multiply
 *     a 0.  dove_dwconv3d_tile reports the th x tw output tile of a workgroup on an h x w map (tw is 7 or 8, th at most 16).
 *   vqa_resized_view_f32: clip as in vqa_fragments_f32.  Output pixel (t, y, x) of the [t][oh][ow] view is frame frames[t] (clamped into the
 *     clip) resampled by two separable tap tables on the device: ytab [oh][2] int32 (first source row, tap count <= ymax) and yw [oh][ymax]
 *     fp64 weights, xtab / xw likewise.  sum_j yw[j] (sum_i xw[i] X[first_y + j][first_x + i]) in fp64 with X the u8 value or 255.0 v, source
 *     coordinates clamped into the frame, then (sum - mean_c) / std_c, rounded once.  cols as in vqa_fragments_f32: [t][oh][ow][3], or the
 *     patch GEMM's rows [t / 2][oh / 4][ow / 4][96] (t even, oh and ow multiples of 4). */
void dove_dwconv3d_tile(int h, int w, int* th, int* tw);
int dove_dwconv3d_f32(const float* x, int b, int d, int h, int w, int c, const float* weight, const float* bias, float* out, void* stream);
int dove_vqa_resized_view_f32(const dove_image_view* clip, int frames_in, int h, int w, const int* frames, int t, const int* ytab, const double* yw,
                              int ymax, const int* xtab, const double* xw, int xmax, int oh, int ow, const double* mean, const double* std,
                              int cols, float* out, void* stream);

/* MANIQA (csrc/maniqa.hip; tests/maniqa_ref.py is the definition): what the ViT-B/8 trunk, the transposed ("channel")
 * attention and the 2-D Swin stages need beside the operators above.  fp32, no atomics, identical bits on repetition, a sample's result
 * independent of the batch.  None needs a workspace.
 *   bmm_f32: per batch i < batch, out_i = alpha (A_i B_i) (+ bias) (+ res_i) on v_mfma_f32_32x32x2_f32.  A_i = a + i sa is [m][k] rows of stride
 *     lda; B_i = b + i sb is [k][n] rows of stride ldb, or with DOVE_BMM_B_TRANSPOSED [n][k] rows of stride ldb (q k^T).  A batch stride of 0
 *     shares the operand.  k and n multiples of 4, m any; lda, ldb, sa, sb multiples of 4; a, b 16-byte aligned.  Every output is one fp32 fmaf
 *     chain over k ascending whatever the shape, the tile and the batch (no split-K, no padded k), then, each step rounded on its own: times
 *     alpha (when alpha != 1), plus bias[column] (bias[row] under DOVE_BMM_BIAS_ROWS), plus the residual.  out_i = out + i so has rows of stride
 *     ldo; DOVE_BMM_STORE_TRANSPOSED stores element (row, column) at out_i[column ldo + row] and reads the residual (stride ldr, batch stride
 *     sr) the same way.  res may be out; out must not overlap a or b.  dove_bmm_f32_tiles reports the 128 x 128 x 32 tile and
 *     dove_bmm_f32_kernel_name the kernel a flag set runs; neither needs a device.
 *   softmax_rows_f32: out[r] = softmax(x[r]) over cols columns (rows of stride ldx / ldo): the true row maximum, the accurate expf, the sum in
 *     a fixed order, e / sum.  out may be x.
 *   window_attention_f32: as swin3d_window_attention_f32 for 2-D windows with wider heads: `windows` windows of n <= 64 rows, head h in columns
 *     [head_dim h, head_dim (h + 1)), head_dim a multiple of 32 up to 192; s = (q . k) scale + table[index[query][key]][h] + (region[query] !=
 *     region[key] ? -100 : 0), out = softmax(s) v with the two-pass softmax.  One table, no fragment gate.  dove_window_attention_tiles
 *     reports the 32-row tile, the longest window and the widest head.  K and V of a window are kept in LDS: 32 ceil(n / 32) (8 head_dim + 8) +
 *     4 table_rows bytes must fit 128 KiB.
 *   maniqa_crops_f32: img as above; crop k of frame f is the side x side square at origins[k] = (row, column) (int32 [crops][2] on the device,
 *     clamped into the frame), (v - 0.5) / 0.5 in fp64 rounded once, written as the rows of the patch embedding's GEMM: out [n crops (side /
 *     patch)^2][3 patch^2], column c patch^2 + (y % patch) patch + x % patch.  One channel is repeated.
 *   maniqa_tokens_f32: out [n][tokens + 1][dim]: row 0 = cls + pos[0], row 1 + t = emb[n tokens + t] + pos[1 + t].
 *   mix_f32: per batch, out = alpha a (+ r) on [rows][cols] matrices (strides lda, ldr, ldo, batch strides sa, sr, so), each step rounded on its
 *     own; transpose != 0 stores out[col ldo + row] (out must then be neither input; otherwise out may be a or r).
 *   maniqa_score: hidden [frames crops positions] rows of 2 hid at stride ld (the score branch's ReLU'd hidden units, then the weight
 *     branch's); per position f = relu(wf . h + bf), w = sigmoid(ww . h' + bw) in fp64; crop_scores[frame crops + crop] = sum f w / sum w (fp64
 *     [frames crops], an output of its own), out[frame] = the mean over its crops, every sum in a fixed order. */
#define DOVE_BMM_B_TRANSPOSED 1
#define DOVE_BMM_STORE_TRANSPOSED 2
#define DOVE_BMM_BIAS_ROWS 4
void dove_bmm_f32_tiles(int* m_tile, int* n_tile, int* k_tile);
const char* dove_bmm_f32_kernel_name(int flags);
int dove_bmm_f32(const float* a, long long lda, long long sa, const float* b, long long ldb, long long sb, const float* bias, const float* res,
                 long long ldr, long long sr, float* out, long long ldo, long long so, int batch, int m, int n, int k, float alpha, int flags,
                 void* stream);
int dove_softmax_rows_f32(const float* x, long long ldx, long long rows, int cols, float* out, long long ldo, void* stream);
void dove_window_attention_tiles(int* tile, int* max_n, int* max_head_dim);
int dove_window_attention_f32(const float* q, const float* k, const float* v, long long ld, long long windows, int n, int heads, int head_dim,
                              float scale, const float* table, int table_rows, const int* index, const int* region, int id_windows, float* out,
                              long long ldo, void* stream);
int dove_maniqa_crops_f32(const dove_image_view* img, int n, int c, int h, int w, const int* origins, int crops, int side, int patch, float* out,
                          void* stream);
int dove_maniqa_tokens_f32(const float* emb, const float* cls, const float* pos, long long n, int tokens, int dim, float* out, void* stream);
int dove_mix_f32(const float* a, long long lda, long long sa, const float* r, long long ldr, long long sr, float alpha, int batch, int rows,
                 int cols, int transpose, float* out, long long ldo, long long so, void* stream);
int dove_maniqa_score(const float* hidden, long long ld, int frames, int crops, int positions, int hid, const float* wf, const float* bf,
                      const float* ww, const float* bw, double* crop_scores, double* out, void* stream);

/* ---- PNG encoder (csrc/png.hip; tests/png_ref.py is the bit-exact definition of the filtered stream) ----
 * png_encode: img is a strided [n,channels,h,w] view as above (channels 3 = RGB, 1 = grey; u8 as it is, f32 / bf16 quantised as
 *   dove_postprocess_u8 does, trunc(clamp(255 x, 0, 255))).  Frame i becomes a complete 8-bit, non-interlaced PNG file at
 *   out + i * dove_png_bound(h, w, channels), sizes[i] bytes long (sizes is on the device): signature, IHDR, IDAT chunks, IEND, every
 *   CRC-32 and the Adler-32 computed on the device.  Each scanline takes the filter (None, Sub, Up, Average, Paeth) with the smallest sum
 *   of |filtered byte read as int8|, ties to the lower id.  The filtered stream is cut into segments of dove_png_segment_rows(w, channels)
 *   whole rows (ceil(32768 / (w channels + 1))); each segment is one literal-only dynamic-Huffman deflate block (code lengths <= 15 bits,
 *   or the flat code - 255 symbols of 8 bits, 2 of 9 - where the built code would cost more payload bits) followed by an empty stored
 *   block, in an IDAT chunk of its own.  No LZ77 matches: a file is never below 1/8 of its raw size.
 *   dove_png_bound = filtered bytes * 9 / 8 + 256 per segment + 64, the most bytes a file can take (0 for a bad shape).
 *   ws: device scratch of dove_png_workspace_bytes(n, h, w, channels) bytes, 8-byte aligned.  Integer arithmetic only: two calls give
 *   identical bytes and a frame's file does not depend on the batch it is encoded in.
 * zlib_huffman: the same deflate stage on nbytes >= 1 plain bytes in segments of segment_bytes (1 KiB .. 1 MiB): out receives one zlib
 *   stream (header 78 01, the segments, a final empty block, Adler-32) of *size bytes (size is on the device), at most
 *   dove_zlib_huffman_bound(nbytes, segment_bytes); ws: dove_zlib_huffman_workspace_bytes(nbytes, segment_bytes) bytes. */
int dove_png_segment_rows(int w, int channels);
size_t dove_png_bound(int h, int w, int channels);
size_t dove_png_workspace_bytes(int n, int h, int w, int channels);
int dove_png_encode(const dove_image_view* img, int n, int h, int w, int channels, void* ws, size_t ws_bytes, unsigned char* out,
                    long long* sizes, void* stream);
size_t dove_zlib_huffman_bound(long long nbytes, long long segment_bytes);
size_t dove_zlib_huffman_workspace_bytes(long long nbytes, long long segment_bytes);
int dove_zlib_huffman(const unsigned char* in, long long nbytes, long long segment_bytes, void* ws, size_t ws_bytes, unsigned char* out,
                      long long* size, void* stream);

/* ---- JPEG encoder (csrc/jpeg.hip; tests/jpeg_ref.py is the byte-exact definition of the file) ----
 * jpeg_encode: img is a strided [n,3,h,w] RGB view as above (u8 as it is, f32 / bf16 quantised as dove_postprocess_u8 does,
 *   trunc(clamp(255 x, 0, 255))).  Frame i becomes a complete baseline JFIF file at out + i * dove_jpeg_bound(h, w, subsampling), sizes[i]
 *   bytes long (sizes is on the device): SOI, APP0 (JFIF 1.01, density 1:1), two DQT, SOF0, the four Annex-K Huffman tables, DRI, SOS,
 *   the entropy-coded data, EOI.  Colour conversion, the 2x2 chroma mean of 4:2:0, the integer DCT and the quantiser under libjpeg's
 *   quality rule are those of dove_jpeg_roundtrip (quality is a HOST array of n entries, 1..100); 4:4:4 skips the chroma mean and pads to
 *   whole 8 x 8 instead of 16 x 16.  AC levels are clamped to -1023..1023 and DC levels to -1024..1023 after the quantiser (never binding
 *   for 8-bit samples).  The scan is cut into restart intervals of dove_jpeg_restart_mcus() MCUs: each resets the DC predictors, is padded
 *   with 1-bits to a byte, has 0x00 after every 0xFF data byte and is followed by RST(m mod 8), the last one by EOI.
 *   dove_jpeg_bound = 629 header bytes + 416 per 8 x 8 block (at most 22 + 63 * 26 = 1660 bits, 208 bytes with padding, doubled by
 *   stuffing) + 2 per interval: a true upper bound, far above real files (0 for a bad shape or subsampling; h, w <= 65535).
 *   ws: device scratch of dove_jpeg_workspace_bytes(n, h, w, subsampling) bytes, 16-byte aligned.  Integer arithmetic only: two calls
 *   give identical bytes and a frame's file does not depend on the batch it is encoded in. */
#define DOVE_JPEG_420 0
#define DOVE_JPEG_444 1
int dove_jpeg_restart_mcus(void);
size_t dove_jpeg_bound(int h, int w, int subsampling);
size_t dove_jpeg_workspace_bytes(int n, int h, int w, int subsampling);
int dove_jpeg_encode(const dove_image_view* img, int n, int h, int w, const int* quality, int subsampling, void* ws, size_t ws_bytes,
                     unsigned char* out, long long* sizes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DOVE_HIP_H */
