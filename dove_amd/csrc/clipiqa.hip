// CLIP-IQA (include/dove_hip.h has the contract): the operators of CLIP RN50's ModifiedResNet in exact fp32, the
// attention-pool head and the prompt-pair score in fp64.  Activations are channels-last fp32 [n][h][w][c] with pixel strides, as in
// percep.hip.  The tower's convolution (dove_resnet_conv_f32, pool-on-load and residual included) is in conv_f32.hip.
//
// avgpool_cl_kernel: one thread per output element, ((a + b) + (c + d)) * 0.25f in the order of pool-on-load.
// Attention pool.  Only token 0 (the mean token) is a query, so K and V are never projected over the tokens.  With T the h w + 1 tokens,
//   q = Wq T_0 + bq, per head u_h = Wk_h^T q_h and c_h = q_h . bk_h give the scores s_t,h = (T_t . u_h + c_h) / 8 = q_h . (Wk_h T_t + bk_h) / 8;
//   after the softmax over t, p_h = sum_t a_t,h T_t and o_h = Wv_h p_h + bv_h = sum_t a_t,h (Wv_h T_t + bv_h) because the a_t,h sum to one;
//   e = Wc o + bc.  This is the mathematics of standard multi-head attention in another rounding order.  Everything behind the fp32 feature
//   map is carried in fp64 (token sums, projections, softmax) and rounded once, into the fp32 embedding; the weights are read as fp32.
//   Sums over tokens go through slices of AP_SLICE tokens, one fp64 partial per (slice, channel), merged in slice order; sums over channels
//   are a fixed butterfly over the wave.  No atomics: an image's embedding does not depend on the batch it runs in.
// clipiqa_score_kernel: one block per image, fp64: f = e / |e|, logits = scale f . t_j, value = mean over pairs of 1 / (1 + exp(l_neg - l_pos)).
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int AP_SLICE = 256;                                       // tokens per attention-pool partial
constexpr int AP_C = 2048, AP_HEADS = 32, AP_HD = 64, AP_OUT = 1024;
constexpr int AP_TOK = 4;                                           // tokens per block of the score kernel
constexpr long long MAX_ELEMS = (long long)NT * 0x7fffffffLL;

inline unsigned blocks_for(long long total) { return (unsigned)((total + NT - 1) / NT); }

// ----------------------------------------------------------------- avgpool -----------------------------------------------------------------
__global__ __launch_bounds__(NT) void avgpool_cl_kernel(const float* __restrict__ x, long long ldx, int h, int w, int c, int ho, int wo,
                                                        long long total, float* __restrict__ out, long long ldo) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % c);
  const long long pix = i / c;
  const int ox = (int)(pix % wo), oy = (int)((pix / wo) % ho);
  const long long n = pix / ((long long)wo * ho);
  const float* s = x + ((n * h + 2 * oy) * w + 2 * ox) * ldx + ch;
  const long long row = (long long)w * ldx;
  out[pix * ldo + ch] = ((s[0] + s[ldx]) + (s[row] + s[row + ldx])) * 0.25f;
}

// ------------------------------------------------------------ attention pool ------------------------------------------------------------
// Workspace of one image, in doubles (ap_ws_doubles): part [S][32][2048] | mean [2048] | q [2048] | u [32][2048] | cst [32] |
// sc [HW + 1][32] | pv [32][2048] | o [2048].  The token-sum partials of the mean use the first S x 2048 doubles of part.
struct ApWs {
  long long part, mean, q, u, cst, sc, pv, o, total;
};

inline ApWs ap_layout(long long HW) {
  const long long S = (HW + AP_SLICE - 1) / AP_SLICE;
  ApWs l;
  l.part = 0;
  l.mean = l.part + S * AP_HEADS * AP_C;
  l.q = l.mean + AP_C;
  l.u = l.q + AP_C;
  l.cst = l.u + (long long)AP_HEADS * AP_C;
  l.sc = l.cst + AP_HEADS;
  l.pv = l.sc + (HW + 1) * AP_HEADS;
  l.o = l.pv + (long long)AP_HEADS * AP_C;
  l.total = l.o + AP_C;
  return l;
}

// grid (S, 2048 / NT, n): the sum of a slice's tokens per channel
__global__ __launch_bounds__(NT) void ap_mean_partial_kernel(const float* __restrict__ x, long long ld, int HW, double* __restrict__ ws,
                                                             ApWs l) {
  const int c = blockIdx.y * NT + threadIdx.x, s = blockIdx.x, n = blockIdx.z;
  const int t0 = s * AP_SLICE, cnt = min(AP_SLICE, HW - t0);
  const float* xp = x + ((long long)n * HW + t0) * ld + c;
  double sum = 0.0;
  for (int i = 0; i < cnt; ++i) sum += (double)xp[(long long)i * ld];
  ws[n * l.total + l.part + (long long)s * AP_C + c] = sum;
}

// grid (2048 / NT, n): the slices in order, then one division
__global__ __launch_bounds__(NT) void ap_mean_merge_kernel(int HW, int S, double* __restrict__ ws, ApWs l) {
  const int c = blockIdx.x * NT + threadIdx.x, n = blockIdx.y;
  double* w = ws + n * l.total;
  double sum = 0.0;
  for (int s = 0; s < S; ++s) sum += w[l.part + (long long)s * AP_C + c];
  w[l.mean + c] = sum / (double)HW;
}

// out[r] = W[r] . vec_g + b[r], g = r / group_rows (one vector for all rows when group_rows == rows); one wave per row.
// grid (rows / 4, n); exactly one of out64 (workspace offset) and out32 is used.
__global__ __launch_bounds__(NT) void ap_matvec_kernel(const float* __restrict__ W, const float* __restrict__ b, int rows, int group_rows,
                                                       double* __restrict__ ws, long long ws_stride, long long vec_off, long long out_off,
                                                       float* __restrict__ out32) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), n = blockIdx.y;
  if (r >= rows) return;                       // a whole wave leaves together
  double* w = ws + n * ws_stride;
  const double* vec = w + vec_off + (long long)(r / group_rows) * AP_C;
  const float* wr = W + (long long)r * AP_C;
  double sum = 0.0;
  for (int c = lane; c < AP_C; c += 64) sum += (double)wr[c] * vec[c];
  sum = wave_sum_f64(sum) + (double)b[r];
  if (lane == 0) {
    if (out32) out32[(long long)n * rows + r] = (float)sum;
    else w[out_off + r] = sum;
  }
}

// grid (2048 / NT, 32, n): u[h][c] = sum_j Wk[64 h + j][c] q[64 h + j] with j ascending; the block of channel 0 also writes c_h = q_h . bk_h
__global__ __launch_bounds__(NT) void ap_u_kernel(const float* __restrict__ Wk, const float* __restrict__ bk, double* __restrict__ ws, ApWs l) {
  const int c = blockIdx.x * NT + threadIdx.x, h = blockIdx.y, n = blockIdx.z;
  double* w = ws + n * l.total;
  const double* q = w + l.q + h * AP_HD;
  const float* wk = Wk + (long long)h * AP_HD * AP_C + c;
  double sum = 0.0;
  for (int j = 0; j < AP_HD; ++j) sum += (double)wk[(long long)j * AP_C] * q[j];
  w[l.u + (long long)h * AP_C + c] = sum;
  if (c == 0) {
    double k = 0.0;
    for (int j = 0; j < AP_HD; ++j) k += q[j] * (double)bk[h * AP_HD + j];
    w[l.cst + h] = k;
  }
}

// grid (ceil((HW + 1) / AP_TOK), n): wave v of a block owns heads 8 v .. 8 v + 7 of AP_TOK tokens; token 0 is the mean
__global__ __launch_bounds__(NT) void ap_scores_kernel(const float* __restrict__ x, long long ld, int HW, double* __restrict__ ws, ApWs l) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y;
  double* w = ws + n * l.total;
  const int t0 = blockIdx.x * AP_TOK;
  double acc[AP_TOK][8];
#pragma unroll
  for (int t = 0; t < AP_TOK; ++t)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[t][k] = 0.0;
  const double* u = w + l.u + (long long)(8 * wave) * AP_C;
  for (int c = lane; c < AP_C; c += 64) {
    double tv[AP_TOK];
#pragma unroll
    for (int t = 0; t < AP_TOK; ++t) {
      const int tok = t0 + t;
      tv[t] = tok == 0 ? w[l.mean + c] : tok <= HW ? (double)x[((long long)n * HW + tok - 1) * ld + c] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double uv = u[(long long)k * AP_C + c];
#pragma unroll
      for (int t = 0; t < AP_TOK; ++t) acc[t][k] += tv[t] * uv;
    }
  }
#pragma unroll
  for (int t = 0; t < AP_TOK; ++t)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double s = wave_sum_f64(acc[t][k]);
      if (lane == 0 && t0 + t <= HW) w[l.sc + (long long)(t0 + t) * AP_HEADS + 8 * wave + k] = (s + w[l.cst + 8 * wave + k]) * 0.125;
    }
}

// grid (32, n): softmax over the HW + 1 tokens of one head, in place
__global__ __launch_bounds__(NT) void ap_softmax_kernel(int HW, double* __restrict__ ws, ApWs l) {
  __shared__ double red[NT];
  const int tid = threadIdx.x, h = blockIdx.x, n = blockIdx.y;
  double* sc = ws + n * l.total + l.sc + h;
  double m = -INFINITY;
  for (int t = tid; t <= HW; t += NT) m = fmax(m, sc[(long long)t * AP_HEADS]);
  red[tid] = m;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  m = red[0];
  __syncthreads();
  double sum = 0.0;
  for (int t = tid; t <= HW; t += NT) {
    const double e = exp(sc[(long long)t * AP_HEADS] - m);
    sc[(long long)t * AP_HEADS] = e;
    sum += e;
  }
  red[tid] = sum;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  sum = red[0];
  for (int t = tid; t <= HW; t += NT) sc[(long long)t * AP_HEADS] /= sum;
}

// grid (S, 2048 / NT, n): part[s][h][c] = sum over the slice's feature tokens of a_t,h T_t[c], tokens ascending
__global__ __launch_bounds__(NT) void ap_pv_partial_kernel(const float* __restrict__ x, long long ld, int HW, double* __restrict__ ws, ApWs l) {
  const int c = blockIdx.y * NT + threadIdx.x, s = blockIdx.x, n = blockIdx.z;
  double* w = ws + n * l.total;
  const int t0 = s * AP_SLICE, cnt = min(AP_SLICE, HW - t0);
  const float* xp = x + ((long long)n * HW + t0) * ld + c;
  const double* a = w + l.sc + (long long)(t0 + 1) * AP_HEADS;       // feature token i of the slice is token t0 + 1 + i
  double acc[AP_HEADS];
#pragma unroll
  for (int h = 0; h < AP_HEADS; ++h) acc[h] = 0.0;
  for (int i = 0; i < cnt; ++i) {
    const double v = (double)xp[(long long)i * ld];
#pragma unroll
    for (int h = 0; h < AP_HEADS; ++h) acc[h] += a[(long long)i * AP_HEADS + h] * v;
  }
#pragma unroll
  for (int h = 0; h < AP_HEADS; ++h) w[l.part + ((long long)s * AP_HEADS + h) * AP_C + c] = acc[h];
}

// grid (2048 / NT, 32, n): the mean token's share, then the slices in order
__global__ __launch_bounds__(NT) void ap_pv_merge_kernel(int S, double* __restrict__ ws, ApWs l) {
  const int c = blockIdx.x * NT + threadIdx.x, h = blockIdx.y, n = blockIdx.z;
  double* w = ws + n * l.total;
  double sum = w[l.sc + h] * w[l.mean + c];
  for (int s = 0; s < S; ++s) sum += w[l.part + ((long long)s * AP_HEADS + h) * AP_C + c];
  w[l.pv + (long long)h * AP_C + c] = sum;
}

// ------------------------------------------------------------------ score ------------------------------------------------------------------
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();                             // the previous use of red is over
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(NT) void clipiqa_score_kernel(const float* __restrict__ emb, const double* __restrict__ text, int pairs, int dim,
                                                           double scale, double* __restrict__ out) {
  __shared__ double red[NT];
  const int tid = threadIdx.x, n = blockIdx.x;
  const float* e = emb + (long long)n * dim;
  double ss = 0.0;
  for (int c = tid; c < dim; c += NT) ss += (double)e[c] * (double)e[c];
  const double norm = sqrt(block_sum_f64(ss, red));
  double tot = 0.0;
  for (int p = 0; p < pairs; ++p) {
    double dp = 0.0, dn = 0.0;
    for (int c = tid; c < dim; c += NT) {
      const double f = (double)e[c] / norm;
      dp += f * text[(long long)(2 * p) * dim + c];
      dn += f * text[(long long)(2 * p + 1) * dim + c];
    }
    const double lp = scale * block_sum_f64(dp, red), ln = scale * block_sum_f64(dn, red);
    tot += 1.0 / (1.0 + exp(ln - lp));
  }
  if (tid == 0) out[n] = tot / (double)pairs;
}

size_t ap_ws_bytes(int n, int h, int w) { return (size_t)n * (size_t)ap_layout((long long)h * w).total * sizeof(double); }

}  // namespace

// ------------------------------------------------------------- C entries -------------------------------------------------------------
extern "C" int dove_avgpool_cl_f32(const float* x, long long ldx, int n, int h, int w, int c, float* out, long long ldo, void* stream) {
  DOVE_CHECK_ARG(x && out, "dove_avgpool_cl_f32: null x / out");
  DOVE_CHECK_ARG(n > 0 && h >= 2 && w >= 2 && c > 0, "dove_avgpool_cl_f32: n, c must be positive and h, w at least 2");
  DOVE_CHECK_ARG(ldx >= c && ldo >= c, "dove_avgpool_cl_f32: ldx %lld or ldo %lld < c %d", ldx, ldo, c);
  const int ho = h / 2, wo = w / 2;
  const long long total = (long long)n * ho * wo * c;
  DOVE_CHECK_ARG(total < MAX_ELEMS, "dove_avgpool_cl_f32: tensor too large");
  hipLaunchKernelGGL(avgpool_cl_kernel, dim3(blocks_for(total)), dim3(NT), 0, (hipStream_t)stream, x, ldx, h, w, c, ho, wo, total, out, ldo);
  DOVE_CHECK_LAUNCH("dove_avgpool_cl_f32");
  return DOVE_OK;
}

extern "C" size_t dove_clip_attnpool_workspace_bytes(int n, int h, int w) { return (n > 0 && h > 0 && w > 0) ? ap_ws_bytes(n, h, w) : 0; }

extern "C" int dove_clip_attnpool_f32(const float* x, long long ldx, int n, int h, int w, const float* wq, const float* bq, const float* wk,
                                      const float* bk, const float* wv, const float* bv, const float* wc, const float* bc, void* ws,
                                      size_t ws_bytes, float* out, void* stream) {
  DOVE_CHECK_ARG(x && wq && bq && wk && bk && wv && bv && wc && bc && ws && out, "dove_clip_attnpool_f32: null x / weights / ws / out");
  DOVE_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && (long long)h * w < (1LL << 24),
                 "dove_clip_attnpool_f32: n (<= 65535), h, w must be positive and h w below 2^24");
  DOVE_CHECK_ARG(ldx >= AP_C, "dove_clip_attnpool_f32: ldx %lld < %d channels", ldx, AP_C);
  DOVE_CHECK_ARG(ws_bytes >= ap_ws_bytes(n, h, w), "dove_clip_attnpool_f32: workspace of %zu bytes, %zu needed", ws_bytes, ap_ws_bytes(n, h, w));
  const int HW = h * w, S = (HW + AP_SLICE - 1) / AP_SLICE;
  const ApWs l = ap_layout(HW);
  double* d = (double*)ws;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ap_mean_partial_kernel, dim3(S, AP_C / NT, n), dim3(NT), 0, st, x, ldx, HW, d, l);
  hipLaunchKernelGGL(ap_mean_merge_kernel, dim3(AP_C / NT, n), dim3(NT), 0, st, HW, S, d, l);
  hipLaunchKernelGGL(ap_matvec_kernel, dim3(AP_C / 4, n), dim3(NT), 0, st, wq, bq, AP_C, AP_C, d, l.total, l.mean, l.q, (float*)nullptr);
  hipLaunchKernelGGL(ap_u_kernel, dim3(AP_C / NT, AP_HEADS, n), dim3(NT), 0, st, wk, bk, d, l);
  hipLaunchKernelGGL(ap_scores_kernel, dim3((HW + 1 + AP_TOK - 1) / AP_TOK, n), dim3(NT), 0, st, x, ldx, HW, d, l);
  hipLaunchKernelGGL(ap_softmax_kernel, dim3(AP_HEADS, n), dim3(NT), 0, st, HW, d, l);
  hipLaunchKernelGGL(ap_pv_partial_kernel, dim3(S, AP_C / NT, n), dim3(NT), 0, st, x, ldx, HW, d, l);
  hipLaunchKernelGGL(ap_pv_merge_kernel, dim3(AP_C / NT, AP_HEADS, n), dim3(NT), 0, st, S, d, l);
  hipLaunchKernelGGL(ap_matvec_kernel, dim3(AP_C / 4, n), dim3(NT), 0, st, wv, bv, AP_C, AP_HD, d, l.total, l.pv, l.o, (float*)nullptr);
  hipLaunchKernelGGL(ap_matvec_kernel, dim3(AP_OUT / 4, n), dim3(NT), 0, st, wc, bc, AP_OUT, AP_OUT, d, l.total, l.o, 0LL, out);
  DOVE_CHECK_LAUNCH("dove_clip_attnpool_f32");
  return DOVE_OK;
}

extern "C" int dove_clipiqa_score(const float* emb, const double* text, int n, int pairs, int dim, double logit_scale, double* out,
                                  void* stream) {
  DOVE_CHECK_ARG(emb && text && out, "dove_clipiqa_score: null emb / text / out");
  DOVE_CHECK_ARG(n > 0 && pairs > 0 && dim > 0, "dove_clipiqa_score: n, pairs, dim must be positive");
  hipLaunchKernelGGL(clipiqa_score_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, emb, text, pairs, dim, logit_scale, out);
  DOVE_CHECK_LAUNCH("dove_clipiqa_score");
  return DOVE_OK;
}
