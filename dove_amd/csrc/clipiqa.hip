// CLIP-IQA (include/dove_hip.h has the contract): the operators of CLIP RN50's ModifiedResNet in exact fp32, the
// attention-pool head and the prompt-pair score in fp64.  Activations are channels-last fp32 [n][h][w][c] with pixel strides, weights
// [kh][kw][cin][cout] with BatchNorm folded in by the host, as in percep.hip.
//
// dove_resnet_conv_f32 chooses one of four walks from the arguments alone (dove_resnet_conv_f32_kernel_name):
//   pointwise_f32_kernel (new): k = 1, stride 1, cin % 32 == 0, cout % 4 == 0, ldx % 4 == 0, 16-byte aligned x and w.  A plain GEMM of M = n h w
//     pixels on v_mfma_f32_32x32x2_f32.  One 256-thread block owns 128 pixels x TN channels, TN = 128 for cout >= 128 and 64 below; the four
//     waves form a 2 x 2 grid of 64 x TN/2 quarters.  K advances 32 channels at a time through double-buffered LDS exactly as in
//     convnet3x3_f32_kernel: the loads of step k + 1 are issued before the MFMAs of step k, one barrier per step.  K ascends in one fmaf
//     chain per output, no split-K, so the bits do not depend on TN or on the tile an output falls in and equal conv_f32_kernel's.  With
//     pool = 2 (the same body, MODE_POOL) the A loader keeps the four input pixels of an output pixel in flight and stages ((a + b) + (c + d)) * 0.25f: the conv of the 2 x 2
//     average (floor sizes) without the pooled map ever being written.  Epilogue: (acc + bias) + residual, then ReLU.  residual may be out:
//     each element is read and written by the same thread.
//   convnet3x3_n64_f32_kernel (new): k = 3, stride 1, pad 1, cin % 32 == 0, cout in {32, 64}: the walk of convnet3x3_f32_kernel (tap-major K,
//     one tap x 32 channels per step, a 9-bit tap mask per row) on the 128 x 64 tile, so no MFMA of the stem and stage-1 convs multiplies an
//     empty half tile.  Same K order, same bits.
//   convnet3x3_f32_kernel (percep.hip, called through its hidden launcher): k = 3, stride 1, cout >= 128.
//   conv_f32_kernel (flow.hip): everything else, i.e. the 3 -> 32 stride-2 stem conv (K = 27) and a k = 1 conv whose cin is no multiple
//     of 32.  It has neither a residual nor pool-on-load: those two are refused outside pointwise_f32_kernel.
//   LDS banks of the two new walks (one body): fragments are read with ds_read_b32, bank = dword address mod 32 within a 32-lane half.
//     A [128][33]: lane l of a half reads row r0 + l, column 2 s + half: dword 33 (r0 + l) + k, bank (const + l) mod 32: 32 different banks
//       (an unpadded row of 32 would put all lanes on one).  B [32][TN]: lane l reads row 2 s + half, column c0 + l: consecutive dwords, 32
//       different banks for TN = 64 as for 128, since a row is a multiple of 32 dwords and the lanes walk along it.
//     A is filled with ds_write_b32: a half holds rows r .. r + 3 x 8 chunks q, dword 33 row + 4 q + e -> bank (const + (l >> 3) + 4 (l & 7))
//       mod 32, all different.  B is filled with 16-byte writes of consecutive dwords.
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

int dove_conv_f32_general_launch(const float* x, const float* w, const float* bias, float* out, int n, int h, int w_in, int cin, int cout,
                                 int kh, int kw, int stride, int pad_h, int pad_w, int relu, long long ldx, long long ldo, void* stream);
int dove_convnet3x3_fast_launch(const float* x, const float* w, const float* bias, float* out, int n, int h, int w_in, int cin, int cout,
                                int relu, long long ldx, long long ldo, void* stream);

namespace {

constexpr int NT = 256;
constexpr int TM = 128, TK = 32, TLDA = TK + 1;
constexpr int AP_SLICE = 256;                                       // tokens per attention-pool partial
constexpr int AP_C = 2048, AP_HEADS = 32, AP_HD = 64, AP_OUT = 1024;
constexpr int AP_TOK = 4;                                           // tokens per block of the score kernel
constexpr long long MAX_ELEMS = (long long)NT * 0x7fffffffLL;
const char* const POINTWISE_NAME = "pointwise_f32_kernel";
const char* const N64_NAME = "convnet3x3_n64_f32_kernel";
const char* const FAST_NAME = "convnet3x3_f32_kernel";
const char* const GENERAL_NAME = "conv_f32_kernel";

inline unsigned blocks_for(long long total) { return (unsigned)((total + NT - 1) / NT); }
constexpr int tile_lds(int tn) { return 2 * (TM * TLDA + TK * tn) * (int)sizeof(float); }   // 66,560 bytes for 128, 50,176 for 64

// ------------------------------------------------- the 128 x TN tile: 1 x 1, pooled 1 x 1, 3 x 3 -------------------------------------------------
struct TileP {
  const float* x; const float* w; const float* bias; const float* res; float* out;
  int H, W, Cin, Cout, relu;                   // H, W: the output map (the pooled map under pool-on-load)
  int Hi, Wi;                                  // MODE_POOL: the input map, H = Hi / 2, W = Wi / 2
  long long M, ldx, ldr, ldo;
};

enum { MODE_1X1 = 0, MODE_POOL = 1, MODE_3X3 = 2 };

template <int TN, int MODE>
__device__ __forceinline__ void tile_body(const TileP& p) {
  constexpr int F_A = TM * TLDA, F_B = TK * TN;
  constexpr int BQ = TN / 4, BROWS = NT / BQ, NBJ = TK / BROWS;   // B loader: chunk bq of K rows br + BROWS j
  constexpr int WN = TN / 2, NJ = WN / 32;                        // a wave's columns and accumulators across
  constexpr int NP = MODE == MODE_POOL ? 4 : 1;                   // input pixels a row keeps in flight
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const As = smem;                      // [2][TM][TLDA]
  float* const Bs = smem + 2 * F_A;            // [2][TK][TN]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * TM;
  const int n0 = blockIdx.y * TN;

  // A loader: this thread reads the 16-byte chunk aq of rows ar + 32 j
  const int aq = tid & 7, ar = tid >> 3;
  const int bq = tid % BQ, br = tid / BQ;
  long long poff[4];
  unsigned vmask[4];                           // MODE_3X3: the valid taps; otherwise bit 0 = the row exists
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long m = m0 + ar + 32 * j;
    poff[j] = 0;
    vmask[j] = 0;
    if (m < p.M) {
      poff[j] = m * p.ldx + aq * 4;
      vmask[j] = 1u;
      if (MODE != MODE_1X1) {
        const long long hw = (long long)p.H * p.W, img = m / hw;
        const int r = (int)(m - img * hw), oy = r / p.W, ox = r - oy * p.W;
        if (MODE == MODE_POOL) poff[j] = ((img * p.Hi + 2 * oy) * p.Wi + 2 * ox) * p.ldx + aq * 4;   // the upper left of the four
        if (MODE == MODE_3X3) vmask[j] = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int iy = oy + t / 3 - 1, ix = ox + t % 3 - 1;
          if (MODE == MODE_3X3 && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) vmask[j] |= 1u << t;
        }
      }
    }
  }
  const bool bvalid = n0 + bq * 4 < p.Cout;    // cout % 4 == 0: a chunk is inside or outside as a whole
  const float* wp = p.w + (long long)br * p.Cout + n0 + bq * 4;

  f32x16 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * WN, l31 = lane & 31, half = lane >> 5;

  int tap = 0, kx = 0, ci = 0;
  long long toff = MODE == MODE_3X3 ? -((long long)p.W + 1) * p.ldx : 0;
  const long long wstep = (long long)TK * p.Cout, prow = (long long)p.Wi * p.ldx;
  f32x4 av[4][NP], bv[NBJ];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  auto load = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (MODE == MODE_3X3) {
        av[j][0] = ((vmask[j] >> tap) & 1u) ? *(const f32x4*)(p.x + poff[j] + toff + ci) : zero4;
      } else {
        const float* s = p.x + poff[j] + ci;
        av[j][0] = vmask[j] ? *(const f32x4*)s : zero4;
        if constexpr (MODE == MODE_POOL) {     // the other three pixels of the 2 x 2 window stay in flight with it
          av[j][1] = vmask[j] ? *(const f32x4*)(s + p.ldx) : zero4;
          av[j][2] = vmask[j] ? *(const f32x4*)(s + prow) : zero4;
          av[j][3] = vmask[j] ? *(const f32x4*)(s + prow + p.ldx) : zero4;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NBJ; ++j) bv[j] = bvalid ? *(const f32x4*)(wp + (long long)(BROWS * j) * p.Cout) : zero4;
    wp += wstep;
    ci += TK;
    if (MODE == MODE_3X3 && ci == p.Cin) {
      ci = 0;
      ++tap;
      toff += p.ldx;
      if (++kx == 3) {
        kx = 0;
        toff += ((long long)p.W - 3) * p.ldx;
      }
    }
  };
  auto stage = [&](int buf) {
    float* a = As + buf * F_A;
    float* b = Bs + buf * F_B;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float* d = a + (ar + 32 * j) * TLDA + aq * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (MODE == MODE_POOL) d[e] = ((av[j][0][e] + av[j][1][e]) + (av[j][2][e] + av[j][3][e])) * 0.25f;
        else d[e] = av[j][0][e];
      }
    }
#pragma unroll
    for (int j = 0; j < NBJ; ++j) *(f32x4*)(b + (br + BROWS * j) * TN + bq * 4) = bv[j];
  };

  const int KT = (MODE == MODE_3X3 ? 9 : 1) * (p.Cin / TK);
  load();
  stage(0);
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < KT) load();                   // in flight under this step's MFMAs
    const float* a0 = As + buf * F_A + (wm + l31) * TLDA + half;
    const float* a1 = a0 + 32 * TLDA;
    const float* b0 = Bs + buf * F_B + half * TN + wn + l31;
#pragma unroll
    for (int s = 0; s < TK / 2; ++s) {
      const float x0 = a0[2 * s], x1 = a1[2 * s];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float y = b0[2 * s * TN + 32 * j];
        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, y, acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, y, acc[1][j], 0, 0, 0);
      }
    }
    if (kt + 1 < KT) stage(buf ^ 1);           // the other buffer: its readers finished before the barrier that ended step kt - 1
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = n0 + wn + 32 * j + l31;
    if (n >= p.Cout) continue;
    const float b = p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= p.M) continue;
        float v = acc[i][j][r] + b;
        if (p.res) v += p.res[m * p.ldr + n];
        if (p.relu) v = fmaxf(v, 0.f);
        p.out[m * p.ldo + n] = v;
      }
  }
}

template <int TN, int MODE>
__global__ __launch_bounds__(NT) void pointwise_f32_kernel(TileP p) { tile_body<TN, MODE>(p); }

__global__ __launch_bounds__(NT) void convnet3x3_n64_f32_kernel(TileP p) { tile_body<64, MODE_3X3>(p); }

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

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
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

// ------------------------------------------------------------- conv dispatch -------------------------------------------------------------
enum Walk { WALK_REFUSED = 0, WALK_POINTWISE, WALK_N64, WALK_FAST, WALK_GENERAL };

Walk conv_walk(const dove_resnet_conv_f32_args* a, bool report) {
#define REFUSE(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      if (report) dove_set_error(__VA_ARGS__);   \
      return WALK_REFUSED;                       \
    }                                            \
  } while (0)
  REFUSE(a && a->struct_size == sizeof(dove_resnet_conv_f32_args), "dove_resnet_conv_f32: struct_size %u is not the library's %zu",
         a ? a->struct_size : 0u, sizeof(dove_resnet_conv_f32_args));
  REFUSE(a->x && a->w && a->out, "dove_resnet_conv_f32: null x / w / out");
  REFUSE(a->n > 0 && a->h > 0 && a->w_in > 0 && a->cin > 0 && a->cout > 0, "dove_resnet_conv_f32: n, h, w, cin, cout must be positive");
  REFUSE(a->k == 1 || a->k == 3, "dove_resnet_conv_f32: kernel side %d (1 or 3)", a->k);
  REFUSE(a->stride == 1 || a->stride == 2, "dove_resnet_conv_f32: stride %d (1 or 2)", a->stride);
  REFUSE(a->pool == 1 || a->pool == 2, "dove_resnet_conv_f32: pool %d (1 or 2)", a->pool);
  REFUSE(a->pool == 1 || (a->k == 1 && a->stride == 1), "dove_resnet_conv_f32: pool 2 belongs to a 1 x 1 conv of stride 1 (k %d, stride %d)", a->k,
         a->stride);
  REFUSE(a->pool == 1 || (a->h >= 2 && a->w_in >= 2), "dove_resnet_conv_f32: image %d x %d is smaller than the 2 x 2 pool", a->h, a->w_in);
  REFUSE(a->ldx >= a->cin && a->ldo >= a->cout && (!a->residual || a->ldr >= a->cout),
         "dove_resnet_conv_f32: ldx %lld < cin %d, ldo %lld or ldr %lld < cout %d", a->ldx, a->cin, a->ldo, a->ldr, a->cout);
  REFUSE((long long)a->n * a->h * a->w_in <= 0x7fffffffLL * 32 && (long long)a->n * a->h * a->w_in * a->ldx < (1LL << 46) &&
             (long long)a->k * a->k * a->cin < (1 << 24),
         "dove_resnet_conv_f32: problem too large");
  const bool vec = a->cin % TK == 0 && a->cout % 4 == 0 && a->ldx % 4 == 0 && ((uintptr_t)a->x & 15) == 0 && ((uintptr_t)a->w & 15) == 0;
  if (a->k == 1 && a->stride == 1 && vec) return WALK_POINTWISE;
  REFUSE(a->pool == 1 && !a->residual,
         "dove_resnet_conv_f32: pool 2 and a residual need pointwise_f32_kernel (k 1, stride 1, cin %% 32 == 0, cout %% 4 == 0, ldx %% 4 == 0, "
         "16-byte aligned x and w); got k %d, stride %d, cin %d, cout %d, ldx %lld", a->k, a->stride, a->cin, a->cout, a->ldx);
#undef REFUSE
  if (a->k == 3 && a->stride == 1 && vec) {
    if (a->cout == 32 || a->cout == 64) return WALK_N64;
    if (a->cout >= 128) return WALK_FAST;
  }
  return WALK_GENERAL;
}

template <typename K>
void launch_tile(K kernel, PerDeviceOnce& once, int tn, long long M, int cout, const TileP& p, void* stream) {
  if (auto once_ = once.guard()) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, tile_lds(tn));
  dim3 grid((unsigned)((M + TM - 1) / TM), (unsigned)((cout + tn - 1) / tn), 1);
  hipLaunchKernelGGL(kernel, grid, dim3(NT), tile_lds(tn), (hipStream_t)stream, p);
}

size_t ap_ws_bytes(int n, int h, int w) { return (size_t)n * (size_t)ap_layout((long long)h * w).total * sizeof(double); }

}  // namespace

// ------------------------------------------------------------- C entries -------------------------------------------------------------
extern "C" const char* dove_resnet_conv_f32_kernel_name(const dove_resnet_conv_f32_args* a) {
  switch (conv_walk(a, false)) {
    case WALK_POINTWISE: return POINTWISE_NAME;
    case WALK_N64: return N64_NAME;
    case WALK_FAST: return FAST_NAME;
    case WALK_GENERAL: return GENERAL_NAME;
    default: return "";
  }
}

extern "C" int dove_resnet_conv_f32(const dove_resnet_conv_f32_args* a, void* stream) {
  const Walk walk = conv_walk(a, true);
  if (walk == WALK_REFUSED) return DOVE_EINVAL;
  const int pad = a->k / 2;
  if (walk == WALK_GENERAL)
    return dove_conv_f32_general_launch(a->x, a->w, a->bias, a->out, a->n, a->h, a->w_in, a->cin, a->cout, a->k, a->k, a->stride, pad, pad,
                                        a->relu, a->ldx, a->ldo, stream);
  if (walk == WALK_FAST)
    return dove_convnet3x3_fast_launch(a->x, a->w, a->bias, a->out, a->n, a->h, a->w_in, a->cin, a->cout, a->relu, a->ldx, a->ldo, stream);
  TileP p;
  p.x = a->x; p.w = a->w; p.bias = a->bias; p.res = a->residual; p.out = a->out;
  p.H = a->h / a->pool; p.W = a->w_in / a->pool; p.Cin = a->cin; p.Cout = a->cout; p.relu = a->relu;
  p.Hi = a->h; p.Wi = a->w_in;
  p.M = (long long)a->n * p.H * p.W; p.ldx = a->ldx; p.ldr = a->ldr; p.ldo = a->ldo;
  static PerDeviceOnce once[5];
  if (walk == WALK_N64) {
    launch_tile(convnet3x3_n64_f32_kernel, once[0], 64, p.M, a->cout, p, stream);
  } else if (a->pool == 2) {
    if (a->cout >= 128) launch_tile(pointwise_f32_kernel<128, MODE_POOL>, once[1], 128, p.M, a->cout, p, stream);
    else launch_tile(pointwise_f32_kernel<64, MODE_POOL>, once[2], 64, p.M, a->cout, p, stream);
  } else {
    if (a->cout >= 128) launch_tile(pointwise_f32_kernel<128, MODE_1X1>, once[3], 128, p.M, a->cout, p, stream);
    else launch_tile(pointwise_f32_kernel<64, MODE_1X1>, once[4], 64, p.M, a->cout, p, stream);
  }
  DOVE_CHECK_LAUNCH("dove_resnet_conv_f32");
  return DOVE_OK;
}

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
