// MUSIQ (include/dove_hip.h has the contract): the operators of pyiqa's `musiq` that the fp32 metric block did not have.
// The convs and Linears of the network run on dove_resnet_conv_f32 (conv_f32.hip: the 1 x 1 walk is the fp32 MFMA GEMM, tokens as pixels)
// and dove_convnet_conv_f32 (the 7 x 7 stem conv on conv_f32_kernel, over the explicitly padded frame that the gather writes); this file
// adds what sits between them.  Activations are channels-last fp32; no atomics; repeated calls give identical bits; a frame's values do
// not depend on the batch it is in (every sum below belongs to one patch, one token row or one query row).
//
// musiq_patches_kernel: one thread per output pixel of out [n tp][side][side][3].  A token's 32 x 32 patch sits at [before, before + 32)^2
//   of its side x side frame, the rest is 0 (before 2, side 37 is the stem conv's 'same' frame; before 0, side 32 the bare patch).  A patch
//   pixel maps to (y, x) = 32 (i, j) + (py, px) - (pad_top, pad_left) of its scale's image; outside [0, rh) x [0, rw) it is the zero padding
//   of the mapped values.  Inside, the original-resolution scale is (float)(2 v - 1); a resized scale is torch's bicubic (A = -0.75,
//   align_corners = False, border-clamped indices, no antialias) of 2 v - 1 evaluated in fp64 from the source values (rows first: sum_a cy[a]
//   (sum_b cx[b] v[a][b]), taps ascending) and rounded once to fp32.  u8 is read as u / 255.0 in fp64.  The token table and the three
//   scales' geometry come from the host (dove_amd.musiq.token_geometry).
// musiq_groupnorm_kernel: one 256-thread block per patch map [side][side][c], 32 groups.  Eight threads own a group: thread s of the eight
//   adds elements s, s + 8, ... (element e = pixel e / cpg, channel e % cpg of the group) in fp64, the eight partials meet in a fixed
//   butterfly; the mean first, then the sum of squared deviations (two passes), var = that / count, rstd = 1 / sqrt(var + eps).  Output
//   (x - mean) rstd gamma + beta in fp64, plus the same of a second operand y when given (relu(gn3(x) + gn_proj(y))), rounded once to fp32,
//   then ReLU.  pool = 1: the zero-'same' (0 before, 1 after) 3 x 3 stride-2 max of those values is written instead, side / 2 square.
//   The map is read from global memory three times (64 KiB, cache-resident); LDS holds only the 4 x 32 statistics.
// layernorm_f32_kernel: one wave per row: fp64 mean, fp64 sum of squared deviations (lane c, c + 64, ... ascending, then a fixed butterfly),
//   (x - mean) rstd gamma + beta in fp64, one rounding.
// musiq_embed_kernel: out[f][0] = cls, out[f][1 + t] = (emb[f tp + t] + pos[spatial(t)]) + scale_emb[scale(t)] in fp32.
// mha_f32_kernel: multi-head attention, heads of 64, fp32 on v_mfma_f32_32x32x2_f32, flash-style (no T x T matrix in memory).
//   Q tile 64 rows (one 128-thread block: two waves of 32 query rows), KV tile 32 keys through LDS (K padded to 65 dwords per row so that
//   the 32 lanes of a half read 32 banks; V rows are read along d).  Per KV tile a wave computes S^T = K Q^T (keys down, queries across: a
//   lane holds one query and 16 of the 32 keys, the other half-wave the other 16), so the row maximum and row sum are 16 in-lane steps and
//   one exchange between the halves; P^T stays in registers as the B operand of O^T += V^T P^T.  s = (q . k) scale, the running maximum m,
//   l = l exp(m - m') + sum (registers ascending, then the other half), O scaled by exp(m - m'); keys >= T score -inf; out = O / l.  T >= 1.
//   expf is the accurate one.  Each MFMA chain runs in d order (scores) and key order (values).
// gelu_f32_kernel: its own pass, 0.5 x (1 + erff(x / sqrt 2)) in fp32.  (Not an epilogue of the GEMM: the 1 x 1 walk stays as it is.)
// musiq_score_kernel: one wave per frame, fp64: row_k = w_k . f + b_k (lane c, c + 64, ..., fixed butterfly); K = 1: the row; K > 1: sum_k
//   (k + 1) softmax(row)_k.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int PATCH = 32;
constexpr int GN_GROUPS = 32;
constexpr int AT_Q = 64, AT_KV = 32, AT_D = 64, AT_NT = 128, AT_LDK = AT_D + 1;
constexpr int SCORE_MAX_K = 64;

inline unsigned blocks_for(long long total, int nt) { return (unsigned)((total + nt - 1) / nt); }

struct Scales {
  dove_musiq_scale s[3];
};

// ----------------------------------------------------------------- patch gather -----------------------------------------------------------------
__device__ __forceinline__ double view_value(const dove_image_view& v, long long off) {
  if (v.dtype == DOVE_U8) return (double)((const uint8_t*)v.data)[off] / 255.0;
  if (v.dtype == DOVE_BF16) return (double)bf2f(((const bf16_t*)v.data)[off]);
  return (double)((const float*)v.data)[off];
}

// torch's cubic convolution coefficients for the fraction t (A = -0.75), taps -1, 0, 1, 2
__device__ __forceinline__ void cubic_coeffs(double t, double (&c)[4]) {
  const double A = -0.75;
  const double x0 = t + 1.0, x1 = t, x2 = 1.0 - t, x3 = 2.0 - t;
  c[0] = ((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A;
  c[1] = ((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0;
  c[2] = ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0;
  c[3] = ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A;
}

__global__ __launch_bounds__(NT) void musiq_patches_kernel(dove_image_view v, int c, int H, int W, Scales sc, const int* __restrict__ tokens,
                                                           int tp, int before, int side, long long total, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int px = (int)(idx % side), py = (int)((idx / side) % side);
  const long long pt = idx / ((long long)side * side);
  const int t = (int)(pt % tp);
  const long long f = pt / tp;
  const int s = tokens[4 * t], pi = tokens[4 * t + 1], pj = tokens[4 * t + 2];
  const dove_musiq_scale g = sc.s[s];
  const int yy = py - before, xx = px - before;
  float r[3] = {0.f, 0.f, 0.f};
  if (yy >= 0 && yy < PATCH && xx >= 0 && xx < PATCH) {
    const int y = pi * PATCH + yy - g.pad_top, x = pj * PATCH + xx - g.pad_left;
    if (y >= 0 && y < g.rh && x >= 0 && x < g.rw) {
      const long long base = f * v.sn;
      if (!g.resized) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          r[ch] = (float)(2.0 * view_value(v, base + (c == 1 ? 0 : ch) * v.sc + (long long)y * v.sh + (long long)x * v.sw) - 1.0);
      } else {
        const double ry = (double)H / (double)g.rh * ((double)y + 0.5) - 0.5, rx = (double)W / (double)g.rw * ((double)x + 0.5) - 0.5;
        const double fy = floor(ry), fx = floor(rx);
        double cy[4], cx[4];
        cubic_coeffs(ry - fy, cy);
        cubic_coeffs(rx - fx, cx);
        long long roff[4], coff[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          roff[a] = (long long)min(max((int)fy - 1 + a, 0), H - 1) * v.sh;
          coff[a] = (long long)min(max((int)fx - 1 + a, 0), W - 1) * v.sw;
        }
        for (int ch = 0; ch < (c == 1 ? 1 : 3); ++ch) {
          const long long cb = base + ch * v.sc;
          double acc = 0.0;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            double row = 0.0;
#pragma unroll
            for (int b = 0; b < 4; ++b) row += cx[b] * (2.0 * view_value(v, cb + roff[a] + coff[b]) - 1.0);
            acc += cy[a] * row;
          }
          r[ch] = (float)acc;
        }
        if (c == 1) r[1] = r[2] = r[0];
      }
    }
  }
  float* o = out + idx * 3;
  o[0] = r[0];
  o[1] = r[1];
  o[2] = r[2];
}

// ------------------------------------------------------------------ GroupNorm ------------------------------------------------------------------
__device__ __forceinline__ double sum8_f64(double v) {           // the eight threads of a group: a fixed butterfly
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

// mean and rstd of group g of one map, by the group's eight threads (sub = 0 .. 7); every one of them returns the same pair
__device__ __forceinline__ void group_stats(const float* __restrict__ x, int hw, int c, int cpg, int g, int sub, double eps, double& mean,
                                            double& rstd) {
  const int cnt = hw * cpg;
  const float* xg = x + g * cpg;
  double s = 0.0;
  for (int e = sub; e < cnt; e += 8) s += (double)xg[(long long)(e / cpg) * c + e % cpg];
  mean = sum8_f64(s) / (double)cnt;
  double q = 0.0;
  for (int e = sub; e < cnt; e += 8) {
    const double d = (double)xg[(long long)(e / cpg) * c + e % cpg] - mean;
    q += d * d;
  }
  rstd = 1.0 / sqrt(sum8_f64(q) / (double)cnt + eps);
}

__global__ __launch_bounds__(NT) void musiq_groupnorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ y,
                                                             const float* __restrict__ gamma_y, const float* __restrict__ beta_y, int side, int c,
                                                             double eps, int relu, int pool, float* out) {
  __shared__ double st[4][GN_GROUPS];          // mean x, rstd x, mean y, rstd y
  const int tid = threadIdx.x, hw = side * side, cpg = c / GN_GROUPS;
  const long long map = (long long)blockIdx.x * hw * c;
  const float* xm = x + map;
  const float* ym = y ? y + map : nullptr;
  {
    const int g = tid >> 3, sub = tid & 7;
    double mean, rstd;
    group_stats(xm, hw, c, cpg, g, sub, eps, mean, rstd);
    if (sub == 0) {
      st[0][g] = mean;
      st[1][g] = rstd;
    }
    if (ym) {
      group_stats(ym, hw, c, cpg, g, sub, eps, mean, rstd);
      if (sub == 0) {
        st[2][g] = mean;
        st[3][g] = rstd;
      }
    }
  }
  __syncthreads();
  if (!pool) {
    float* om = out + map;                     // may be x: every element is read and written by one thread, after the statistics
    for (int e = tid; e < hw * c; e += NT) {
      const int ch = e % c, g = ch / cpg;
      double v = ((double)xm[e] - st[0][g]) * st[1][g] * (double)gamma[ch] + (double)beta[ch];
      if (ym) v += ((double)ym[e] - st[2][g]) * st[3][g] * (double)gamma_y[ch] + (double)beta_y[ch];
      float r = (float)v;
      if (relu) r = fmaxf(r, 0.f);
      om[e] = r;
    }
  } else {
    const int so = side / 2;
    float* om = out + (long long)blockIdx.x * so * so * c;
    for (int e = tid; e < so * so * c; e += NT) {
      const int ch = e % c, g = ch / cpg, ox = (e / c) % so, oy = e / (c * so);
      const double mean = st[0][g], a = st[1][g] * (double)gamma[ch], b = (double)beta[ch];
      float m = -INFINITY;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int iy = 2 * oy + dy, ix = 2 * ox + dx;
          float r = 0.f;                       // the zero padding behind the last row and column
          if (iy < side && ix < side) {
            r = (float)(((double)xm[((long long)iy * side + ix) * c + ch] - mean) * a + b);
            if (relu) r = fmaxf(r, 0.f);
          }
          m = fmaxf(m, r);
        }
      om[e] = m;
    }
  }
}

// ------------------------------------------------------------------ LayerNorm ------------------------------------------------------------------
__global__ __launch_bounds__(NT) void layernorm_f32_kernel(const float* __restrict__ x, long long ldx, long long rows, int dim,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, double eps,
                                                           float* __restrict__ out, long long ldo) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                       // a whole wave leaves together
  const float* xr = x + r * ldx;
  double s = 0.0;
  for (int c = lane; c < dim; c += 64) s += (double)xr[c];
  const double mean = wave_sum_f64(s) / (double)dim;
  double q = 0.0;
  for (int c = lane; c < dim; c += 64) {
    const double d = (double)xr[c] - mean;
    q += d * d;
  }
  const double rstd = 1.0 / sqrt(wave_sum_f64(q) / (double)dim + eps);
  float* o = out + r * ldo;
  for (int c = lane; c < dim; c += 64) o[c] = (float)(((double)xr[c] - mean) * rstd * (double)gamma[c] + (double)beta[c]);
}

// ------------------------------------------------------------- embeddings and cls -------------------------------------------------------------
__global__ __launch_bounds__(NT) void musiq_embed_kernel(const float* __restrict__ emb, const float* __restrict__ pos,
                                                         const float* __restrict__ scale_emb, const float* __restrict__ cls,
                                                         const int* __restrict__ tokens, int tp, int dim, long long total, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int ch = (int)(idx % dim);
  const long long row = idx / dim;
  const int t = (int)(row % (tp + 1));
  const long long f = row / (tp + 1);
  if (t == 0) {
    out[idx] = cls[ch];
    return;
  }
  const int s = tokens[4 * (t - 1)], sp = tokens[4 * (t - 1) + 3];
  out[idx] = (emb[(f * tp + t - 1) * dim + ch] + pos[(long long)sp * dim + ch]) + scale_emb[s * dim + ch];
}

// ------------------------------------------------------------------ attention ------------------------------------------------------------------
__global__ __launch_bounds__(AT_NT) void mha_f32_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                        long long ld, int T, float scale, float* __restrict__ out, long long ldo) {
  __shared__ __attribute__((aligned(16))) float Ks[AT_KV * AT_LDK];
  __shared__ __attribute__((aligned(16))) float Vs[AT_KV * AT_D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const long long base = (long long)blockIdx.z * T;
  const int col0 = blockIdx.y * AT_D;
  const int qrow = blockIdx.x * AT_Q + wave * 32 + l31;

  float qf[AT_D / 2];                          // Q[qrow][2 s + half]: the B operand of S^T = K Q^T
  {
    const float* qp = q + (base + min(qrow, T - 1)) * ld + col0 + half;
#pragma unroll
    for (int s = 0; s < AT_D / 2; ++s) qf[s] = qrow < T ? qp[2 * s] : 0.f;
  }
  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) o0[r] = o1[r] = 0.f;
  float m = -INFINITY, l = 0.f;

  // tile loader: 32 rows x 16 chunks of 16 bytes = 512 chunks each for K and V, four per thread
  f32x4 kr[4], vr[4];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + AT_NT * j, row = e >> 4, c4 = (e & 15) * 4;
      const bool ok = k0 + row < T;
      const long long off = (base + (ok ? k0 + row : 0)) * ld + col0 + c4;
      kr[j] = ok ? *(const f32x4*)(k + off) : zero4;
      vr[j] = ok ? *(const f32x4*)(v + off) : zero4;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + AT_NT * j, row = e >> 4, c4 = (e & 15) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) Ks[row * AT_LDK + c4 + i] = kr[j][i];
      *(f32x4*)(Vs + row * AT_D + c4) = vr[j];
    }
  };

  const int tiles = (T + AT_KV - 1) / AT_KV;
  load(0);
  for (int kt = 0; kt < tiles; ++kt) {
    __syncthreads();                           // the readers of the previous tile are done
    stage();
    __syncthreads();
    if (kt + 1 < tiles) load((kt + 1) * AT_KV);   // in flight under this tile's MFMAs

    f32x16 sa;
#pragma unroll
    for (int r = 0; r < 16; ++r) sa[r] = 0.f;
    const float* kp = Ks + l31 * AT_LDK + half;
#pragma unroll
    for (int s = 0; s < AT_D / 2; ++s) sa = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * s], qf[s], sa, 0, 0, 0);

    // this lane: query l31, keys kt 32 + (r & 3) + 8 (r >> 2) + 4 half
    float mx = m;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * AT_KV + (r & 3) + 8 * (r >> 2) + 4 * half;
      sa[r] = key < T ? sa[r] * scale : -INFINITY;
      mx = fmaxf(mx, sa[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));        // finite: key kt 32 of the tile exists
    const float alpha = expf(m - mx);          // 0 on the first tile
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sa[r] = expf(sa[r] - mx);
      sum += sa[r];
    }
    sum += __shfl_xor(sum, 32);
    l = l * alpha + sum;
    m = mx;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      o0[r] *= alpha;
      o1[r] *= alpha;
    }
    // O^T[d][query] += V^T[d][key] P^T[key][query]: the two keys of step r are this half's and the other half's register r
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* vp = Vs + ((r & 3) + 8 * (r >> 2) + 4 * half) * AT_D + l31;
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[0], sa[r], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[32], sa[r], o1, 0, 0, 0);
    }
  }
  if (qrow < T) {
    float* op = out + (base + qrow) * ldo + col0 + 4 * half;
#pragma unroll
    for (int g = 0; g < 4; ++g) {              // d = 8 g + 4 half + (0 .. 3), and 32 more for o1
      const f32x4 a = {o0[4 * g] / l, o0[4 * g + 1] / l, o0[4 * g + 2] / l, o0[4 * g + 3] / l};
      const f32x4 b = {o1[4 * g] / l, o1[4 * g + 1] / l, o1[4 * g + 2] / l, o1[4 * g + 3] / l};
      *(f32x4*)(op + 8 * g) = a;
      *(f32x4*)(op + 32 + 8 * g) = b;
    }
  }
}

// -------------------------------------------------------------------- GELU --------------------------------------------------------------------
__global__ __launch_bounds__(NT) void gelu_f32_kernel(const float* __restrict__ x, long long total, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const float a = x[i];
  out[i] = 0.5f * a * (1.0f + erff(a * 0.70710678118654752440f));
}

// -------------------------------------------------------------------- score --------------------------------------------------------------------
__global__ __launch_bounds__(64) void musiq_score_kernel(const float* __restrict__ feat, long long ld, const float* __restrict__ w,
                                                         const float* __restrict__ b, int dim, int K, double* __restrict__ out) {
  const int lane = threadIdx.x;
  const float* f = feat + (long long)blockIdx.x * ld;
  __shared__ double row[SCORE_MAX_K];
  for (int kk = 0; kk < K; ++kk) {
    double s = 0.0;
    for (int c = lane; c < dim; c += 64) s += (double)w[(long long)kk * dim + c] * (double)f[c];
    s = wave_sum_f64(s) + (double)b[kk];
    if (lane == 0) row[kk] = s;
  }
  if (lane != 0) return;                       // lane 0 reads what it wrote
  if (K == 1) {
    out[blockIdx.x] = row[0];
    return;
  }
  double mx = row[0];
  for (int kk = 1; kk < K; ++kk) mx = fmax(mx, row[kk]);
  double den = 0.0, num = 0.0;
  for (int kk = 0; kk < K; ++kk) {
    const double e = exp(row[kk] - mx);
    den += e;
    num += (double)(kk + 1) * e;
  }
  out[blockIdx.x] = num / den;
}

}  // namespace

// ------------------------------------------------------------- C entries -------------------------------------------------------------
extern "C" int dove_musiq_patches_f32(const dove_image_view* img, int n, int c, int h, int w, const dove_musiq_scale* scales, const int* tokens,
                                      int tokens_per_frame, int before, int side, float* out, void* stream) {
  DOVE_CHECK_ARG(img && img->data && scales && tokens && out, "dove_musiq_patches_f32: null view / data / scales / tokens / out");
  DOVE_CHECK_ARG(n > 0 && (c == 1 || c == 3) && h > 0 && w > 0 && tokens_per_frame > 0,
                 "dove_musiq_patches_f32: n, h, w, tokens_per_frame must be positive and c 1 or 3 (n %d c %d h %d w %d tokens %d)", n, c, h, w,
                 tokens_per_frame);
  DOVE_CHECK_ARG(img->dtype >= DOVE_F32 && img->dtype <= DOVE_U8, "dove_musiq_patches_f32: bad dtype %d (0 f32, 1 bf16, 2 u8)", img->dtype);
  DOVE_CHECK_ARG(before >= 0 && side >= before + PATCH && side <= 64, "dove_musiq_patches_f32: before %d, side %d (side >= before + 32, <= 64)",
                 before, side);
  Scales sc;
  for (int s = 0; s < 3; ++s) {
    sc.s[s] = scales[s];
    DOVE_CHECK_ARG(sc.s[s].rh > 0 && sc.s[s].rw > 0 && sc.s[s].pad_top >= 0 && sc.s[s].pad_left >= 0 &&
                       (sc.s[s].resized || (sc.s[s].rh == h && sc.s[s].rw == w)),
                   "dove_musiq_patches_f32: scale %d: %d x %d, padding %d / %d, resized %d of a %d x %d image", s, sc.s[s].rh, sc.s[s].rw,
                   sc.s[s].pad_top, sc.s[s].pad_left, sc.s[s].resized, h, w);
  }
  const long long total = (long long)n * tokens_per_frame * side * side;
  DOVE_CHECK_ARG(total < (long long)NT * 0x7fffffffLL, "dove_musiq_patches_f32: batch too large");
  hipLaunchKernelGGL(musiq_patches_kernel, dim3(blocks_for(total, NT)), dim3(NT), 0, (hipStream_t)stream, *img, c, h, w, sc, tokens,
                     tokens_per_frame, before, side, total, out);
  DOVE_CHECK_LAUNCH("dove_musiq_patches_f32");
  return DOVE_OK;
}

extern "C" int dove_musiq_groupnorm_f32(const float* x, const float* gamma, const float* beta, const float* y, const float* gamma_y,
                                        const float* beta_y, long long maps, int side, int c, double eps, int relu, int pool, float* out,
                                        void* stream) {
  DOVE_CHECK_ARG(x && gamma && beta && out, "dove_musiq_groupnorm_f32: null x / gamma / beta / out");
  DOVE_CHECK_ARG(!y || (gamma_y && beta_y), "dove_musiq_groupnorm_f32: a second operand needs its gamma and beta");
  DOVE_CHECK_ARG(maps > 0 && maps <= 0x7fffffffLL && side > 0 && side <= 64 && c > 0 && c % GN_GROUPS == 0 && c <= 1024,
                 "dove_musiq_groupnorm_f32: maps %lld, side %d (<= 64), c %d (a multiple of 32, <= 1024)", maps, side, c);
  DOVE_CHECK_ARG(!pool || (!y && side >= 2 && out != x), "dove_musiq_groupnorm_f32: the pool takes one operand, side >= 2 and its own output");
  DOVE_CHECK_ARG(eps > 0.0, "dove_musiq_groupnorm_f32: eps must be positive");
  hipLaunchKernelGGL(musiq_groupnorm_kernel, dim3((unsigned)maps), dim3(NT), 0, (hipStream_t)stream, x, gamma, beta, y, gamma_y, beta_y, side, c,
                     eps, relu, pool, out);
  DOVE_CHECK_LAUNCH("dove_musiq_groupnorm_f32");
  return DOVE_OK;
}

extern "C" int dove_layernorm_f32(const float* x, long long ldx, long long rows, int dim, const float* gamma, const float* beta, double eps,
                                  float* out, long long ldo, void* stream) {
  DOVE_CHECK_ARG(x && gamma && beta && out, "dove_layernorm_f32: null x / gamma / beta / out");
  DOVE_CHECK_ARG(rows > 0 && rows < (1LL << 32) && dim > 0 && ldx >= dim && ldo >= dim && eps > 0.0,
                 "dove_layernorm_f32: rows %lld, dim %d, ldx %lld, ldo %lld, eps %g", rows, dim, ldx, ldo, eps);
  hipLaunchKernelGGL(layernorm_f32_kernel, dim3(blocks_for(rows, NT / 64)), dim3(NT), 0, (hipStream_t)stream, x, ldx, rows, dim, gamma, beta, eps,
                     out, ldo);
  DOVE_CHECK_LAUNCH("dove_layernorm_f32");
  return DOVE_OK;
}

extern "C" int dove_musiq_embed_f32(const float* emb, const float* pos, const float* scale_emb, const float* cls, const int* tokens, int n,
                                    int tokens_per_frame, int dim, float* out, void* stream) {
  DOVE_CHECK_ARG(emb && pos && scale_emb && cls && tokens && out, "dove_musiq_embed_f32: null emb / pos / scale_emb / cls / tokens / out");
  DOVE_CHECK_ARG(n > 0 && tokens_per_frame > 0 && dim > 0, "dove_musiq_embed_f32: n, tokens_per_frame, dim must be positive");
  const long long total = (long long)n * (tokens_per_frame + 1) * dim;
  DOVE_CHECK_ARG(total < (long long)NT * 0x7fffffffLL, "dove_musiq_embed_f32: batch too large");
  hipLaunchKernelGGL(musiq_embed_kernel, dim3(blocks_for(total, NT)), dim3(NT), 0, (hipStream_t)stream, emb, pos, scale_emb, cls, tokens,
                     tokens_per_frame, dim, total, out);
  DOVE_CHECK_LAUNCH("dove_musiq_embed_f32");
  return DOVE_OK;
}

extern "C" int dove_mha_f32(const float* q, const float* k, const float* v, long long ld, int n, int t, int heads, float scale, float* out,
                            long long ldo, void* stream) {
  DOVE_CHECK_ARG(q && k && v && out, "dove_mha_f32: null q / k / v / out");
  DOVE_CHECK_ARG(n > 0 && n <= 65535 && t > 0 && heads > 0 && heads <= 65535, "dove_mha_f32: n %d, heads %d (1 .. 65535), t %d (>= 1)", n, heads, t);
  DOVE_CHECK_ARG(ld >= (long long)heads * AT_D && ldo >= (long long)heads * AT_D && ld % 4 == 0 && ldo % 4 == 0,
                 "dove_mha_f32: ld %lld and ldo %lld must hold %d heads of 64 and be multiples of 4", ld, ldo, heads);
  DOVE_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0, "dove_mha_f32: q, k, v, out must be 16-byte aligned");
  hipLaunchKernelGGL(mha_f32_kernel, dim3((unsigned)((t + AT_Q - 1) / AT_Q), (unsigned)heads, (unsigned)n), dim3(AT_NT), 0, (hipStream_t)stream, q,
                     k, v, ld, t, scale, out, ldo);
  DOVE_CHECK_LAUNCH("dove_mha_f32");
  return DOVE_OK;
}

extern "C" void dove_mha_f32_tiles(int* q_tile, int* kv_tile) {
  if (q_tile) *q_tile = AT_Q;
  if (kv_tile) *kv_tile = AT_KV;
}

extern "C" int dove_gelu_f32(const float* x, long long count, float* out, void* stream) {
  DOVE_CHECK_ARG(x && out && count > 0 && count < (long long)NT * 0x7fffffffLL, "dove_gelu_f32: null x / out, or a count outside (0, 2^39)");
  hipLaunchKernelGGL(gelu_f32_kernel, dim3(blocks_for(count, NT)), dim3(NT), 0, (hipStream_t)stream, x, count, out);
  DOVE_CHECK_LAUNCH("dove_gelu_f32");
  return DOVE_OK;
}

extern "C" int dove_musiq_score(const float* features, long long ld, const float* w, const float* b, int n, int dim, int k, double* out,
                                void* stream) {
  DOVE_CHECK_ARG(features && w && b && out, "dove_musiq_score: null features / w / b / out");
  DOVE_CHECK_ARG(n > 0 && dim > 0 && ld >= dim && k >= 1 && k <= SCORE_MAX_K, "dove_musiq_score: n %d, dim %d, ld %lld, k %d (1 .. %d)", n, dim, ld,
                 k, SCORE_MAX_K);
  hipLaunchKernelGGL(musiq_score_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, features, ld, w, b, dim, k, out);
  DOVE_CHECK_LAUNCH("dove_musiq_score");
  return DOVE_OK;
}
