// MANIQA (include/dove_hip.h has the contract): what pyiqa's `maniqa` needs beside the fp32 metric block's LayerNorm,
// GELU, flash attention with heads of 64 (musiq.hip), the K % 32 == 0 Linear (conv_f32.hip) and the window gather / scatter (swin3d.hip).
// Activations are fp32; no atomics; repeated calls give identical bits; a sample's values do not depend on the batch it is in.
//
// bmm_f32_kernel<BT, TR>: per batch z, out = alpha (A B) (+ bias) (+ residual) on v_mfma_f32_32x32x2_f32.  A is [M][K] rows of stride lda; B is
//   [K][N] rows of stride ldb, or (BT) [N][K] rows of stride ldb, the q k^T form; batch strides may be 0 (a shared operand).  One 256-thread
//   block owns a 128 x 128 tile, its four waves a 2 x 2 grid of 64 x 64 quarters (2 x 2 accumulators each).  K advances 32 at a time through
//   double-buffered LDS, loaded 16 bytes at a time: K, N, lda, ldb and the batch strides are multiples of 4 and a, b 16-byte aligned, so a
//   chunk lies inside or outside K (or N) as a whole.  The last K step issues only the MFMAs of the k that exist, so every output is exactly
//   one fp32 fmaf chain over k = 0 .. K - 1 ascending, whatever M, N, the tile and the batch: the promise of conv_f32.hip's walks, kept here
//   for K % 32 != 0 (784 = 24 x 32 + 16).  Rows >= M and columns >= N load zeros and store nothing.  Epilogue, each step rounded on its own:
//   v = chain; v *= alpha (when alpha != 1); v += bias[n] (or bias[m] under DOVE_BMM_BIAS_ROWS); v += res; the store.  TR stores out[n][m]
//   (rows of stride ldo) and reads the residual the same way: the transposed store is what turns MANIQA's `transpose(1, 2).reshape` quirk and
//   its token-row <-> channel-row changes into a GEMM's epilogue.  The residual may be out (each element is read and written by one thread).
//   LDS banks (ds_read_b32: bank = dword address mod 32 within a 32-lane half): A [128][33] and the transposed B [128][33] are read at row
//   r0 + l, column 2 s + half: 33 (r0 + l) + k, 32 different banks; B [32][128] is read along a row.  As conv_f32.hip's tile_body.
// softmax_rows_f32_kernel: one 256-thread block per row of any length: the true row maximum, e = expf(x - max) (the accurate expf) written to
//   out, the sum of e with thread t adding columns t, t + 256, ... ascending, a fixed butterfly per wave and the four waves in order, then
//   out = e / sum.  out may be x.
// window_attention_f32_kernel: one workgroup per (window, head) for windows of n <= 64 tokens and heads of 32 j <= 192 columns.  K (padded to
//   hd + 1 dwords per row) and V of the window, the per-token region ids and the head's column of the bias table stay in LDS.  Wave w owns
//   query rows 32 w .. 32 w + 31; it computes S^T = K Q^T for the one or two key tiles (keys down, queries across: a lane holds one query and 16
//   of a tile's 32 keys), s = (q . k) scale + table[index[query][key]][head] + (-100 where the region ids differ); keys >= n score -inf.  All
//   scores of a row are in registers, so the softmax is the two-pass one without recomputation: the true maximum, p = expf(s - max), the row
//   sum in key order (registers ascending, tile 0 then tile 1, then the other half-wave), then O^T += V^T P^T per 32 columns of the head,
//   out = O / sum.  As swin3d.hip's kernel, whose head width is fixed at 32.
// maniqa_crops_kernel: one thread per crop pixel.  Crop k of frame f starts at origins[k] (clamped into the frame); its pixel (y, x) is
//   (v - 0.5) / 0.5 in fp64 without contraction, rounded once (u8 read as u / 255.0), written as the patch embedding's GEMM row ((f crops + k)
//   g + y / P) g + x / P, column c P P + (y % P) P + x % P: the order of a flattened Conv2d weight [out][3][P][P].
// maniqa_tokens_kernel: out[b][0] = cls + pos[0], out[b][1 + t] = emb[b T + t] + pos[1 + t].
// mix_f32_kernel<TR>: out = alpha a (+ r), each step rounded on its own, on [rows][cols] matrices per batch; TR writes out[col][row] through a
//   32 x 33 LDS tile.  The hooked-block gather (token rows without cls -> channel rows) and x = scale layer(x) + x are this kernel.
// maniqa_crop_score_kernel: one 1024-thread block per crop, fp64.  hidden rows [frames crops positions][2 hid]: the score branch's hidden
//   units, then the weight branch's.  Per position (a wave each, lane c, c + 64, ..., fixed butterfly) f = relu(wf . h + bf), w =
//   sigmoid(ww . h' + bw); a wave adds f w and w of its positions in order, the 16 waves are added in order, crop = sum f w / sum w.
// maniqa_frame_mean_kernel: one thread per frame: the mean of its crops' scores, added in crop order.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int GM = 128, GN = 128, GK = 32, GLD = GK + 1;
constexpr int G_FA = GM * GLD, G_FB = GN * GLD;                       // B [32][128] needs 4096 floats, transposed [128][33] 4224: one size
constexpr int G_LDS = 2 * (G_FA + G_FB) * (int)sizeof(float);         // 67,584 bytes: dynamic
constexpr int WA_T = 32, WA_MAX_N = 64, WA_MAX_HD = 192, WA_MAX_LDS = 128 * 1024;
constexpr int SC_NT = 1024;
constexpr int TT = 32;

inline unsigned blocks_for(long long total, int nt) { return (unsigned)((total + nt - 1) / nt); }

// --------------------------------------------------------------- batched GEMM ---------------------------------------------------------------
struct BmmP {
  const float *a, *b, *bias, *res;
  float* out;
  int M, N, K, bias_rows;
  float alpha;
  long long lda, ldb, ldo, ldr, sa, sb, so, sr;
};

__device__ __forceinline__ float bmm_epilogue(float v, float alpha, bool has_bias, float bias, bool has_res, float res) {
#pragma clang fp contract(off)
  if (alpha != 1.f) v = v * alpha;
  if (has_bias) v = v + bias;
  if (has_res) v = v + res;
  return v;
}

template <bool BT, bool TR>
__global__ __launch_bounds__(NT) void bmm_f32_kernel(BmmP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const As = smem;                      // [2][GM][GLD]
  float* const Bs = smem + 2 * G_FA;           // [2][GK][GN], or transposed [2][GN][GLD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int m0 = blockIdx.x * GM, n0 = blockIdx.y * GN;
  const float* A = p.a + (long long)blockIdx.z * p.sa;
  const float* B = p.b + (long long)blockIdx.z * p.sb;

  // A loader (and the transposed B's): the 16-byte chunk aq of rows ar + 32 j; B [K][N] loader: chunk bq of k rows br + 8 j
  const int aq = tid & 7, ar = tid >> 3, bq = tid & 31, br = tid >> 5;
  const float* ap[4];
  const float* bp[4];
  bool aok[4], bok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m0 + ar + 32 * j;
    aok[j] = m < p.M;
    ap[j] = A + (long long)(aok[j] ? m : 0) * p.lda + aq * 4;
    if (BT) {
      const int n = n0 + ar + 32 * j;
      bok[j] = n < p.N;
      bp[j] = B + (long long)(bok[j] ? n : 0) * p.ldb + aq * 4;
    } else {
      bok[j] = n0 + bq * 4 < p.N;              // N % 4 == 0: a chunk is inside or outside as a whole
      bp[j] = B + (long long)(br + 8 * j) * p.ldb + (bok[j] ? n0 + bq * 4 : 0);
    }
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

  int kl = 0;                                  // the first k of the next load
  f32x4 av[4], bv[4];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load = [&]() {
    const bool kok = kl + aq * 4 < p.K;        // K % 4 == 0
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      av[j] = (aok[j] && kok) ? *(const f32x4*)(ap[j] + kl) : zero4;
      if (BT) bv[j] = (bok[j] && kok) ? *(const f32x4*)(bp[j] + kl) : zero4;
      else bv[j] = (bok[j] && kl + br + 8 * j < p.K) ? *(const f32x4*)(bp[j] + (long long)kl * p.ldb) : zero4;
    }
    kl += GK;
  };
  auto stage = [&](int buf) {
    float* a = As + buf * G_FA;
    float* b = Bs + buf * G_FB;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float* d = a + (ar + 32 * j) * GLD + aq * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = av[j][e];
      if (BT) {
        float* t = b + (ar + 32 * j) * GLD + aq * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = bv[j][e];
      } else {
        *(f32x4*)(b + (br + 8 * j) * GN + bq * 4) = bv[j];
      }
    }
  };

  const int KT = (p.K + GK - 1) / GK;
  load();
  stage(0);
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < KT) load();                   // in flight under this step's MFMAs
    const float* a0 = As + buf * G_FA + (wm + l31) * GLD + half;
    const float* a1 = a0 + 32 * GLD;
    const float* b0 = BT ? Bs + buf * G_FB + (wn + l31) * GLD + half : Bs + buf * G_FB + half * GN + wn + l31;
    auto step = [&](int s) {
      const float x0 = a0[2 * s], x1 = a1[2 * s];
      const float y0 = BT ? b0[2 * s] : b0[2 * s * GN];
      const float y1 = BT ? b0[32 * GLD + 2 * s] : b0[2 * s * GN + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, y0, acc[0][0], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, y0, acc[1][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, y1, acc[0][1], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, y1, acc[1][1], 0, 0, 0);
    };
    const int left = p.K - kt * GK;            // block-uniform
    if (left >= GK) {
#pragma unroll
      for (int s = 0; s < GK / 2; ++s) step(s);
    } else {                                   // the last, short step: only the k that exist (K is even)
      for (int s = 0; s < left / 2; ++s) step(s);
    }
    if (kt + 1 < KT) stage(buf ^ 1);           // the other buffer: its readers finished before the barrier that ended step kt - 1
    __syncthreads();
  }

  float* out = p.out + (long long)blockIdx.z * p.so;
  const float* res = p.res ? p.res + (long long)blockIdx.z * p.sr : nullptr;
  const bool brow = p.bias && p.bias_rows, bcol = p.bias && !p.bias_rows;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 32 * j + l31;
    if (n >= p.N) continue;
    const float bn = bcol ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= p.M) continue;
        const long long o = TR ? (long long)n * p.ldo + m : (long long)m * p.ldo + n;
        const float rv = res ? res[TR ? (long long)n * p.ldr + m : (long long)m * p.ldr + n] : 0.f;
        out[o] = bmm_epilogue(acc[i][j][r], p.alpha, p.bias != nullptr, brow ? p.bias[m] : bn, res != nullptr, rv);
      }
  }
}

// ---------------------------------------------------------------- row softmax ----------------------------------------------------------------
__global__ __launch_bounds__(NT) void softmax_rows_f32_kernel(const float* x, long long ldx, int cols, float* out, long long ldo) {
  __shared__ float red[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xr = x + (long long)blockIdx.x * ldx;
  float* o = out + (long long)blockIdx.x * ldo;
  float mx = -INFINITY;
  for (int c = tid; c < cols; c += NT) mx = fmaxf(mx, xr[c]);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();                             // red is reused
  float sum = 0.f;
  for (int c = tid; c < cols; c += NT) {       // out may be x: a thread reads and writes its own columns only
    const float e = expf(xr[c] - mx);
    o[c] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  const float total = ((red[0] + red[1]) + red[2]) + red[3];
  for (int c = tid; c < cols; c += NT) o[c] = o[c] / total;
}

// -------------------------------------------------------------- window attention --------------------------------------------------------------
struct WinP {
  const float *q, *k, *v;
  long long ld;
  int n, heads, hd;
  float scale;
  const float* table;
  int table_rows;
  const int *index, *region;
  int id_windows;
  float* out;
  long long ldo;
};

__global__ __launch_bounds__(128) void window_attention_f32_kernel(WinP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int N = p.n, Npad = (N + WA_T - 1) / WA_T * WA_T, D = p.hd, LDK = D + 1, D4 = D >> 2;
  float* Ks = smem;                            // [Npad][D + 1]
  float* Vs = Ks + Npad * LDK;                 // [Npad][D]; Npad LDK is a multiple of 32 floats
  int* regS = (int*)(Vs + Npad * D);
  float* tabS = (float*)(regS + Npad);         // this head's column of the table
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int head = blockIdx.y, col0 = head * D, tiles = Npad / WA_T;
  const long long base = (long long)blockIdx.x * N;
  const long long idw = (long long)(blockIdx.x % p.id_windows) * N;

  for (int e = tid; e < Npad * D4; e += blockDim.x) {
    const int row = e / D4, c4 = (e - row * D4) * 4;
    f32x4 kk = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
    if (row < N) {
      const long long off = (base + row) * p.ld + col0 + c4;
      kk = *(const f32x4*)(p.k + off);
      vv = *(const f32x4*)(p.v + off);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) Ks[row * LDK + c4 + i] = kk[i];
    *(f32x4*)(Vs + row * D + c4) = vv;
  }
  for (int row = tid; row < Npad; row += blockDim.x) regS[row] = (p.region && row < N) ? p.region[idw + row] : 0;
  for (int i = tid; i < p.table_rows; i += blockDim.x) tabS[i] = p.table[(long long)i * p.heads + head];
  __syncthreads();

  // this wave: query rows 32 wave .. 32 wave + 31 (blockDim.x = 64 tiles); this lane: query l31, keys 32 kt + (r & 3) + 8 (r >> 2) + 4 half
  const int qrow = wave * WA_T + l31, qr = min(qrow, N - 1);
  const bool two = tiles == 2;                 // block-uniform
  f32x16 s0, s1;
#pragma unroll
  for (int r = 0; r < 16; ++r) s0[r] = s1[r] = 0.f;
  {
    const float* qp = p.q + (base + qr) * p.ld + col0 + half;   // Q[qrow][2 s + half]: the B operand of S^T = K Q^T
    const float* k0 = Ks + l31 * LDK + half;
    const float* k1 = k0 + WA_T * LDK;
    for (int s = 0; s < D / 2; ++s) {
      const float qv = qrow < N ? qp[2 * s] : 0.f;
      s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[2 * s], qv, s0, 0, 0, 0);
      if (two) s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[2 * s], qv, s1, 0, 0, 0);
    }
  }
  const int rq = regS[qr];
  const int* irow = p.index + (long long)qr * N;
  auto finish = [&](f32x16& sa, int kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * WA_T + (r & 3) + 8 * (r >> 2) + 4 * half;
      float s = -INFINITY;
      if (key < N) {
        const int id = min(max(irow[key], 0), p.table_rows - 1);
        s = sa[r] * p.scale + tabS[id];
        if (regS[key] != rq) s += -100.f;
      }
      sa[r] = s;
    }
  };
  finish(s0, 0);
  if (two) finish(s1, 1);
  float mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s0[r]);
  if (two) {
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s1[r]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32));          // finite: key 0 exists and the mask is finite
  float sum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    s0[r] = expf(s0[r] - mx);
    sum += s0[r];
  }
  if (two) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s1[r] = expf(s1[r] - mx);
      sum += s1[r];
    }
  }
  sum += __shfl_xor(sum, 32);

  for (int j = 0; j < D / 32; ++j) {           // O^T[d][query] += V^T[d][key] P^T[key][query] for the head's columns 32 j .. 32 j + 31
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* vp = Vs + ((r & 3) + 8 * (r >> 2) + 4 * half) * D + 32 * j + l31;
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[0], s0[r], o, 0, 0, 0);
    }
    if (two) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* vp = Vs + (WA_T + (r & 3) + 8 * (r >> 2) + 4 * half) * D + 32 * j + l31;
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[0], s1[r], o, 0, 0, 0);
      }
    }
    if (qrow < N) {
      float* op = p.out + (base + qrow) * p.ldo + col0 + 32 * j + 4 * half;
#pragma unroll
      for (int g = 0; g < 4; ++g) {            // d = 32 j + 8 g + 4 half + (0 .. 3)
        const f32x4 a = {o[4 * g] / sum, o[4 * g + 1] / sum, o[4 * g + 2] / sum, o[4 * g + 3] / sum};
        *(f32x4*)(op + 8 * g) = a;
      }
    }
  }
}

// ------------------------------------------------------------------ crop gather ------------------------------------------------------------------
__device__ __forceinline__ double view_value(const dove_image_view& v, long long off) {
  if (v.dtype == DOVE_U8) return (double)((const uint8_t*)v.data)[off] / 255.0;
  if (v.dtype == DOVE_BF16) return (double)bf2f(((const bf16_t*)v.data)[off]);
  return (double)((const float*)v.data)[off];
}

__device__ __forceinline__ double centred(double x) {
#pragma clang fp contract(off)
  return (x - 0.5) / 0.5;
}

__global__ __launch_bounds__(NT) void maniqa_crops_kernel(dove_image_view v, int c, int H, int W, const int* __restrict__ origins, int crops,
                                                          int side, int patch, long long total, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % side), y = (int)((idx / side) % side), k = (int)((idx / ((long long)side * side)) % crops);
  const long long f = idx / ((long long)side * side * crops);
  const int sy = min(max(origins[2 * k], 0), H - side) + y, sx = min(max(origins[2 * k + 1], 0), W - side) + x;
  const long long base = f * v.sn + (long long)sy * v.sh + (long long)sx * v.sw;
  const int g = side / patch, pp = patch * patch;
  const long long row = ((f * crops + k) * g + y / patch) * g + x / patch;
  float* o = out + row * 3 * pp + (y % patch) * patch + x % patch;
  float r[3];
  r[0] = (float)centred(view_value(v, base));
  r[1] = c == 1 ? r[0] : (float)centred(view_value(v, base + v.sc));
  r[2] = c == 1 ? r[0] : (float)centred(view_value(v, base + 2 * v.sc));
  o[0] = r[0];
  o[pp] = r[1];
  o[2 * pp] = r[2];
}

// ------------------------------------------------------------- cls and positions -------------------------------------------------------------
__global__ __launch_bounds__(NT) void maniqa_tokens_kernel(const float* __restrict__ emb, const float* __restrict__ cls,
                                                           const float* __restrict__ pos, int T, int dim, long long total,
                                                           float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int ch = (int)(idx % dim);
  const long long row = idx / dim;
  const int t = (int)(row % (T + 1));
  const long long b = row / (T + 1);
  const float a = t == 0 ? cls[ch] : emb[(b * T + t - 1) * dim + ch];
  out[idx] = a + pos[(long long)t * dim + ch];
}

// ------------------------------------------------------------ scale, add, transpose ------------------------------------------------------------
struct MixP {
  const float *a, *r;
  float* out;
  int rows, cols;
  float alpha;
  long long lda, ldr, ldo, sa, sr, so;
};

__device__ __forceinline__ float mixed(float a, float alpha, bool has_r, float r) {
#pragma clang fp contract(off)
  if (alpha != 1.f) a = alpha * a;
  if (has_r) a = a + r;
  return a;
}

template <bool TR>
__global__ __launch_bounds__(NT) void mix_f32_kernel(MixP p) {
  __shared__ float tile[TT][TT + 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;        // 32 x 8
  const int c0 = blockIdx.x * TT, r0 = blockIdx.y * TT;
  const float* a = p.a + (long long)blockIdx.z * p.sa;
  const float* r = p.r ? p.r + (long long)blockIdx.z * p.sr : nullptr;
  float* out = p.out + (long long)blockIdx.z * p.so;
#pragma unroll
  for (int j = 0; j < TT; j += 8) {
    const int row = r0 + ty + j, col = c0 + tx;
    if (row < p.rows && col < p.cols) {
      const float v = mixed(a[(long long)row * p.lda + col], p.alpha, r != nullptr, r ? r[(long long)row * p.ldr + col] : 0.f);
      if (TR) tile[ty + j][tx] = v;
      else out[(long long)row * p.ldo + col] = v;
    }
  }
  if (!TR) return;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TT; j += 8) {
    const int col = c0 + ty + j, row = r0 + tx;                  // lanes along the source rows: the transposed output's columns
    if (row < p.rows && col < p.cols) out[(long long)col * p.ldo + row] = tile[tx][ty + j];
  }
}

// -------------------------------------------------------------------- score --------------------------------------------------------------------
__global__ __launch_bounds__(SC_NT) void maniqa_crop_score_kernel(const float* __restrict__ hidden, long long ld, int positions, int hid,
                                                                  const float* __restrict__ wf, const float* __restrict__ bf,
                                                                  const float* __restrict__ ww, const float* __restrict__ bw,
                                                                  double* __restrict__ crop_scores) {
  __shared__ double num[SC_NT / 64], den[SC_NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* crop = hidden + (long long)blockIdx.x * positions * ld;
  double sn = 0.0, sd = 0.0;
  for (int t = wave; t < positions; t += SC_NT / 64) {
    const float* h = crop + (long long)t * ld;
    double a = 0.0, b = 0.0;
    for (int c = lane; c < hid; c += 64) {
      a += (double)wf[c] * (double)h[c];
      b += (double)ww[c] * (double)h[hid + c];
    }
    const double f = fmax(wave_sum_f64(a) + (double)bf[0], 0.0);
    const double w = 1.0 / (1.0 + exp(-(wave_sum_f64(b) + (double)bw[0])));
    sn += f * w;
    sd += w;
  }
  if (lane == 0) {
    num[wave] = sn;
    den[wave] = sd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double n = 0.0, d = 0.0;
    for (int w = 0; w < SC_NT / 64; ++w) {
      n += num[w];
      d += den[w];
    }
    crop_scores[blockIdx.x] = n / d;
  }
}

__global__ __launch_bounds__(NT) void maniqa_frame_mean_kernel(const double* __restrict__ crop_scores, int frames, int crops,
                                                               double* __restrict__ out) {
  const int f = blockIdx.x * NT + threadIdx.x;
  if (f >= frames) return;
  double s = 0.0;
  for (int k = 0; k < crops; ++k) s += crop_scores[(long long)f * crops + k];   // crop order
  out[f] = s / (double)crops;
}

const char* bmm_name(int flags) {
  const bool bt = flags & DOVE_BMM_B_TRANSPOSED, tr = flags & DOVE_BMM_STORE_TRANSPOSED;
  return bt ? (tr ? "bmm_f32_kernel<bt,tr>" : "bmm_f32_kernel<bt>") : (tr ? "bmm_f32_kernel<tr>" : "bmm_f32_kernel");
}

}  // namespace

// ------------------------------------------------------------- C entries -------------------------------------------------------------
extern "C" void dove_bmm_f32_tiles(int* m_tile, int* n_tile, int* k_tile) {
  if (m_tile) *m_tile = GM;
  if (n_tile) *n_tile = GN;
  if (k_tile) *k_tile = GK;
}

extern "C" const char* dove_bmm_f32_kernel_name(int flags) { return bmm_name(flags); }

extern "C" int dove_bmm_f32(const float* a, long long lda, long long sa, const float* b, long long ldb, long long sb, const float* bias,
                            const float* res, long long ldr, long long sr, float* out, long long ldo, long long so, int batch, int m, int n,
                            int k, float alpha, int flags, void* stream) {
  DOVE_CHECK_ARG(a && b && out, "dove_bmm_f32: null a / b / out");
  DOVE_CHECK_ARG((flags & ~(DOVE_BMM_B_TRANSPOSED | DOVE_BMM_STORE_TRANSPOSED | DOVE_BMM_BIAS_ROWS)) == 0, "dove_bmm_f32: unknown flags %d", flags);
  const bool bt = flags & DOVE_BMM_B_TRANSPOSED, tr = flags & DOVE_BMM_STORE_TRANSPOSED;
  DOVE_CHECK_ARG(batch > 0 && batch <= 65535 && m > 0 && n > 0 && k > 0 && k % 4 == 0 && n % 4 == 0 && (n + GN - 1) / GN <= 65535,
                 "dove_bmm_f32: batch %d (1 .. 65535), m %d, n %d, k %d (positive; k and n multiples of 4)", batch, m, n, k);
  DOVE_CHECK_ARG(lda >= k && ldb >= (bt ? k : n) && lda % 4 == 0 && ldb % 4 == 0 && sa >= 0 && sb >= 0 && sa % 4 == 0 && sb % 4 == 0,
                 "dove_bmm_f32: lda %lld, ldb %lld, batch strides %lld, %lld must hold the rows, be non-negative and multiples of 4", lda, ldb, sa, sb);
  DOVE_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "dove_bmm_f32: a and b must be 16-byte aligned");
  DOVE_CHECK_ARG(ldo >= (tr ? m : n) && so >= 0 && (batch == 1 || so > 0), "dove_bmm_f32: ldo %lld, output batch stride %lld", ldo, so);
  DOVE_CHECK_ARG(!res || (ldr >= (tr ? m : n) && sr >= 0), "dove_bmm_f32: ldr %lld, residual batch stride %lld", ldr, sr);
  static PerDeviceOnce attr_set;
  if (auto once_ = attr_set.guard()) {
    (void)hipFuncSetAttribute((const void*)bmm_f32_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS);
    (void)hipFuncSetAttribute((const void*)bmm_f32_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS);
    (void)hipFuncSetAttribute((const void*)bmm_f32_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS);
    (void)hipFuncSetAttribute((const void*)bmm_f32_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, G_LDS);
  }
  BmmP p{a, b, bias, res, out, m, n, k, (flags & DOVE_BMM_BIAS_ROWS) ? 1 : 0, alpha, lda, ldb, ldo, ldr, sa, sb, so, sr};
  const dim3 grid((unsigned)((m + GM - 1) / GM), (unsigned)((n + GN - 1) / GN), (unsigned)batch);
  if (bt && tr) hipLaunchKernelGGL((bmm_f32_kernel<true, true>), grid, dim3(NT), G_LDS, (hipStream_t)stream, p);
  else if (bt) hipLaunchKernelGGL((bmm_f32_kernel<true, false>), grid, dim3(NT), G_LDS, (hipStream_t)stream, p);
  else if (tr) hipLaunchKernelGGL((bmm_f32_kernel<false, true>), grid, dim3(NT), G_LDS, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((bmm_f32_kernel<false, false>), grid, dim3(NT), G_LDS, (hipStream_t)stream, p);
  DOVE_CHECK_LAUNCH("dove_bmm_f32");
  return DOVE_OK;
}

extern "C" int dove_softmax_rows_f32(const float* x, long long ldx, long long rows, int cols, float* out, long long ldo, void* stream) {
  DOVE_CHECK_ARG(x && out, "dove_softmax_rows_f32: null x / out");
  DOVE_CHECK_ARG(rows > 0 && rows <= 0x7fffffffLL && cols > 0 && ldx >= cols && ldo >= cols,
                 "dove_softmax_rows_f32: rows %lld, cols %d, ldx %lld, ldo %lld", rows, cols, ldx, ldo);
  hipLaunchKernelGGL(softmax_rows_f32_kernel, dim3((unsigned)rows), dim3(NT), 0, (hipStream_t)stream, x, ldx, cols, out, ldo);
  DOVE_CHECK_LAUNCH("dove_softmax_rows_f32");
  return DOVE_OK;
}

extern "C" void dove_window_attention_tiles(int* tile, int* max_n, int* max_head_dim) {
  if (tile) *tile = WA_T;
  if (max_n) *max_n = WA_MAX_N;
  if (max_head_dim) *max_head_dim = WA_MAX_HD;
}

extern "C" int dove_window_attention_f32(const float* q, const float* k, const float* v, long long ld, long long windows, int n, int heads,
                                         int head_dim, float scale, const float* table, int table_rows, const int* index, const int* region,
                                         int id_windows, float* out, long long ldo, void* stream) {
  DOVE_CHECK_ARG(q && k && v && table && index && out, "dove_window_attention_f32: null q / k / v / table / index / out");
  DOVE_CHECK_ARG(windows > 0 && windows <= 0x7fffffffLL && n >= 1 && n <= WA_MAX_N && heads > 0 && heads <= 65535 && table_rows > 0,
                 "dove_window_attention_f32: windows %lld, n %d (1 .. %d), heads %d (1 .. 65535), table_rows %d", windows, n, WA_MAX_N, heads,
                 table_rows);
  DOVE_CHECK_ARG(head_dim >= 32 && head_dim <= WA_MAX_HD && head_dim % 32 == 0, "dove_window_attention_f32: head_dim %d (a multiple of 32, <= %d)",
                 head_dim, WA_MAX_HD);
  DOVE_CHECK_ARG(ld >= (long long)heads * head_dim && ldo >= (long long)heads * head_dim && ld % 4 == 0 && ldo % 4 == 0,
                 "dove_window_attention_f32: ld %lld and ldo %lld must hold %d heads of %d and be multiples of 4", ld, ldo, heads, head_dim);
  DOVE_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0,
                 "dove_window_attention_f32: q, k, v, out must be 16-byte aligned");
  DOVE_CHECK_ARG(!region || (id_windows > 0 && windows % id_windows == 0), "dove_window_attention_f32: id_windows %d must divide windows %lld",
                 id_windows, windows);
  const int npad = (n + WA_T - 1) / WA_T * WA_T, tiles = npad / WA_T;
  const size_t lds = (size_t)npad * (2 * head_dim + 1) * sizeof(float) + (size_t)npad * sizeof(int) + (size_t)table_rows * sizeof(float);
  DOVE_CHECK_ARG(lds <= WA_MAX_LDS, "dove_window_attention_f32: a window of %d tokens, heads of %d and a table of %d rows need %zu bytes of LDS (limit %d)",
                 n, head_dim, table_rows, lds, WA_MAX_LDS);
  static PerDeviceOnce attr_set;
  if (auto once_ = attr_set.guard())
    (void)hipFuncSetAttribute((const void*)window_attention_f32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WA_MAX_LDS);
  WinP a{q, k, v, ld, n, heads, head_dim, scale, table, table_rows, index, region, region ? id_windows : 1, out, ldo};
  hipLaunchKernelGGL(window_attention_f32_kernel, dim3((unsigned)windows, (unsigned)heads), dim3(64 * tiles), lds, (hipStream_t)stream, a);
  DOVE_CHECK_LAUNCH("dove_window_attention_f32");
  return DOVE_OK;
}

extern "C" int dove_maniqa_crops_f32(const dove_image_view* img, int n, int c, int h, int w, const int* origins, int crops, int side, int patch,
                                     float* out, void* stream) {
  DOVE_CHECK_ARG(img && img->data && origins && out, "dove_maniqa_crops_f32: null view / data / origins / out");
  DOVE_CHECK_ARG(img->dtype >= DOVE_F32 && img->dtype <= DOVE_U8, "dove_maniqa_crops_f32: bad dtype %d (0 f32, 1 bf16, 2 u8)", img->dtype);
  DOVE_CHECK_ARG(n > 0 && (c == 1 || c == 3) && crops > 0 && patch > 0 && side > 0 && side % patch == 0 && h >= side && w >= side,
                 "dove_maniqa_crops_f32: n %d, c %d (1 or 3), %d crops of %d (a multiple of the patch %d) in a %d x %d frame", n, c, crops, side,
                 patch, h, w);
  const long long total = (long long)n * crops * side * side;
  DOVE_CHECK_ARG(total < (long long)NT * 0x7fffffffLL, "dove_maniqa_crops_f32: batch too large");
  hipLaunchKernelGGL(maniqa_crops_kernel, dim3(blocks_for(total, NT)), dim3(NT), 0, (hipStream_t)stream, *img, c, h, w, origins, crops, side, patch,
                     total, out);
  DOVE_CHECK_LAUNCH("dove_maniqa_crops_f32");
  return DOVE_OK;
}

extern "C" int dove_maniqa_tokens_f32(const float* emb, const float* cls, const float* pos, long long n, int tokens, int dim, float* out,
                                      void* stream) {
  DOVE_CHECK_ARG(emb && cls && pos && out && emb != out, "dove_maniqa_tokens_f32: null emb / cls / pos / out, or out aliasing emb");
  DOVE_CHECK_ARG(n > 0 && tokens > 0 && dim > 0, "dove_maniqa_tokens_f32: n, tokens, dim must be positive");
  const long long total = n * (tokens + 1) * dim;
  DOVE_CHECK_ARG(total < (long long)NT * 0x7fffffffLL, "dove_maniqa_tokens_f32: batch too large");
  hipLaunchKernelGGL(maniqa_tokens_kernel, dim3(blocks_for(total, NT)), dim3(NT), 0, (hipStream_t)stream, emb, cls, pos, tokens, dim, total, out);
  DOVE_CHECK_LAUNCH("dove_maniqa_tokens_f32");
  return DOVE_OK;
}

extern "C" int dove_mix_f32(const float* a, long long lda, long long sa, const float* r, long long ldr, long long sr, float alpha, int batch,
                            int rows, int cols, int transpose, float* out, long long ldo, long long so, void* stream) {
  DOVE_CHECK_ARG(a && out, "dove_mix_f32: null a / out");
  DOVE_CHECK_ARG(batch > 0 && batch <= 65535 && rows > 0 && cols > 0 && (rows + TT - 1) / TT <= 65535,
                 "dove_mix_f32: batch %d (1 .. 65535), rows %d (<= 2097120), cols %d", batch, rows, cols);
  DOVE_CHECK_ARG(lda >= cols && (!r || ldr >= cols) && ldo >= (transpose ? rows : cols) && sa >= 0 && sr >= 0 && so >= 0,
                 "dove_mix_f32: lda %lld, ldr %lld, ldo %lld must hold the rows; batch strides non-negative", lda, ldr, ldo);
  DOVE_CHECK_ARG(!transpose || (out != a && out != r), "dove_mix_f32: the transposed output must not be an input");
  MixP p{a, r, out, rows, cols, alpha, lda, ldr, ldo, sa, sr, so};
  const dim3 grid((unsigned)((cols + TT - 1) / TT), (unsigned)((rows + TT - 1) / TT), (unsigned)batch);
  if (transpose) hipLaunchKernelGGL(mix_f32_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(mix_f32_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, p);
  DOVE_CHECK_LAUNCH("dove_mix_f32");
  return DOVE_OK;
}

extern "C" int dove_maniqa_score(const float* hidden, long long ld, int frames, int crops, int positions, int hid, const float* wf,
                                 const float* bf, const float* ww, const float* bw, double* crop_scores, double* out, void* stream) {
  DOVE_CHECK_ARG(hidden && wf && bf && ww && bw && crop_scores && out && crop_scores != out,
                 "dove_maniqa_score: null hidden / wf / bf / ww / bw / crop_scores / out, or out aliasing crop_scores");
  DOVE_CHECK_ARG(frames > 0 && crops > 0 && (long long)frames * crops <= 0x7fffffffLL && positions > 0 && hid > 0 && ld >= 2LL * hid,
                 "dove_maniqa_score: frames %d, crops %d, positions %d, hid %d, ld %lld (>= 2 hid)", frames, crops, positions, hid, ld);
  hipLaunchKernelGGL(maniqa_crop_score_kernel, dim3((unsigned)(frames * crops)), dim3(SC_NT), 0, (hipStream_t)stream, hidden, ld, positions, hid,
                     wf, bf, ww, bw, crop_scores);
  DOVE_CHECK_LAUNCH("dove_maniqa_score");
  hipLaunchKernelGGL(maniqa_frame_mean_kernel, dim3(blocks_for(frames, NT)), dim3(NT), 0, (hipStream_t)stream, crop_scores, frames, crops, out);
  DOVE_CHECK_LAUNCH("dove_maniqa_score");
  return DOVE_OK;
}
