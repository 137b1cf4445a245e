// NIQE (pyiqa's 'niqe' with its defaults, a port of the MATLAB release), the no-reference metric of the reference's
// evaluation step, in fp64 on the device.
//
//   niqe_block_kernel<true>   one workgroup per 96 x 96 block of the cropped luma, all frames in one launch: luma of the block and a
//                             3-pixel halo into LDS (bytes: the rounded luma is an integer 0..255), the 7 x 7 Gaussian local mean and
//                             deviation separably (horizontal from LDS, vertical in registers), the MSCN block in LDS, the 5 x 6 moments
//                             of the in-block circular-shift products and the block's mean sigma; and the block's 48 x 48 tile of the
//                             half-scale image I2 (every tap of MATLAB's antialiased bicubic at 0.5, reflected ones included, lies in the
//                             block's halo), so the input is read from HBM once
//   niqe_block_kernel<false>  the same on 48 x 48 blocks of I2 (fp64 in LDS)
//   niqe_solve_kernel         one thread per (block, scale, product): moments -> alpha (table search) and the AGGD features
//   niqe_stats_kernel         one workgroup per frame: nanmean, NaN-free covariance, the two counts
//
// No atomics: every sum has a fixed order and two calls give the same bits.  The device runs only + - * fma / sqrt; exp (the Gaussian) and
// Gamma (the tables) are evaluated on the host.  dove_niqe_distance is host code: pooled covariance, Jacobi eigen-solve, pinv, sqrt.
#include "common.h"
#include "../../include/dove_hip.h"

#include <math.h>
#include <mutex>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int PAD = 3, TAPS = 2 * PAD + 1;    // 7 x 7 Gaussian window, sigma 7/6
constexpr int RG = 8;                         // row groups per block: a thread owns one column of BS / RG rows
constexpr int NGAM = 9801;                    // gam = 0.2, 0.201, ..., 10.000
constexpr int NMOM = 31;                      // per block: 5 products x {n<0, n>0, sum b^2 | b<0, sum b^2 | b>0, sum |b|, sum b^2}, mean sigma
constexpr int NFEAT = 36, NSTAT = 256, CHUNK = 64;

struct Gauss {                                // normalised 1-D Gaussian g[0..3] (g[6-i] = g[i])
  double g[4];
};

struct View {
  const void* data;
  int dtype;
  long long sn, sc, sh, sw;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// rounded luma (0..255) of a (BS+6)^2 region around block (bx, by) of frame n, indices clamped into the cropped image (replicate padding
// at the cropped edge; every load is inside the frame)
template <int DT, int LS, int NT>
__device__ __forceinline__ void stage_luma(const View& v, int C, long long base, int y0, int x0, int Hc, int Wc, const double* u8_scale,
                                           uint8_t* lum) {
  const long long sc = C == 3 ? v.sc : 0;                        // 1 channel: the three loads read the same element
  for (int e = threadIdx.x; e < LS * LS; e += NT) {
    const int ly = e / LS, lx = e - ly * LS;
    const int y = min(max(y0 + ly, 0), Hc - 1), x = min(max(x0 + lx, 0), Wc - 1);
    const long long o = base + (long long)y * v.sh + (long long)x * v.sw;
    double ch[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (DT == DOVE_U8) ch[c] = u8_scale[((const uint8_t*)v.data)[o + c * sc]];
      else if (DT == DOVE_BF16) ch[c] = (double)bf2f(((const bf16_t*)v.data)[o + c * sc]);
      else ch[c] = (double)((const float*)v.data)[o + c * sc];
    }
    const double l = C == 3 ? luma255(ch[0], ch[1], ch[2]) : rint(255.0 * ch[0]);
    lum[e] = (uint8_t)fmin(fmax(l, 0.0), 255.0);                 // values in [0,1] by contract; anything else saturates (NaN -> 0)
  }
}

// SCALE1: 96 x 96 blocks of the luma of `v` (also writes the block's 48 x 48 tile of i2_out); otherwise 48 x 48 blocks of i2_in.
// Hc x Wc: the image of this scale (whole blocks).  mom: [n][nby * nbx][NMOM].
template <bool SCALE1>
__global__ void __launch_bounds__((SCALE1 ? 96 : 48) * RG)
niqe_block_kernel(View v, const double* __restrict__ i2_in, int C, int Hc, int Wc, int nbx, int nby, Gauss gw, double* __restrict__ mom,
                  double* __restrict__ i2_out) {
  constexpr int BS = SCALE1 ? 96 : 48, LS = BS + 2 * PAD, NT = BS * RG, RPT = BS / RG, NW = NT / 64;
  using LT = std::conditional_t<SCALE1, uint8_t, double>;
  __shared__ LT lum[LS * LS];
  __shared__ double ms[BS * BS];
  __shared__ double red[NW][NMOM];
  __shared__ double u8_scale[SCALE1 ? 256 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = nbx * nby;
  const int n = blockIdx.x / B, blk = blockIdx.x - n * B;
  const int by = blk / nbx, bx = blk - by * nbx;

  if constexpr (SCALE1) {
    if (tid < 256) u8_scale[tid] = (double)tid / 255.0;
    __syncthreads();
    const long long base = (long long)n * v.sn;
    if (v.dtype == DOVE_U8) stage_luma<DOVE_U8, LS, NT>(v, C, base, by * BS - PAD, bx * BS - PAD, Hc, Wc, u8_scale, lum);
    else if (v.dtype == DOVE_BF16) stage_luma<DOVE_BF16, LS, NT>(v, C, base, by * BS - PAD, bx * BS - PAD, Hc, Wc, u8_scale, lum);
    else stage_luma<DOVE_F32, LS, NT>(v, C, base, by * BS - PAD, bx * BS - PAD, Hc, Wc, u8_scale, lum);
  } else {
    const double* src = i2_in + (long long)n * Hc * Wc;
    for (int e = tid; e < LS * LS; e += NT) {
      const int ly = e / LS, lx = e - ly * LS;
      const int y = min(max(by * BS - PAD + ly, 0), Hc - 1), x = min(max(bx * BS - PAD + lx, 0), Wc - 1);
      lum[e] = src[(long long)y * Wc + x];
    }
  }
  __syncthreads();

  // ---- half scale: I2 = 255 imresize(I / 255, 0.5), the 8-tap filter [-3 -9 29 111 111 29 -9 -3] / 256 at source 2i-3 .. 2i+4, symmetric
  // reflection at the cropped edge.  Integer taps on integer luma: the 2-D sum is exact in int32 (|sum| <= 255 * 304^2) and / 65536 is exact.
  if constexpr (SCALE1) {
    constexpr int HB = BS / 2;
    const int H2 = Hc / 2, W2 = Wc / 2;
    const int T[8] = {-3, -9, 29, 111, 111, 29, -9, -3};
    for (int e = tid; e < HB * HB; e += NT) {
      const int oy = e / HB, ox = e - oy * HB;
      const int gy = by * HB + oy, gx = bx * HB + ox;
      int lx[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        int sx = 2 * gx - 3 + k;
        sx = sx < 0 ? -1 - sx : (sx >= Wc ? 2 * Wc - 1 - sx : sx);
        lx[k] = min(max(sx - bx * BS + PAD, 0), LS - 1);         // in the halo by construction; the clamp costs nothing
      }
      int acc = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        int sy = 2 * gy - 3 + r;
        sy = sy < 0 ? -1 - sy : (sy >= Hc ? 2 * Hc - 1 - sy : sy);
        const LT* row = lum + min(max(sy - by * BS + PAD, 0), LS - 1) * LS;
        int h = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) h += T[k] * (int)row[lx[k]];
        acc += T[r] * h;
      }
      i2_out[((long long)n * H2 + gy) * W2 + gx] = (double)acc / 65536.0;
    }
  }

  // ---- local mean and deviation: horizontal 7-tap pass per input row from LDS, vertical pass accumulated in registers; MSCN into LDS ----
  // Both moments are taken of I - c, c the output pixel itself: d = g * (I - c) = mu - I and sigma^2 = g * (I - c)^2 - d^2, which is the
  // definition's E[I^2] - mu^2 without its cancellation.  A flat window gives exactly d = 0 and sigma = 0 (with the plain form the rounding
  // of sum g_k c leaves +-1 ulp for about half of the grey levels, and a flat region then counts as all-negative or all-positive).
  // Separably: with a = I[r][x+k] - I[r][x] and b = I[r][x] - c, sum_k g_k (a + b)^j splits into the row's shared h1 = sum g_k a,
  // h2 = sum g_k a^2 and the per-output b (sum_k g_k = 1): g * (I - c) = sum_r g_r (h1 + b), g * (I - c)^2 = sum_r g_r (h2 + b (2 h1 + b)).
  const int g = tid / BS, x = tid - g * BS, r0 = g * RPT;
  const double G[TAPS] = {gw.g[0], gw.g[1], gw.g[2], gw.g[3], gw.g[2], gw.g[1], gw.g[0]};
  LT cen[RPT + 2 * PAD];                                         // the thread's column of the halo tile
#pragma unroll
  for (int j = 0; j < RPT + 2 * PAD; ++j) cen[j] = lum[(r0 + j) * LS + x + PAD];
  double acc[RPT][2];
#pragma unroll
  for (int i = 0; i < RPT; ++i) acc[i][0] = acc[i][1] = 0.0;
#pragma unroll
  for (int rr = 0; rr < RPT + 2 * PAD; ++rr) {
    const LT* row = lum + (r0 + rr) * LS + x;
    const double c = (double)cen[rr];
    double t[TAPS];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) t[k] = (double)row[k] - c;    // integer differences at scale 1: exact, and so are their squares
    double h1 = 0.0, h2 = 0.0;
#pragma unroll
    for (int k = 0; k < PAD; ++k) {
      h1 = fma(G[k], t[k] + t[TAPS - 1 - k], h1);
      h2 = fma(G[k], t[k] * t[k] + t[TAPS - 1 - k] * t[TAPS - 1 - k], h2);
    }
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
      const int i = rr - k;                                      // input row r0+rr is tap k of output row r0+i
      if (i >= 0 && i < RPT) {
        const double b = c - (double)cen[i + PAD];
        acc[i][0] = fma(G[k], h1 + b, acc[i][0]);
        acc[i][1] = fma(G[k], h2 + b * (2.0 * h1 + b), acc[i][1]);
      }
    }
  }
  double part[NMOM];
#pragma unroll
  for (int j = 0; j < NMOM; ++j) part[j] = 0.0;
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const double d = acc[i][0];                                  // mu - I
    const double sg = sqrt(fabs(acc[i][1] - d * d));
    ms[(r0 + i) * BS + x] = (0.0 - d) / (sg + 1.0);
    part[NMOM - 1] += sg;
  }
  __syncthreads();

  // ---- moments of m and of m * roll(m, shift), shifts (0,1), (1,0), (1,1), (1,-1) over (row, col), circular inside the block ----
  const int xm = x == 0 ? BS - 1 : x - 1, xp = x == BS - 1 ? 0 : x + 1;
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int r = r0 + i, rm = r == 0 ? BS - 1 : r - 1;
    const double m = ms[r * BS + x];
    const double b[5] = {m, m * ms[r * BS + xm], m * ms[rm * BS + x], m * ms[rm * BS + xm], m * ms[rm * BS + xp]};
#pragma unroll
    for (int p = 0; p < 5; ++p) {
      const double bb = b[p] * b[p];
      const bool neg = b[p] < 0.0, pos = b[p] > 0.0;
      part[p * 6 + 0] += neg ? 1.0 : 0.0;
      part[p * 6 + 1] += pos ? 1.0 : 0.0;
      part[p * 6 + 2] += neg ? bb : 0.0;
      part[p * 6 + 3] += pos ? bb : 0.0;
      part[p * 6 + 4] += fabs(b[p]);
      part[p * 6 + 5] += bb;
    }
  }

  // ---- workgroup sums in a fixed order: lanes (butterfly), then waves 0..NW-1 ----
#pragma unroll
  for (int j = 0; j < NMOM; ++j) {
    const double s = wave_sum(part[j]);
    if (lane == 0) red[wave][j] = s;
  }
  __syncthreads();
  if (tid < NMOM) {
    double s = 0.0;
    for (int w = 0; w < NW; ++w) s += red[w][tid];
    mom[((long long)n * B + blk) * NMOM + tid] = tid == NMOM - 1 ? s / (double)(BS * BS) : s;
  }
}

// tab: [4][NGAM] = r(gam), gam, sqrt(Gamma(1/gam) / Gamma(3/gam)), Gamma(2/gam) / Gamma(1/gam).  One thread per (frame, block, scale, product).
__global__ void __launch_bounds__(256) niqe_solve_kernel(const double* __restrict__ mom1, const double* __restrict__ mom2,
                                                         const double* __restrict__ tab, long long blocks_total,
                                                         double* __restrict__ features, double* __restrict__ sharpness) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= blocks_total * 10) return;
  const long long blk = t / 10;
  const int sp = (int)(t - blk * 10), scale = sp / 5, p = sp - scale * 5;
  const double* m = (scale ? mom2 : mom1) + blk * NMOM + p * 6;
  const double count = scale ? 48.0 * 48.0 : 96.0 * 96.0;
  const double left = sqrt(m[2] / m[0]), right = sqrt(m[3] / m[1]);          // an empty sign set: 0 / 0 = NaN
  const double gh = left / right;
  const double ma = m[4] / count;
  const double rhat = (ma * ma) / (m[5] / count);
  const double gh2 = gh * gh;
  const double R = (rhat * (gh2 * gh + 1.0) * (gh + 1.0)) / ((gh2 + 1.0) * (gh2 + 1.0));
  const double* r = tab;
  const double nan = __builtin_nan("");
  double alpha = nan, c1 = nan, c2 = nan;
  if (R == R) {                                                  // a NaN R leaves every feature of the product NaN
    // first-index argmin of (r_k - R)^2 over the strictly increasing r: the neighbours of R, the lower one on a tie
    int lo = 0, hi = NGAM - 1;                                   // invariant: r[lo] <= R or lo == 0; r[hi] > R or hi == NGAM - 1
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (r[mid] <= R) lo = mid; else hi = mid;
    }
    const double d0 = (r[lo] - R) * (r[lo] - R), d1 = (r[hi] - R) * (r[hi] - R);
    const int k = d1 < d0 ? hi : lo;
    alpha = tab[NGAM + k];
    c1 = tab[2 * NGAM + k];
    c2 = tab[3 * NGAM + k];
  }
  const double bl = left * c1, br = right * c1;
  double* f = features + blk * NFEAT + scale * 18;
  if (p == 0) {
    f[0] = alpha;
    f[1] = (bl + br) / 2.0;
    if (scale == 0 && sharpness) sharpness[blk] = mom1[blk * NMOM + NMOM - 1];
  } else {
    f += 2 + (p - 1) * 4;
    f[0] = alpha;
    f[1] = (br - bl) * c2;
    f[2] = bl;
    f[3] = br;
  }
}

// one workgroup per frame.  features [n][B][36] -> mu[36] (nanmean per column), cov[36][36] (divisor n-1 over the blocks without a NaN,
// around their own mean), counts {blocks without a NaN, blocks with at least one non-NaN feature}.  Blocks are summed in index order.
__global__ void __launch_bounds__(NSTAT) niqe_stats_kernel(const double* __restrict__ features, int B, double* __restrict__ mu,
                                                           double* __restrict__ cov, int* __restrict__ counts) {
  __shared__ double f[CHUNK][NFEAT + 1];
  __shared__ int clean[CHUNK], some[CHUNK];
  __shared__ double cmean[NFEAT];
  __shared__ int nclean_s;
  const int n = blockIdx.x, tid = threadIdx.x;
  const double* src = features + (long long)n * B * NFEAT;
  auto load_chunk = [&](int b0) {
    const int nb = min(CHUNK, B - b0);
    __syncthreads();                                             // the previous chunk has been consumed
    for (int e = tid; e < nb * NFEAT; e += NSTAT) f[e / NFEAT][e % NFEAT] = src[(long long)b0 * NFEAT + e];
    __syncthreads();
    if (tid < nb) {
      int nans = 0;
      for (int c = 0; c < NFEAT; ++c) nans += f[tid][c] != f[tid][c];
      clean[tid] = nans == 0;
      some[tid] = nans < NFEAT;
    }
    __syncthreads();
    return nb;
  };
  // pass 1: the column sums
  double ns = 0.0, cs = 0.0;
  int nc = 0, ncl = 0, nso = 0;
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int nb = load_chunk(b0);
    if (tid < NFEAT) {
      for (int b = 0; b < nb; ++b) {
        const double val = f[b][tid];
        if (val == val) { ns += val; ++nc; }
        if (clean[b]) cs += val;
      }
    } else if (tid == NFEAT) {
      for (int b = 0; b < nb; ++b) { ncl += clean[b]; nso += some[b]; }
    }
  }
  if (tid < NFEAT) mu[n * NFEAT + tid] = ns / (double)nc;        // no value in the column: 0 / 0 = NaN
  if (tid == NFEAT) {
    nclean_s = ncl;
    counts[2 * n] = ncl;
    counts[2 * n + 1] = nso;
  }
  __syncthreads();
  const int nclean = nclean_s;
  if (tid < NFEAT) cmean[tid] = cs / (double)nclean;
  // pass 2: the covariance around the mean of the NaN-free blocks
  constexpr int PER = (NFEAT * NFEAT + NSTAT - 1) / NSTAT;
  double a[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) a[q] = 0.0;
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int nb = load_chunk(b0);                               // its barriers also publish cmean
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = tid + q * NSTAT;
      if (e < NFEAT * NFEAT) {
        const int i = e / NFEAT, j = e - i * NFEAT;
        const double mi = cmean[i], mj = cmean[j];
        for (int b = 0; b < nb; ++b)
          if (clean[b]) a[q] += (f[b][i] - mi) * (f[b][j] - mj);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int e = tid + q * NSTAT;
    if (e < NFEAT * NFEAT) cov[(long long)n * NFEAT * NFEAT + e] = nclean >= 2 ? a[q] / (double)(nclean - 1) : __builtin_nan("");
  }
}

// the device-resident tables, built once per device on the host (lgamma) and kept for the life of the process
std::mutex g_tab_mutex;
double* g_tab[64] = {};

int gamma_tables(const double** out) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    dove_set_error("niqe: no usable HIP device");
    return DOVE_ELAUNCH;
  }
  std::lock_guard<std::mutex> lock(g_tab_mutex);
  if (!g_tab[dev]) {
    std::vector<double> h(4 * (size_t)NGAM);
    for (int k = 0; k < NGAM; ++k) {
      const double gam = 0.2 + 0.001 * (double)k;                // numpy.arange(0.2, 10.001, 0.001)[k]
      const double l1 = lgamma(1.0 / gam), l2 = lgamma(2.0 / gam), l3 = lgamma(3.0 / gam);
      h[k] = exp(2.0 * l2 - l1 - l3);
      h[NGAM + k] = gam;
      h[2 * NGAM + k] = sqrt(exp(l1 - l3));
      h[3 * NGAM + k] = exp(l2 - l1);
    }
    double* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, h.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      if (d) (void)hipFree(d);
      dove_set_error("niqe: gamma tables: %s", hipGetErrorString(e));
      return DOVE_ELAUNCH;
    }
    g_tab[dev] = d;
  }
  *out = g_tab[dev];
  return DOVE_OK;
}

// eigenvalues and eigenvectors (columns of v) of the symmetric a (destroyed), cyclic Jacobi
void jacobi_eig(double (&a)[NFEAT][NFEAT], double (&v)[NFEAT][NFEAT], double (&w)[NFEAT]) {
  constexpr int N = NFEAT;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < N; ++p)
      for (int q = p + 1; q < N; ++q) off += a[p][q] * a[p][q];
    if (off == 0.0) break;
    for (int p = 0; p < N; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double g = 100.0 * fabs(apq);
        if (sweep > 3 && fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
          a[p][q] = a[q][p] = 0.0;                               // below the rounding of both diagonal entries
          continue;
        }
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; ++k) {                            // A <- A J
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {                            // A <- J^T A
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
        a[p][q] = a[q][p] = 0.0;
        for (int k = 0; k < N; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < N; ++i) w[i] = a[i][i];
}

}  // namespace

static long long niqe_blocks(int h, int w) { return (long long)(h / 96) * (w / 96); }

extern "C" size_t dove_niqe_workspace_bytes(int n, int h, int w) {
  if (n <= 0 || h < 96 || w < 96) return 0;
  const long long B = niqe_blocks(h, w);
  return (size_t)n * (size_t)(B * 2 * NMOM + B * 48 * 48) * sizeof(double);    // the moments of both scales, I2
}

extern "C" int dove_niqe_features(const dove_image_view* img, int n, int channels, int h, int w, void* ws, size_t ws_bytes, double* features,
                                  double* sharpness, void* stream) {
  // argument checks first, the null-pointer check last: a call that is wrong in any way never reaches a launch
  DOVE_CHECK_ARG(img, "niqe_features: null view");
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0, "niqe_features: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(channels == 1 || channels == 3, "niqe_features: channels must be 1 or 3, got %d", channels);
  DOVE_CHECK_ARG(h >= 96 && w >= 96, "niqe_features: NIQE needs H and W >= 96 (one 96 x 96 block), got %d x %d", h, w);
  DOVE_CHECK_ARG(img->dtype >= DOVE_F32 && img->dtype <= DOVE_U8, "niqe_features: bad dtype %d (0 f32, 1 bf16, 2 u8)", img->dtype);
  const size_t need = dove_niqe_workspace_bytes(n, h, w);
  DOVE_CHECK_ARG(ws_bytes >= need, "niqe_features: workspace of %zu bytes is too small, need %zu (dove_niqe_workspace_bytes)", ws_bytes, need);
  const int nby = h / 96, nbx = w / 96;
  const long long B = (long long)nby * nbx, total = (long long)n * B;
  DOVE_CHECK_ARG(total * 10 < (1LL << 31), "niqe_features: %lld blocks exceed one launch", total);
  DOVE_CHECK_ARG(img->data && ws && features, "niqe_features: null pointer");
  const double* tab = nullptr;
  if (int rc = gamma_tables(&tab)) return rc;
  Gauss gw;
  double e[TAPS], sum = 0.0;
  const double sigma = 7.0 / 6.0;
  for (int i = 0; i < TAPS; ++i) sum += e[i] = exp(-(double)((i - PAD) * (i - PAD)) / (2.0 * sigma * sigma));
  for (int i = 0; i <= PAD; ++i) gw.g[i] = e[i] / sum;
  double* mom1 = (double*)ws;
  double* mom2 = mom1 + total * NMOM;
  double* i2 = mom2 + total * NMOM;
  const View v{img->data, img->dtype, img->sn, img->sc, img->sh, img->sw};
  const int Hc = nby * 96, Wc = nbx * 96;                        // crop to whole blocks before any filtering
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(niqe_block_kernel<true>, dim3((unsigned)total), dim3(96 * RG), 0, st, v, (const double*)nullptr, channels, Hc, Wc, nbx,
                     nby, gw, mom1, i2);
  DOVE_CHECK_LAUNCH("dove_niqe_features (scale 1)");
  hipLaunchKernelGGL(niqe_block_kernel<false>, dim3((unsigned)total), dim3(48 * RG), 0, st, v, (const double*)i2, channels, Hc / 2, Wc / 2,
                     nbx, nby, gw, mom2, (double*)nullptr);
  DOVE_CHECK_LAUNCH("dove_niqe_features (scale 2)");
  hipLaunchKernelGGL(niqe_solve_kernel, dim3((unsigned)((total * 10 + 255) / 256)), dim3(256), 0, st, (const double*)mom1,
                     (const double*)mom2, tab, total, features, sharpness);
  DOVE_CHECK_LAUNCH("dove_niqe_features (solve)");
  return DOVE_OK;
}

extern "C" int dove_niqe_stats(const double* features, int n, int blocks, double* mu, double* cov, int* counts, void* stream) {
  DOVE_CHECK_ARG(n > 0 && blocks > 0, "niqe_stats: bad shape n=%d blocks=%d", n, blocks);
  DOVE_CHECK_ARG(features && mu && cov && counts, "niqe_stats: null pointer");
  hipLaunchKernelGGL(niqe_stats_kernel, dim3((unsigned)n), dim3(NSTAT), 0, (hipStream_t)stream, features, blocks, mu, cov, counts);
  DOVE_CHECK_LAUNCH("dove_niqe_stats");
  return DOVE_OK;
}

extern "C" int dove_niqe_distance(const double* mu_a, const double* cov_a, const double* mu_b, const double* cov_b, double* out) {
  DOVE_CHECK_ARG(mu_a && cov_a && mu_b && cov_b && out, "niqe_distance: null pointer");
  constexpr int N = NFEAT;
  static thread_local double a[N][N], v[N][N];
  double w[N], d[N];
  bool finite = true;
  for (int i = 0; i < N; ++i) {
    d[i] = mu_a[i] - mu_b[i];
    finite = finite && isfinite(d[i]);
    for (int j = 0; j < N; ++j) {
      // the pooled covariance, symmetrised (a covariance is symmetric up to the rounding of whoever computed it)
      a[i][j] = ((cov_a[i * N + j] + cov_b[i * N + j]) / 2.0 + (cov_a[j * N + i] + cov_b[j * N + i]) / 2.0) / 2.0;
      finite = finite && isfinite(a[i][j]);
    }
  }
  if (!finite) {                                                 // fewer than two NaN-free blocks, an empty column: the score is NaN
    *out = __builtin_nan("");
    return DOVE_OK;
  }
  jacobi_eig(a, v, w);
  double smax = 0.0;
  for (int i = 0; i < N; ++i) smax = fmax(smax, fabs(w[i]));
  const double cut = (double)N * 2.220446049250313e-16 * smax;   // pinv: singular values (|eigenvalues|) at or below 36 eps sigma_max are dropped
  double q = 0.0;
  for (int k = 0; k < N; ++k) {
    if (!(fabs(w[k]) > cut)) continue;
    double proj = 0.0;
    for (int i = 0; i < N; ++i) proj += v[i][k] * d[i];
    q += proj * proj / w[k];
  }
  *out = sqrt(q);
  return DOVE_OK;
}
