// Degradation synthesis: the operators that turn ground-truth frames into a low-quality clip (include/dove_hip.h has the
// contract, tests/degrade_ref.py the definitions in numpy).  Frames are fp32 [n][h][w][3] in the 0..255 scale.
//
// blur2d: one 256-thread block owns a 64 x 32 tile of one frame.  The tile and its k/2 halo (reflect-101 comes with the load) sit in LDS as
//   [32 + k - 1][64 + k - 1][3] floats (52 KB at k = 21) next to the k x k weights.  A thread owns one column and 8 consecutive rows: a tile
//   value is read once per (row, dx) and feeds up to 8 outputs x 3 channels, so the LDS traffic is (3 + 8) reads per 24 FMAs instead of one
//   per FMA.  Lanes of a wave read pixels 12 bytes apart (3 is coprime to the 64 banks).  Every output sums its taps in row-major order with
//   fp32 FMAs, whatever the tile it falls in: the bits do not depend on the launch geometry.
// resize: one thread per output pixel, three channels.  Source positions are integer quotients and remainders of ((2 i + 1) h - oh) / (2 oh);
//   the fraction is one fp32 division of two exact integers.
// noise: one thread per Philox block (Gaussian: 4 elements) or per element (Poisson).  The Poisson pass first marks the values present in
//   each frame in a 256-flag table (LDS per block, then plain stores of 1), the second pass counts the flags and samples.
// jpeg: kernel 1 runs one 16 x 16 MCU per block - colour conversion, 2x2 chroma mean, and for each of the six 8x8 blocks two integer
//   matrix passes each way through LDS with quantisation in between - and leaves the decoded Y, Cb, Cr planes in the workspace; kernel 2
//   does the fancy chroma upsampling, which reads across MCU borders, and the conversion back to RGB.
#include "common.h"
#include "philox.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = 64;                 // frames per launch: their per-frame parameters travel as a kernel argument
constexpr int BT_W = 64, BT_H = 32, BR = 8;

struct FrameF { float v[CHUNK]; };
struct FrameI { int v[CHUNK]; };

// ---------------------------------------------------------------- blur ----------------------------------------------------------------
__device__ __forceinline__ int reflect101(int p, int n) {
  if (p < 0) p = -p;
  if (p >= n) p = 2 * n - 2 - p;
  return min(max(p, 0), n - 1);           // only positions whose outputs are never stored need the clamp
}

__global__ __launch_bounds__(NT) void blur_kernel(const float* __restrict__ x, const float* __restrict__ kern, int per_frame, int k, int H,
                                                  int W, int tiles_x, int tiles_y, float* __restrict__ out) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, r = k >> 1, tw = BT_W + k - 1, th = BT_H + k - 1;
  float* tile = lds;
  float* wl = lds + th * tw * 3;
  const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y;
  const long long fr = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = bx * BT_W, y0 = by * BT_H;
  const float* xf = x + fr * H * W * 3;
  const float* kf = kern + (per_frame ? fr * k * k : 0);
  for (int i = tid; i < k * k; i += NT) wl[i] = kf[i];
  for (int i = tid; i < th * tw * 3; i += NT) {
    const int p = i / 3, c = i - p * 3, ty = p / tw, tx = p - ty * tw;
    const int gy = reflect101(y0 + ty - r, H), gx = reflect101(x0 + tx - r, W);
    tile[i] = xf[((long long)gy * W + gx) * 3 + c];
  }
  __syncthreads();
  const int lx = tid & 63, ly = (tid >> 6) * BR;     // (row, dy) below are the same for a whole wave
  float acc[BR][3];
#pragma unroll
  for (int j = 0; j < BR; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.f;
  for (int rr = 0; rr < k + BR - 1; ++rr) {
    const float* row = tile + ((ly + rr) * tw + lx) * 3;
    for (int dx = 0; dx < k; ++dx) {
      const float v0 = row[dx * 3], v1 = row[dx * 3 + 1], v2 = row[dx * 3 + 2];
#pragma unroll
      for (int j = 0; j < BR; ++j) {
        const int dy = rr - j;
        if (dy >= 0 && dy < k) {
          const float wv = wl[dy * k + dx];
          acc[j][0] = fmaf(wv, v0, acc[j][0]);
          acc[j][1] = fmaf(wv, v1, acc[j][1]);
          acc[j][2] = fmaf(wv, v2, acc[j][2]);
        }
      }
    }
  }
  const int gx = x0 + lx;
  if (gx >= W) return;
  float* of = out + fr * H * W * 3;
#pragma unroll
  for (int j = 0; j < BR; ++j) {
    const int gy = y0 + ly + j;
    if (gy >= H) break;
    float* o = of + ((long long)gy * W + gx) * 3;
    o[0] = acc[j][0];
    o[1] = acc[j][1];
    o[2] = acc[j][2];
  }
}

// --------------------------------------------------------------- resize ---------------------------------------------------------------
// half-pixel source position of output i: floor and fraction of ((2 i + 1) n - on) / (2 on), from integers
__device__ __forceinline__ void src_pos(int i, int n, int on, int* i0, float* f) {
  const long long num = (2LL * i + 1) * n - on, den = 2LL * on;
  long long q = num / den, rem = num - q * den;
  if (rem < 0) {
    rem += den;
    --q;
  }
  *i0 = (int)q;
  *f = (float)rem / (float)den;
}

// Keys' cubic, A = -0.75, at distances 1 + t, t, 1 - t, 2 - t: the outer pair in factored form A t (1 - t)^2
__device__ __forceinline__ void cubic_weights(float t, float* w) {
  const float A = -0.75f, u = 1.0f - t;
  w[0] = A * t * u * u;
  w[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  w[2] = ((A + 2.0f) * u - (A + 3.0f)) * u * u + 1.0f;
  w[3] = A * u * t * t;
}

template <int MODE>
__global__ __launch_bounds__(NT) void resize_kernel(const float* __restrict__ x, int H, int W, int OH, int OW, long long total,
                                                    float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  const int ox = (int)(t % OW), oy = (int)((t / OW) % OH);
  const long long fr = t / ((long long)OW * OH);
  const float* xf = x + fr * H * W * 3;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  if (MODE == DOVE_RESIZE_AREA) {
    // in units of 1 / OH the output span is [oy H, (oy + 1) H) and source row s covers [s OH, (s + 1) OH): overlaps are integers
    const long long ys = (long long)oy * H, ye = ys + H, xs = (long long)ox * W, xe = xs + W;
    const int sy0 = (int)(ys / OH), sy1 = (int)((ye + OH - 1) / OH), sx0 = (int)(xs / OW), sx1 = (int)((xe + OW - 1) / OW);
    for (int sy = sy0; sy < sy1; ++sy) {
      const long long oly = min(ye, (long long)(sy + 1) * OH) - max(ys, (long long)sy * OH);
      const float wy = (float)oly / (float)H;
      float r0 = 0.f, r1 = 0.f, r2 = 0.f;
      for (int sx = sx0; sx < sx1; ++sx) {
        const long long olx = min(xe, (long long)(sx + 1) * OW) - max(xs, (long long)sx * OW);
        const float wx = (float)olx / (float)W;
        const float* p = xf + ((long long)sy * W + sx) * 3;
        r0 = fmaf(wx, p[0], r0);
        r1 = fmaf(wx, p[1], r1);
        r2 = fmaf(wx, p[2], r2);
      }
      a0 = fmaf(wy, r0, a0);
      a1 = fmaf(wy, r1, a1);
      a2 = fmaf(wy, r2, a2);
    }
  } else {
    constexpr int T = MODE == DOVE_RESIZE_BICUBIC ? 4 : 2;
    int iy, ix;
    float fy, fx, wy[T], wx[T];
    src_pos(oy, H, OH, &iy, &fy);
    src_pos(ox, W, OW, &ix, &fx);
    if constexpr (MODE == DOVE_RESIZE_BICUBIC) {
      cubic_weights(fy, wy);
      cubic_weights(fx, wx);
      --iy;
      --ix;
    } else {
      wy[0] = 1.0f - fy, wy[1] = fy;
      wx[0] = 1.0f - fx, wx[1] = fx;
    }
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const int sy = min(max(iy + j, 0), H - 1);
      float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
      for (int i = 0; i < T; ++i) {
        const int sx = min(max(ix + i, 0), W - 1);
        const float* p = xf + ((long long)sy * W + sx) * 3;
        r0 = fmaf(wx[i], p[0], r0);
        r1 = fmaf(wx[i], p[1], r1);
        r2 = fmaf(wx[i], p[2], r2);
      }
      a0 = fmaf(wy[j], r0, a0);
      a1 = fmaf(wy[j], r1, a1);
      a2 = fmaf(wy[j], r2, a2);
    }
  }
  float* o = out + t * 3;
  o[0] = a0;
  o[1] = a1;
  o[2] = a2;
}

// ----------------------------------------------------------- Gaussian noise -----------------------------------------------------------
// One thread per Philox block of the stream.  e0 = stream index of the launch's first element, per = elements per frame (h w 3, gray: h w).
template <bool GRAY>
__global__ __launch_bounds__(NT) void gaussian_kernel(const float* __restrict__ x, FrameF sigma, unsigned long long seed,
                                                      unsigned long long stream_id, unsigned long long e0, long long count, long long per,
                                                      long long nblocks, float* __restrict__ out) {
  const unsigned long long first = e0 >> 2;
  for (long long j = (long long)blockIdx.x * NT + threadIdx.x; j < nblocks; j += (long long)gridDim.x * NT) {
    const unsigned long long b = first + (unsigned long long)j;
    const Words wd = philox4x32_10(b, stream_id, seed);
    float z[4];
    box_muller(wd.x[0], wd.x[1], &z[0], &z[1]);
    box_muller(wd.x[2], wd.x[3], &z[2], &z[3]);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const long long e = (long long)(b * 4 + l - e0);       // index inside the launch
      if (e < 0 || e >= count) continue;
      const float nz = sigma.v[e / per] * z[l];
      if (GRAY) {
        out[e * 3] = x[e * 3] + nz;
        out[e * 3 + 1] = x[e * 3 + 1] + nz;
        out[e * 3 + 2] = x[e * 3 + 2] + nz;
      } else {
        out[e] = x[e] + nz;
      }
    }
  }
}

// ------------------------------------------------------------ Poisson noise ------------------------------------------------------------
// the 8-bit value whose Poisson rate an element draws: colour - of the element; gray - of the pixel's fp32 luma (products and sums rounded
// one by one, left to right, so that numpy's float32 arithmetic gives the same value)
template <bool GRAY>
__device__ __forceinline__ int poisson_value(const float* __restrict__ xf, long long e) {
  float v;
  if (GRAY) v = __fadd_rn(__fadd_rn(__fmul_rn(0.299f, xf[e * 3]), __fmul_rn(0.587f, xf[e * 3 + 1])), __fmul_rn(0.114f, xf[e * 3 + 2]));
  else v = xf[e];
  return (int)fminf(fmaxf(rintf(v), 0.f), 255.f);
}

template <bool GRAY>
__global__ __launch_bounds__(NT) void poisson_presence_kernel(const float* __restrict__ x, long long per, int* __restrict__ flags) {
  __shared__ int present[256];
  present[threadIdx.x] = 0;
  __syncthreads();
  const float* xf = x + (long long)blockIdx.y * per * (GRAY ? 3 : 1);
  for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < per; e += (long long)gridDim.x * NT) present[poisson_value<GRAY>(xf, e)] = 1;
  __syncthreads();
  if (present[threadIdx.x]) flags[blockIdx.y * 256 + threadIdx.x] = 1;
}

__device__ __forceinline__ double uniform52(uint32_t hi, uint32_t lo) {       // (m + 1/2) 2^-52, m = 52 bits: inside (0, 1), exact
  const unsigned long long m = ((unsigned long long)hi << 20) | (lo >> 12);
  return ((double)m + 0.5) * 2.220446049250313e-16;
}

// Poisson(lam), lam an integer 0..65280.  Below 10: inversion by sequential search on one uniform.  From 10: Hoermann's transformed rejection
// with squeeze (PTRS, 1993), one Philox block per round.  fp64 throughout.
__device__ __forceinline__ int poisson_sample(int lam_i, unsigned long long e, unsigned long long stream_id, unsigned long long seed) {
  if (lam_i == 0) return 0;
  const double lam = (double)lam_i;
  if (lam_i < 10) {
    const Words wd = philox4x32_10(e, stream_id, seed);
    const double u = uniform52(wd.x[0], wd.x[1]);
    double p = exp(-lam), s = p;
    int k = 0;
    while (u > s && k < 200) {            // the mass beyond 200 at rate < 10 is below 10^-200: the cap only bounds the loop
      ++k;
      p *= lam / k;
      s += p;
    }
    return k;
  }
  const double slam = sqrt(lam), loglam = log(lam), b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
  for (unsigned long long round = 0; round < 64; ++round) {       // a round accepts with probability > 0.8
    const Words wd = philox4x32_10(e, stream_id | (round << 32), seed);
    const double U = uniform52(wd.x[0], wd.x[1]) - 0.5, V = uniform52(wd.x[2], wd.x[3]);
    const double us = 0.5 - fabs(U);
    const double kf = floor((2.0 * a / us + b) * U + lam + 0.43);
    if (us >= 0.07 && V <= vr) return (int)kf;
    if (kf < 0.0 || (us < 0.013 && V > us)) continue;
    if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + kf * loglam - lgamma(kf + 1.0)) return (int)kf;
  }
  return lam_i;
}

template <bool GRAY>
__global__ __launch_bounds__(NT) void poisson_kernel(const float* __restrict__ x, FrameF scale, unsigned long long seed,
                                                     unsigned long long stream_id, unsigned long long e0, long long per,
                                                     const int* __restrict__ flags, float* __restrict__ out) {
  const int distinct = __syncthreads_count(flags[blockIdx.y * 256 + threadIdx.x] != 0);
  int U = 1;
  while (U < distinct) U <<= 1;
  const long long e = (long long)blockIdx.x * NT + threadIdx.x;
  if (e >= per) return;
  const long long base = (long long)blockIdx.y * per;
  const float* xf = x + base * (GRAY ? 3 : 1);
  float* of = out + base * (GRAY ? 3 : 1);
  const int v = poisson_value<GRAY>(xf, e);
  const int kk = poisson_sample(v * U, e0 + (unsigned long long)(base + e), stream_id, seed);
  const float nz = scale.v[blockIdx.y] * ((float)kk / (float)U - (float)v);
  if (GRAY) {
    of[e * 3] = xf[e * 3] + nz;
    of[e * 3 + 1] = xf[e * 3 + 1] + nz;
    of[e * 3 + 2] = xf[e * 3 + 2] + nz;
  } else {
    of[e] = xf[e] + nz;
  }
}

// ----------------------------------------------------------------- JPEG -----------------------------------------------------------------
// ITU-T T.81 Annex K, tables K.1 and K.2, in natural (row-major) order
__constant__ int JPEG_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// rint(4096 cos(m pi / 16)), m = 0..8; the DC row of the transform is rint(8192 / sqrt(8)) = 2896
__constant__ int JPEG_COS[9] = {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799, 0};

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// The 8x8 DCT as an integer matrix C[u][x] = rint(8192 s(u) cos((2 x + 1) u pi / 16)), s(0) = 1 / sqrt(8), s(u) = 1 / 2: forward C f C^T,
// inverse C^T F C.  Each way is two passes; the first keeps 2 fractional bits ((sum + 2^10) >> 11), the second result carries 2^15.
__global__ __launch_bounds__(NT) void jpeg_codec_kernel(const float* __restrict__ x, int H, int W, int mcus_x, FrameI quality,
                                                        uint8_t* __restrict__ ws, long long frame_ws) {
  __shared__ int qt[2][64], ct[8][8], ycc[3][256], blk[6][64], tmp[6][64];
  const int tid = threadIdx.x, fr = blockIdx.y;
  const int mcx = blockIdx.x % mcus_x, mcy = blockIdx.x / mcus_x;
  if (tid < 128) {
    const int q = quality.v[fr], s = q < 50 ? 5000 / q : 200 - 2 * q;
    qt[tid >> 6][tid & 63] = min(max((JPEG_BASE[tid >> 6][tid & 63] * s + 50) / 100, 1), 255);
  } else if (tid < 192) {
    const int u = (tid >> 3) & 7, xx = tid & 7;
    int m = ((2 * xx + 1) * u) & 31;
    if (m > 16) m = 32 - m;
    ct[u][xx] = u == 0 ? 2896 : (m > 8 ? -JPEG_COS[16 - m] : JPEG_COS[m]);
  }
  {
    const int px = tid & 15, py = tid >> 4;
    const int gx = min(mcx * 16 + px, W - 1), gy = min(mcy * 16 + py, H - 1);     // edge replication up to the whole MCU
    const float* p = x + (((long long)fr * H + gy) * W + gx) * 3;
    const int r = (int)fminf(fmaxf(p[0], 0.f), 255.f), g = (int)fminf(fmaxf(p[1], 0.f), 255.f), b = (int)fminf(fmaxf(p[2], 0.f), 255.f);
    const int yy = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    ycc[0][tid] = yy;
    ycc[1][tid] = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    ycc[2][tid] = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
    blk[(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = yy - 128;
  }
  __syncthreads();
  if (tid < 128) {
    const int comp = tid >> 6, i = tid & 63, cy = i >> 3, cx = i & 7;
    const int* c = ycc[1 + comp] + cy * 32 + cx * 2;
    blk[4 + comp][i] = ((c[0] + c[1] + c[16] + c[17] + 1 + (cx & 1)) >> 2) - 128;     // libjpeg's alternating bias
  }
  __syncthreads();
  for (int idx = tid; idx < 384; idx += NT) {          // forward, rows: t[y][u] = sum_x f[y][x] C[u][x]
    const int b = idx >> 6, y = (idx >> 3) & 7, u = idx & 7;
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += blk[b][y * 8 + i] * ct[u][i];
    tmp[b][y * 8 + u] = (s + 1024) >> 11;
  }
  __syncthreads();
  for (int idx = tid; idx < 384; idx += NT) {          // forward, columns: F[v][u] = sum_y t[y][u] C[v][y]; quantise, dequantise
    const int b = idx >> 6, v = (idx >> 3) & 7, u = idx & 7;
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += tmp[b][i * 8 + u] * ct[v][i];
    const int Q = qt[b >= 4][v * 8 + u], Qs = Q << 15;
    const int lev = ((s < 0 ? -s : s) + (Qs >> 1)) / Qs;        // round half away from zero
    blk[b][v * 8 + u] = (s < 0 ? -lev : lev) * Q;
  }
  __syncthreads();
  for (int idx = tid; idx < 384; idx += NT) {          // inverse, rows: t[v][x] = sum_u F[v][u] C[u][x]
    const int b = idx >> 6, v = (idx >> 3) & 7, xx = idx & 7;
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += blk[b][v * 8 + i] * ct[i][xx];
    tmp[b][v * 8 + xx] = (s + 1024) >> 11;
  }
  __syncthreads();
  uint8_t* wf = ws + (long long)fr * frame_ws;
  const int PW = mcus_x * 16, PH = gridDim.x / mcus_x * 16;
  for (int idx = tid; idx < 384; idx += NT) {          // inverse, columns: f[y][x] = sum_v t[v][x] C[v][y]
    const int b = idx >> 6, y = (idx >> 3) & 7, xx = idx & 7;
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += tmp[b][i * 8 + xx] * ct[i][y];
    const uint8_t val = (uint8_t)clamp255(((s + 16384) >> 15) + 128);
    if (b < 4) wf[(long long)(mcy * 16 + (b >> 1) * 8 + y) * PW + mcx * 16 + (b & 1) * 8 + xx] = val;
    else wf[(long long)PH * PW + (long long)(b - 4) * (PH / 2) * (PW / 2) + (long long)(mcy * 8 + y) * (PW / 2) + mcx * 8 + xx] = val;
  }
}

// libjpeg's h2v2 "fancy" upsampling: 3:1 towards the nearer chroma sample on each axis, the farther one clamped to the real chroma extent
// ceil(h / 2) x ceil(w / 2); (sum of 16ths + 8) >> 4 at even columns, + 7 at odd ones.  Then JFIF YCbCr -> RGB in 16-bit fixed point.
__global__ __launch_bounds__(NT) void jpeg_finish_kernel(const uint8_t* __restrict__ ws, long long frame_ws, int H, int W, int PH, int PW,
                                                         long long total, uint8_t* __restrict__ out) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  const int xx = (int)(t % W), y = (int)((t / W) % H);
  const long long fr = t / ((long long)W * H);
  const uint8_t* wf = ws + fr * frame_ws;
  const int CW = (W + 1) / 2, CHH = (H + 1) / 2, PCW = PW / 2;
  const int cy = y >> 1, cx = xx >> 1;
  const int oy = min(max((y & 1) ? cy + 1 : cy - 1, 0), CHH - 1), ox = min(max((xx & 1) ? cx + 1 : cx - 1, 0), CW - 1);
  const int yy = wf[(long long)y * PW + xx];
  int c[2];
#pragma unroll
  for (int comp = 0; comp < 2; ++comp) {
    const uint8_t* p = wf + (long long)PH * PW + (long long)comp * (PH / 2) * PCW;
    const int near = 3 * p[cy * PCW + cx] + p[oy * PCW + cx], far = 3 * p[cy * PCW + ox] + p[oy * PCW + ox];
    c[comp] = (3 * near + far + ((xx & 1) ? 7 : 8)) >> 4;
  }
  const int cb = c[0] - 128, cr = c[1] - 128;
  uint8_t* o = out + t * 3;
  o[0] = (uint8_t)clamp255(yy + ((91881 * cr + 32768) >> 16));
  o[1] = (uint8_t)clamp255(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  o[2] = (uint8_t)clamp255(yy + ((116130 * cb + 32768) >> 16));
}

bool good_shape(int n, int h, int w) { return n > 0 && h > 0 && w > 0 && (long long)h * w <= (1LL << 28); }   // plane offsets stay in 32 bits

long long jpeg_frame_ws(int h, int w) {
  const long long ph = ((long long)h + 15) / 16 * 16, pw = ((long long)w + 15) / 16 * 16;
  return ph * pw * 3 / 2;
}

}  // namespace

extern "C" int dove_blur2d_f32(const float* x, int n, int h, int w, const float* kernel, int k, int per_frame, float* out, void* stream) {
  DOVE_CHECK_ARG(good_shape(n, h, w), "blur2d: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(k >= 3 && k <= 21 && (k & 1), "blur2d: kernel size %d is not odd in 3..21", k);
  DOVE_CHECK_ARG(h > k / 2 && w > k / 2, "blur2d: a %d x %d frame is too small for reflect-101 borders of a %d x %d kernel (needs more than %d)",
                 h, w, k, k, k / 2);
  DOVE_CHECK_ARG(x && kernel && out, "blur2d: null pointer");
  DOVE_CHECK_ARG(x != out, "blur2d: out must not alias x");
  const int tiles_x = (w + BT_W - 1) / BT_W, tiles_y = (h + BT_H - 1) / BT_H;
  const long long blocks = (long long)n * tiles_x * tiles_y;
  DOVE_CHECK_ARG(blocks < (1LL << 31), "blur2d: n=%d frames of %d x %d exceed one launch", n, h, w);
  const size_t lds = ((size_t)(BT_H + k - 1) * (BT_W + k - 1) * 3 + (size_t)k * k) * sizeof(float);
  hipLaunchKernelGGL(blur_kernel, dim3((unsigned)blocks), dim3(NT), lds, (hipStream_t)stream, x, kernel, per_frame != 0, k, h, w, tiles_x, tiles_y,
                     out);
  DOVE_CHECK_LAUNCH("dove_blur2d_f32");
  return DOVE_OK;
}

extern "C" int dove_resize_f32(const float* x, int n, int h, int w, int oh, int ow, int mode, float* out, void* stream) {
  DOVE_CHECK_ARG(good_shape(n, h, w) && good_shape(n, oh, ow), "resize: bad shape n=%d %d x %d -> %d x %d", n, h, w, oh, ow);
  DOVE_CHECK_ARG(mode == DOVE_RESIZE_BILINEAR || mode == DOVE_RESIZE_BICUBIC || mode == DOVE_RESIZE_AREA,
                 "resize: bad mode %d (0 bilinear, 1 bicubic, 2 area)", mode);
  DOVE_CHECK_ARG(x && out, "resize: null pointer");
  DOVE_CHECK_ARG(x != out, "resize: out must not alias x");
  hipStream_t st = (hipStream_t)stream;
  if (oh == h && ow == w) {
    const hipError_t e = hipMemcpyAsync(out, x, (size_t)n * h * w * 3 * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      dove_set_error("dove_resize_f32: copy failed: %s", hipGetErrorString(e));
      return DOVE_ELAUNCH;
    }
    return DOVE_OK;
  }
  const long long total = (long long)n * oh * ow, blocks = (total + NT - 1) / NT;
  DOVE_CHECK_ARG(blocks < (1LL << 31), "resize: n=%d frames of %d x %d exceed one launch", n, oh, ow);
  if (mode == DOVE_RESIZE_BILINEAR)
    hipLaunchKernelGGL(resize_kernel<DOVE_RESIZE_BILINEAR>, dim3((unsigned)blocks), dim3(NT), 0, st, x, h, w, oh, ow, total, out);
  else if (mode == DOVE_RESIZE_BICUBIC)
    hipLaunchKernelGGL(resize_kernel<DOVE_RESIZE_BICUBIC>, dim3((unsigned)blocks), dim3(NT), 0, st, x, h, w, oh, ow, total, out);
  else
    hipLaunchKernelGGL(resize_kernel<DOVE_RESIZE_AREA>, dim3((unsigned)blocks), dim3(NT), 0, st, x, h, w, oh, ow, total, out);
  DOVE_CHECK_LAUNCH("dove_resize_f32");
  return DOVE_OK;
}

extern "C" int dove_add_gaussian_noise_f32(const float* x, int n, int h, int w, const float* sigma, int gray, unsigned long long seed,
                                           unsigned long long stream_id, long long frame0, float* out, void* stream) {
  DOVE_CHECK_ARG(good_shape(n, h, w), "add_gaussian_noise: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(frame0 >= 0 && frame0 < (1LL << 20), "add_gaussian_noise: frame0 %lld out of range", frame0);
  DOVE_CHECK_ARG(x && sigma && out, "add_gaussian_noise: null pointer");
  const long long per = (long long)h * w * (gray ? 1 : 3), frame_floats = (long long)h * w * 3;
  for (int c0 = 0; c0 < n; c0 += CHUNK) {
    const int cn = n - c0 < CHUNK ? n - c0 : CHUNK;
    FrameF s;
    for (int i = 0; i < CHUNK; ++i) s.v[i] = i < cn ? sigma[c0 + i] : 0.f;
    const unsigned long long e0 = (unsigned long long)(frame0 + c0) * (unsigned long long)per;
    const long long count = per * cn, nblocks = (long long)(((e0 + count - 1) >> 2) - (e0 >> 2) + 1);
    const long long want = (nblocks + NT - 1) / NT;
    const unsigned grid = (unsigned)(want < 65536 ? want : 65536);
    const float* xc = x + c0 * frame_floats;
    float* oc = out + c0 * frame_floats;
    if (gray) hipLaunchKernelGGL(gaussian_kernel<true>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, xc, s, seed, stream_id, e0, count, per, nblocks, oc);
    else hipLaunchKernelGGL(gaussian_kernel<false>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, xc, s, seed, stream_id, e0, count, per, nblocks, oc);
    DOVE_CHECK_LAUNCH("dove_add_gaussian_noise_f32");
  }
  return DOVE_OK;
}

extern "C" size_t dove_poisson_noise_workspace_bytes(int n) { return n > 0 ? (size_t)n * 256 * sizeof(int) : 0; }

extern "C" int dove_add_poisson_noise_f32(const float* x, int n, int h, int w, const float* scale, int gray, unsigned long long seed,
                                          unsigned long long stream_id, long long frame0, void* ws, size_t ws_bytes, float* out,
                                          void* stream) {
  DOVE_CHECK_ARG(good_shape(n, h, w), "add_poisson_noise: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(frame0 >= 0 && frame0 < (1LL << 20), "add_poisson_noise: frame0 %lld out of range", frame0);
  DOVE_CHECK_ARG(stream_id < (1ULL << 32), "add_poisson_noise: stream_id must be below 2^32 (the upper counter word counts rejection rounds)");
  DOVE_CHECK_ARG(x && scale && out && ws, "add_poisson_noise: null pointer");
  DOVE_CHECK_ARG(ws_bytes >= dove_poisson_noise_workspace_bytes(n), "add_poisson_noise: workspace of %zu bytes, needs %zu", ws_bytes,
                 dove_poisson_noise_workspace_bytes(n));
  hipStream_t st = (hipStream_t)stream;
  const long long per = (long long)h * w * (gray ? 1 : 3), frame_floats = (long long)h * w * 3;
  const long long fblocks = (per + NT - 1) / NT;
  DOVE_CHECK_ARG(fblocks < (1LL << 31), "add_poisson_noise: a %d x %d frame exceeds one launch", h, w);
  const hipError_t e = hipMemsetAsync(ws, 0, dove_poisson_noise_workspace_bytes(n), st);
  if (e != hipSuccess) {
    dove_set_error("dove_add_poisson_noise_f32: memset failed: %s", hipGetErrorString(e));
    return DOVE_ELAUNCH;
  }
  for (int c0 = 0; c0 < n; c0 += CHUNK) {
    const int cn = n - c0 < CHUNK ? n - c0 : CHUNK;
    FrameF s;
    for (int i = 0; i < CHUNK; ++i) s.v[i] = i < cn ? scale[c0 + i] : 0.f;
    const unsigned long long e0 = (unsigned long long)(frame0 + c0) * (unsigned long long)per;
    const float* xc = x + c0 * frame_floats;
    float* oc = out + c0 * frame_floats;
    int* flags = (int*)ws + (size_t)c0 * 256;
    const dim3 pgrid((unsigned)(fblocks < 1024 ? fblocks : 1024), (unsigned)cn), grid((unsigned)fblocks, (unsigned)cn);
    if (gray) {
      hipLaunchKernelGGL(poisson_presence_kernel<true>, pgrid, dim3(NT), 0, st, xc, per, flags);
      hipLaunchKernelGGL(poisson_kernel<true>, grid, dim3(NT), 0, st, xc, s, seed, stream_id, e0, per, flags, oc);
    } else {
      hipLaunchKernelGGL(poisson_presence_kernel<false>, pgrid, dim3(NT), 0, st, xc, per, flags);
      hipLaunchKernelGGL(poisson_kernel<false>, grid, dim3(NT), 0, st, xc, s, seed, stream_id, e0, per, flags, oc);
    }
    DOVE_CHECK_LAUNCH("dove_add_poisson_noise_f32");
  }
  return DOVE_OK;
}

extern "C" size_t dove_jpeg_roundtrip_workspace_bytes(int n, int h, int w) {
  return good_shape(n, h, w) ? (size_t)n * (size_t)jpeg_frame_ws(h, w) : 0;
}

extern "C" int dove_jpeg_roundtrip(const float* x, int n, int h, int w, const int* quality, void* ws, size_t ws_bytes, unsigned char* out,
                                   void* stream) {
  DOVE_CHECK_ARG(good_shape(n, h, w), "jpeg_roundtrip: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(x && quality && out && ws, "jpeg_roundtrip: null pointer");
  for (int i = 0; i < n; ++i) DOVE_CHECK_ARG(quality[i] >= 1 && quality[i] <= 100, "jpeg_roundtrip: quality[%d] = %d is not in 1..100", i, quality[i]);
  DOVE_CHECK_ARG(ws_bytes >= dove_jpeg_roundtrip_workspace_bytes(n, h, w), "jpeg_roundtrip: workspace of %zu bytes, needs %zu", ws_bytes,
                 dove_jpeg_roundtrip_workspace_bytes(n, h, w));
  const int mcus_x = (w + 15) / 16, mcus_y = (h + 15) / 16;
  const long long mcus = (long long)mcus_x * mcus_y, fws = jpeg_frame_ws(h, w), frame_px = (long long)h * w;
  DOVE_CHECK_ARG(mcus < (1LL << 31), "jpeg_roundtrip: a %d x %d frame exceeds one launch", h, w);
  hipStream_t st = (hipStream_t)stream;
  for (int c0 = 0; c0 < n; c0 += CHUNK) {
    const int cn = n - c0 < CHUNK ? n - c0 : CHUNK;
    FrameI q;
    for (int i = 0; i < CHUNK; ++i) q.v[i] = i < cn ? quality[c0 + i] : 50;
    uint8_t* wc = (uint8_t*)ws + (long long)c0 * fws;
    hipLaunchKernelGGL(jpeg_codec_kernel, dim3((unsigned)mcus, (unsigned)cn), dim3(NT), 0, st, x + c0 * frame_px * 3, h, w, mcus_x, q, wc, fws);
    const long long total = frame_px * cn, blocks = (total + NT - 1) / NT;
    DOVE_CHECK_ARG(blocks < (1LL << 31), "jpeg_roundtrip: %d frames of %d x %d exceed one launch", cn, h, w);
    hipLaunchKernelGGL(jpeg_finish_kernel, dim3((unsigned)blocks), dim3(NT), 0, st, wc, fws, h, w, mcus_y * 16, mcus_x * 16, total,
                       out + c0 * frame_px * 3);
    DOVE_CHECK_LAUNCH("dove_jpeg_roundtrip");
  }
  return DOVE_OK;
}
