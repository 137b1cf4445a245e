// Perceptual metrics LPIPS and DISTS (include/dove_hip.h has the contract): the operators of a VGG16 / AlexNet trunk in
// exact fp32 and the two statistical heads in fp64.  Activations are channels-last fp32 [n][h][w][c] with pixel strides, as in flow.hip.
// The trunk's convolution (dove_convnet_conv_f32) is in conv_f32.hip.
//
// prep, maxpool, l2pool: one thread per output element.
// lpips_layer: 16 lanes per pixel stride over the channels and reduce by a fixed butterfly; a block sums its 128 pixels in a fixed tree and
//   writes one fp64 partial; a second launch sums the partials of an image in a fixed tree and adds the mean into out[n].
// dists_layer: slices of 1024 pixels give (mean x, mean y, M2 x, M2 y, C xy) by a local two-pass sum in fp64; one block per image merges them
//   per channel in slice order (Chan's update) and sums the channel terms in a fixed tree.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int LP_PIX = 128;                                         // pixels per lpips partial
constexpr int DS_SLICE = 1024;                                      // pixels per dists partial
constexpr long long MAX_ELEMS = (long long)NT * 0x7fffffffLL;

inline unsigned blocks_for(long long total) { return (unsigned)((total + NT - 1) / NT); }

// ------------------------------------------------------------------ prep ------------------------------------------------------------------
struct Prep {
  dove_image_view v;
  int c, h, w;
  float mul, add, mean[3], std[3];
};

__global__ __launch_bounds__(NT) void percep_prep_kernel(Prep p, long long total, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % 3);
  const long long pix = i / 3;
  const int x = (int)(pix % p.w), y = (int)((pix / p.w) % p.h);
  const long long n = pix / ((long long)p.w * p.h);
  const long long o = n * p.v.sn + (long long)(p.c == 1 ? 0 : ch) * p.v.sc + y * p.v.sh + x * p.v.sw;
  const float v = p.v.dtype == DOVE_U8 ? (float)((const uint8_t*)p.v.data)[o] / 255.f : ((const float*)p.v.data)[o];
  const float m = ch == 0 ? p.mean[0] : ch == 1 ? p.mean[1] : p.mean[2];
  const float s = ch == 0 ? p.std[0] : ch == 1 ? p.std[1] : p.std[2];
  out[i] = (fmaf(p.mul, v, p.add) - m) / s;
}

// ----------------------------------------------------------------- pools -----------------------------------------------------------------
__global__ __launch_bounds__(NT) void maxpool_kernel(const float* __restrict__ x, long long ldx, int h, int w, int c, int k, int s, int ho,
                                                     int wo, long long total, float* __restrict__ out, long long ldo) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % c);
  const long long pix = i / c;
  const int ox = (int)(pix % wo), oy = (int)((pix / wo) % ho);
  const long long n = pix / ((long long)wo * ho);
  float m = -INFINITY;
  for (int a = 0; a < k; ++a)
    for (int b = 0; b < k; ++b) {
      const float v = x[((n * h + oy * s + a) * w + ox * s + b) * ldx + ch];
      if (v > m || v != v) m = v;              // a NaN in the window is the result, as in torch's max_pool2d (fmaxf would drop it)
    }
  out[pix * ldo + ch] = m;
}

__global__ __launch_bounds__(NT) void l2pool_kernel(const float* __restrict__ x, long long ldx, int h, int w, int c, int ho, int wo,
                                                    long long total, float* __restrict__ out, long long ldo) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % c);
  const long long pix = i / c;
  const int ox = (int)(pix % wo), oy = (int)((pix / wo) % ho);
  const long long n = pix / ((long long)wo * ho);
  double sum = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int iy = 2 * oy + a - 1, ix = 2 * ox + b - 1;
      if (iy < 0 || iy >= h || ix < 0 || ix >= w) continue;
      const double v = (double)x[((n * h + iy) * w + ix) * ldx + ch];
      sum += ((a == 1 ? 0.5 : 0.25) * (b == 1 ? 0.5 : 0.25)) * (v * v);
    }
  out[pix * ldo + ch] = (float)sqrt(sum + 1e-12);
}

// ------------------------------------------------------------------ heads ------------------------------------------------------------------
__device__ __forceinline__ double group16_sum(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// grid (blocks per image, n); block: 16 pixels at a time x 16 lanes over the channels, 8 rounds = LP_PIX pixels
__global__ __launch_bounds__(NT) void lpips_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ld,
                                                           const float* __restrict__ lin, int HW, int c, double* __restrict__ partial) {
  __shared__ double red[16];
  const int tid = threadIdx.x, sub = tid & 15, grp = tid >> 4, n = blockIdx.y;
  double tot = 0.0;
  for (int round = 0; round < LP_PIX / 16; ++round) {
    const int pix = blockIdx.x * LP_PIX + round * 16 + grp;          // uniform over the 16 lanes of a group
    const bool live = pix < HW;
    const float* xp = x + ((long long)n * HW + (live ? pix : 0)) * ld;
    const float* yp = y + ((long long)n * HW + (live ? pix : 0)) * ld;
    double sx = 0.0, sy = 0.0;
    for (int k = sub; k < c; k += 16) {
      const double a = (double)xp[k], b = (double)yp[k];
      sx += a * a;
      sy += b * b;
    }
    sx = group16_sum(sx);
    sy = group16_sum(sy);
    const double dx = sqrt(sx) + 1e-10, dy = sqrt(sy) + 1e-10;
    double d = 0.0;
    for (int k = sub; k < c; k += 16) {
      const double t = (double)xp[k] / dx - (double)yp[k] / dy;
      d += (double)lin[k] * (t * t);
    }
    d = group16_sum(d);
    if (live) tot += d;
  }
  if (sub == 0) red[grp] = tot;
  __syncthreads();
  if (tid == 0) {
    const double s = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7])) +
                     (((red[8] + red[9]) + (red[10] + red[11])) + ((red[12] + red[13]) + (red[14] + red[15])));
    partial[(long long)n * gridDim.x + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(NT) void lpips_sum_kernel(const double* __restrict__ partial, int blocks, double hw, double* __restrict__ out) {
  __shared__ double red[NT];
  const int tid = threadIdx.x, n = blockIdx.x;
  const double* p = partial + (long long)n * blocks;
  double a = 0.0;
  for (int i = tid; i < blocks; i += NT) a += p[i];
  red[tid] = a;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) out[n] += red[0] / hw;
}

// block = 8 pixel rows x 32 channels; partial of slice s of plane (n, c) at ws[((n C + c) S + s) 5]
__global__ __launch_bounds__(NT) void dists_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, long long ld, int HW, int C,
                                                           int S, double* __restrict__ ws) {
  __shared__ double red[2][8][32];
  const int cl = threadIdx.x & 31, row = threadIdx.x >> 5, c = blockIdx.y * 32 + cl, s = blockIdx.x, n = blockIdx.z;
  const int p0 = s * DS_SLICE, cnt = min(DS_SLICE, HW - p0);
  const float* xp = x + ((long long)n * HW + p0) * ld + c;
  const float* yp = y + ((long long)n * HW + p0) * ld + c;
  double sx = 0.0, sy = 0.0;
  if (c < C)
    for (int i = row; i < cnt; i += 8) {
      sx += (double)xp[(long long)i * ld];
      sy += (double)yp[(long long)i * ld];
    }
  red[0][row][cl] = sx;
  red[1][row][cl] = sy;
  __syncthreads();
  double mx = 0.0, my = 0.0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    mx += red[0][r][cl];
    my += red[1][r][cl];
  }
  mx /= (double)cnt;
  my /= (double)cnt;
  __syncthreads();
  double xx = 0.0, yy = 0.0, xy = 0.0;
  if (c < C)
    for (int i = row; i < cnt; i += 8) {
      const double a = (double)xp[(long long)i * ld] - mx, b = (double)yp[(long long)i * ld] - my;
      xx += a * a;
      yy += b * b;
      xy += a * b;
    }
  __shared__ double red3[3][8][32];
  red3[0][row][cl] = xx;
  red3[1][row][cl] = yy;
  red3[2][row][cl] = xy;
  __syncthreads();
  if (row == 0 && c < C) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      t0 += red3[0][r][cl];
      t1 += red3[1][r][cl];
      t2 += red3[2][r][cl];
    }
    double* o = ws + (((long long)n * C + c) * S + s) * 5;
    o[0] = mx; o[1] = my; o[2] = t0; o[3] = t1; o[4] = t2;
  }
}

__global__ __launch_bounds__(NT) void dists_finalize_kernel(const double* __restrict__ ws, const double* __restrict__ alpha,
                                                            const double* __restrict__ beta, int HW, int C, int S, double* __restrict__ out) {
  __shared__ double red[NT];
  const int tid = threadIdx.x, n = blockIdx.x;
  double tot = 0.0;
  for (int c = tid; c < C; c += NT) {
    const double* p = ws + ((long long)n * C + c) * S * 5;
    double na = 0.0, mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
    for (int s = 0; s < S; ++s) {
      // one division per slice: r = nb / (na + nb) weights the mean update and, times na, the cross terms
      const double nb = (double)min(DS_SLICE, HW - s * DS_SLICE), nn = na + nb, r = nb / nn, dx = p[5 * s] - mx, dy = p[5 * s + 1] - my, f = na * r;
      mx += dx * r;
      my += dy * r;
      xx += p[5 * s + 2] + dx * dx * f;
      yy += p[5 * s + 3] + dy * dy * f;
      xy += p[5 * s + 4] + dx * dy * f;
      na = nn;
    }
    const double vx = xx / (double)HW, vy = yy / (double)HW, cov = xy / (double)HW;
    const double s1 = (2.0 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6), s2 = (2.0 * cov + 1e-6) / (vx + vy + 1e-6);
    tot += alpha[c] * s1 + beta[c] * s2;
  }
  red[tid] = tot;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) out[n] += red[0];
}

size_t lpips_ws(int n, int h, int w) { return (size_t)n * (((size_t)h * w + LP_PIX - 1) / LP_PIX) * sizeof(double); }
size_t dists_ws(int n, int h, int w, int c) { return (size_t)n * c * (((size_t)h * w + DS_SLICE - 1) / DS_SLICE) * 5 * sizeof(double); }

}  // namespace

// ------------------------------------------------------------- C entries -------------------------------------------------------------
extern "C" int dove_percep_prep_f32(const dove_image_view* in, int n, int c, int h, int w, float pre_mul, float pre_add, const float* mean,
                                    const float* std, float* out, void* stream) {
  DOVE_CHECK_ARG(in && in->data && mean && std && out, "dove_percep_prep_f32: null view / data / mean / std / out");
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0, "dove_percep_prep_f32: n, h, w must be positive");
  DOVE_CHECK_ARG(c == 1 || c == 3, "dove_percep_prep_f32: %d channels (1 or 3)", c);
  DOVE_CHECK_ARG(in->dtype == DOVE_F32 || in->dtype == DOVE_U8, "dove_percep_prep_f32: dtype %d (DOVE_F32 or DOVE_U8)", in->dtype);
  DOVE_CHECK_ARG(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "dove_percep_prep_f32: std must be nonzero");
  const long long total = (long long)n * h * w * 3;
  DOVE_CHECK_ARG(total < MAX_ELEMS, "dove_percep_prep_f32: tensor too large");
  Prep p;
  p.v = *in; p.c = c; p.h = h; p.w = w; p.mul = pre_mul; p.add = pre_add;
  for (int i = 0; i < 3; ++i) {
    p.mean[i] = mean[i];
    p.std[i] = std[i];
  }
  hipLaunchKernelGGL(percep_prep_kernel, dim3(blocks_for(total)), dim3(NT), 0, (hipStream_t)stream, p, total, out);
  DOVE_CHECK_LAUNCH("dove_percep_prep_f32");
  return DOVE_OK;
}

extern "C" int dove_maxpool_f32(const float* x, long long ldx, int n, int h, int w, int c, int k, int stride, float* out, long long ldo,
                                void* stream) {
  DOVE_CHECK_ARG(x && out, "dove_maxpool_f32: null x / out");
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "dove_maxpool_f32: n, h, w, c must be positive");
  DOVE_CHECK_ARG(k >= 1 && k <= 4 && stride >= 1 && stride <= 4, "dove_maxpool_f32: window %d, stride %d (1 to 4)", k, stride);
  DOVE_CHECK_ARG(h >= k && w >= k, "dove_maxpool_f32: image %d x %d is smaller than the window %d", h, w, k);
  DOVE_CHECK_ARG(ldx >= c && ldo >= c, "dove_maxpool_f32: ldx %lld or ldo %lld < c %d", ldx, ldo, c);
  const int ho = (h - k) / stride + 1, wo = (w - k) / stride + 1;
  const long long total = (long long)n * ho * wo * c;
  DOVE_CHECK_ARG(total < MAX_ELEMS, "dove_maxpool_f32: tensor too large");
  hipLaunchKernelGGL(maxpool_kernel, dim3(blocks_for(total)), dim3(NT), 0, (hipStream_t)stream, x, ldx, h, w, c, k, stride, ho, wo, total, out,
                     ldo);
  DOVE_CHECK_LAUNCH("dove_maxpool_f32");
  return DOVE_OK;
}

extern "C" int dove_l2pool_f32(const float* x, long long ldx, int n, int h, int w, int c, float* out, long long ldo, void* stream) {
  DOVE_CHECK_ARG(x && out, "dove_l2pool_f32: null x / out");
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "dove_l2pool_f32: n, h, w, c must be positive");
  DOVE_CHECK_ARG(ldx >= c && ldo >= c, "dove_l2pool_f32: ldx %lld or ldo %lld < c %d", ldx, ldo, c);
  const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  const long long total = (long long)n * ho * wo * c;
  DOVE_CHECK_ARG(total < MAX_ELEMS, "dove_l2pool_f32: tensor too large");
  hipLaunchKernelGGL(l2pool_kernel, dim3(blocks_for(total)), dim3(NT), 0, (hipStream_t)stream, x, ldx, h, w, c, ho, wo, total, out, ldo);
  DOVE_CHECK_LAUNCH("dove_l2pool_f32");
  return DOVE_OK;
}

extern "C" size_t dove_lpips_layer_workspace_bytes(int n, int h, int w) { return (n > 0 && h > 0 && w > 0) ? lpips_ws(n, h, w) : 0; }

extern "C" int dove_lpips_layer(const float* x, const float* y, long long ld, const float* lin, int n, int h, int w, int c, void* ws,
                                size_t ws_bytes, double* out, void* stream) {
  DOVE_CHECK_ARG(x && y && lin && ws && out, "dove_lpips_layer: null x / y / lin / ws / out");
  DOVE_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && c > 0 && (long long)h * w < (1LL << 31),
                 "dove_lpips_layer: n (<= 65535), h, w, c must be positive");
  DOVE_CHECK_ARG(ld >= c, "dove_lpips_layer: ld %lld < c %d", ld, c);
  DOVE_CHECK_ARG(ws_bytes >= lpips_ws(n, h, w), "dove_lpips_layer: workspace of %zu bytes, %zu needed", ws_bytes, lpips_ws(n, h, w));
  const int HW = h * w, blocks = (HW + LP_PIX - 1) / LP_PIX;
  hipLaunchKernelGGL(lpips_partial_kernel, dim3(blocks, n), dim3(NT), 0, (hipStream_t)stream, x, y, ld, lin, HW, c, (double*)ws);
  hipLaunchKernelGGL(lpips_sum_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, (const double*)ws, blocks, (double)HW, out);
  DOVE_CHECK_LAUNCH("dove_lpips_layer");
  return DOVE_OK;
}

extern "C" size_t dove_dists_layer_workspace_bytes(int n, int h, int w, int c) {
  return (n > 0 && h > 0 && w > 0 && c > 0) ? dists_ws(n, h, w, c) : 0;
}

extern "C" int dove_dists_layer(const float* x, const float* y, long long ld, const double* alpha, const double* beta, int n, int h, int w, int c,
                                void* ws, size_t ws_bytes, double* out, void* stream) {
  DOVE_CHECK_ARG(x && y && alpha && beta && ws && out, "dove_dists_layer: null x / y / alpha / beta / ws / out");
  DOVE_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && c > 0 && (long long)h * w < (1LL << 31),
                 "dove_dists_layer: n (<= 65535), h, w, c must be positive");
  DOVE_CHECK_ARG(ld >= c, "dove_dists_layer: ld %lld < c %d", ld, c);
  DOVE_CHECK_ARG(ws_bytes >= dists_ws(n, h, w, c), "dove_dists_layer: workspace of %zu bytes, %zu needed", ws_bytes, dists_ws(n, h, w, c));
  const int HW = h * w, S = (HW + DS_SLICE - 1) / DS_SLICE;
  hipLaunchKernelGGL(dists_partial_kernel, dim3(S, (c + 31) / 32, n), dim3(NT), 0, (hipStream_t)stream, x, y, ld, HW, c, S, (double*)ws);
  hipLaunchKernelGGL(dists_finalize_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, (const double*)ws, alpha, beta, HW, c, S, out);
  DOVE_CHECK_LAUNCH("dove_dists_layer");
  return DOVE_OK;
}
