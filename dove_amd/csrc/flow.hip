// Optical flow (RAFT) and the warping error, all in fp32 (include/dove_hip.h has the contract).  Activations are
// channels-last fp32: [n][h][w][c] with a pixel stride that may exceed c, so producers fill slices of a concat buffer.  The convolutions and
// the all-pairs correlation are in conv_f32.hip.
//
// instance_norm_f32: slices of 256 pixels give (mean, M2) partials by a local two-pass sum in fp64; one thread per (n, c) merges them in
//   slice order (Chan's update); a third launch applies.  No atomics: two calls give identical bits.
// corr_lookup, gru glue, convex upsampling: one thread per output element.
// flow_warp_error: one thread per pixel; per-block fp64 partials in the workspace, summed in a fixed tree by a second launch.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int IN_SLICE = 256;             // pixels per instance-norm partial
constexpr int LOOKUP_CH = 4 * 81;

// ----------------------------------------------------------- instance norm -----------------------------------------------------------
// block = 8 pixel rows x 32 channels; partial (mean, M2) of slice s of plane (n, c) at ws[((n C + c) S + s) 2]
__global__ __launch_bounds__(NT) void inorm_partial_kernel(const float* __restrict__ x, int HW, int C, int S, double* __restrict__ ws) {
  __shared__ double red[8][32];
  const int cl = threadIdx.x & 31, row = threadIdx.x >> 5, c = blockIdx.y * 32 + cl, s = blockIdx.x, n = blockIdx.z;
  const int p0 = s * IN_SLICE, cnt = min(IN_SLICE, HW - p0);
  const float* xp = x + ((long long)n * HW + p0) * C + c;
  double sum = 0.0;
  if (c < C)
    for (int i = row; i < cnt; i += 8) sum += (double)xp[(long long)i * C];
  red[row][cl] = sum;
  __syncthreads();
  double mean = 0.0;
#pragma unroll
  for (int r = 0; r < 8; ++r) mean += red[r][cl];
  mean /= (double)cnt;
  __syncthreads();
  double m2 = 0.0;
  if (c < C)
    for (int i = row; i < cnt; i += 8) {
      const double d = (double)xp[(long long)i * C] - mean;
      m2 += d * d;
    }
  red[row][cl] = m2;
  __syncthreads();
  if (row == 0 && c < C) {
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) t += red[r][cl];
    double* o = ws + (((long long)n * C + c) * S + s) * 2;
    o[0] = mean;
    o[1] = t;
  }
}

__global__ __launch_bounds__(NT) void inorm_finalize_kernel(const double* __restrict__ ws, int HW, int S, int planes, float eps,
                                                            float* __restrict__ stats) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= planes) return;
  const double* p = ws + (long long)i * S * 2;
  double na = 0.0, mean = 0.0, m2 = 0.0;
  for (int s = 0; s < S; ++s) {
    const double nb = (double)min(IN_SLICE, HW - s * IN_SLICE), d = p[2 * s] - mean, nn = na + nb;
    mean += d * nb / nn;
    m2 += p[2 * s + 1] + d * d * na * nb / nn;
    na = nn;
  }
  stats[2 * i] = (float)mean;
  stats[2 * i + 1] = (float)(1.0 / sqrt(m2 / (double)HW + (double)eps));
}

__global__ __launch_bounds__(NT) void inorm_apply_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                         const float* __restrict__ resid, int relu, int HW, int C, long long total,
                                                         float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const long long n = i / ((long long)HW * C);
  const float* st = stats + (n * C + c) * 2;
  float v = (x[i] - st[0]) * st[1];
  if (relu) v = fmaxf(v, 0.f);
  if (resid) v = fmaxf(resid[i] + v, 0.f);
  out[i] = v;
}

// ------------------------------------------------------------ correlation ------------------------------------------------------------
__global__ __launch_bounds__(NT) void avgpool2_kernel(const float* __restrict__ x, int h, int w, long long total, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int oh = h >> 1, ow = w >> 1, ox = (int)(i % ow), oy = (int)((i / ow) % oh);
  const long long pl = i / ((long long)ow * oh);
  const float* p = x + (pl * h + 2 * oy) * w + 2 * ox;
  out[i] = ((p[0] + p[1]) + (p[w] + p[w + 1])) * 0.25f;
}

// bilinear sample with zeros outside (grid_sample, align_corners=True, on pixel coordinates)
__device__ __forceinline__ float tap(const float* __restrict__ pl, int h, int w, int y, int x, long long sy, long long sx) {
  return (y >= 0 && y < h && x >= 0 && x < w) ? pl[y * sy + x * sx] : 0.f;
}

struct Bilin {
  int x0, y0;
  float nw, ne, sw, se;
};

__device__ __forceinline__ Bilin bilin(float x, float y) {
  Bilin b;
  const float fx0 = floorf(x), fy0 = floorf(y);
  // far outside: every tap is zero anyway; keep the integer conversion defined
  b.x0 = (int)fminf(fmaxf(fx0, -2.f), 1.0e9f);
  b.y0 = (int)fminf(fmaxf(fy0, -2.f), 1.0e9f);
  const float ax = x - fx0, ay = y - fy0, bx = (fx0 + 1.f) - x, by = (fy0 + 1.f) - y;
  b.nw = bx * by; b.ne = ax * by; b.sw = bx * ay; b.se = ax * ay;
  return b;
}

__device__ __forceinline__ float sample(const float* __restrict__ pl, int h, int w, long long sy, long long sx, const Bilin& b) {
  return tap(pl, h, w, b.y0, b.x0, sy, sx) * b.nw + tap(pl, h, w, b.y0, b.x0 + 1, sy, sx) * b.ne +
         tap(pl, h, w, b.y0 + 1, b.x0, sy, sx) * b.sw + tap(pl, h, w, b.y0 + 1, b.x0 + 1, sy, sx) * b.se;
}

struct Levels { const float* l[4]; };

// channel = level * 81 + a * 9 + b samples level `level` at (x / 2^level + a - 4, y / 2^level + b - 4): the window's FIRST index moves x
__global__ __launch_bounds__(NT) void corr_lookup_kernel(Levels lv, const float* __restrict__ coords, long long ldc, int add_grid, int h,
                                                         int w, long long total, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  const int ch = (int)(t % LOOKUP_CH);
  const long long pix = t / LOOKUP_CH;
  const int level = ch / 81, r = ch - level * 81, a = r / 9, b = r - a * 9;
  float cx = coords[pix * ldc], cy = coords[pix * ldc + 1];
  if (add_grid) {
    cx += (float)(pix % w);
    cy += (float)((pix / w) % h);
  }
  const int hl = h >> level, wl = w >> level;
  const float inv = 1.f / (float)(1 << level);
  const Bilin bl = bilin(cx * inv + (float)(a - 4), cy * inv + (float)(b - 4));
  const float* lp = level == 0 ? lv.l[0] : level == 1 ? lv.l[1] : level == 2 ? lv.l[2] : lv.l[3];
  out[t] = sample(lp + pix * hl * wl, hl, wl, wl, 1, bl);
}

// --------------------------------------------------------------- glue ---------------------------------------------------------------
__global__ __launch_bounds__(NT) void gru_gate_kernel(const float* __restrict__ r, long long ldr, const float* __restrict__ hx, long long ld,
                                                      int ch_h, int ch, long long total, float* __restrict__ rhx) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % ch);
  const long long p = i / ch;
  const float v = hx[p * ld + c];
  rhx[p * ld + c] = c < ch_h ? r[p * ldr + c] * v : v;
}

__global__ __launch_bounds__(NT) void gru_update_kernel(const float* __restrict__ z, long long ldz, const float* __restrict__ q, long long ldq,
                                                        float* __restrict__ hx, long long ld, int ch_h, long long total) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % ch_h);
  const long long p = i / ch_h;
  const float zz = z[p * ldz + c];
  hx[p * ld + c] = (1.f - zz) * hx[p * ld + c] + zz * q[p * ldq + c];
}

__global__ __launch_bounds__(NT) void add_kernel(const float* __restrict__ a, long long lda, const float* __restrict__ b, long long ldb,
                                                 float* __restrict__ out, long long ldo, int ch, int relu, long long total) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % ch);
  const long long p = i / ch;
  const float v = a[p * lda + c] + b[p * ldb + c];
  out[p * ldo + c] = relu ? fmaxf(v, 0.f) : v;
}

// flow [n][h][w] pixels of stride ldf (x, y first), mask [n][h][w][576] with channel = tap * 64 + i * 8 + j -> out [n][2][8h][8w]
__global__ __launch_bounds__(NT) void convex_up_kernel(const float* __restrict__ flow, long long ldf, const float* __restrict__ mask, int h,
                                                       int w, long long total, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  const int ij = (int)(t & 63), i = ij >> 3, j = ij & 7;
  const long long pix = t >> 6;
  const int x = (int)(pix % w), y = (int)((pix / w) % h);
  const long long n = pix / ((long long)w * h);
  const float* mp = mask + pix * 576 + ij;
  float m[9], mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    m[k] = mp[k * 64];
    mx = fmaxf(mx, m[k]);
  }
  float s = 0.f, ax = 0.f, ay = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float e = expf(m[k] - mx);
    s += e;
    const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
    if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
      const float* f = flow + ((n * h + yy) * w + xx) * ldf;
      ax = fmaf(e, 8.f * f[0], ax);
      ay = fmaf(e, 8.f * f[1], ay);
    }
  }
  const long long H8 = 8LL * h, W8 = 8LL * w, o = ((n * 2) * H8 + 8 * y + i) * W8 + 8 * x + j;
  out[o] = ax / s;
  out[o + H8 * W8] = ay / s;
}

// ----------------------------------------------------------- warping error -----------------------------------------------------------
template <typename T>
__device__ __forceinline__ float pix_value(const T* p);
template <>
__device__ __forceinline__ float pix_value<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float pix_value<unsigned char>(const unsigned char* p) { return (float)*p / 255.f; }

template <typename T>
__device__ __forceinline__ float sample_img(const T* __restrict__ img, int h, int w, int c, const Bilin& b) {
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = b.y0 + (k >> 1), x = b.x0 + (k & 1);
    v[k] = (y >= 0 && y < h && x >= 0 && x < w) ? pix_value(img + ((long long)y * w + x) * 3 + c) : 0.f;
  }
  return v[0] * b.nw + v[1] * b.ne + v[2] * b.sw + v[3] * b.se;
}

// img [n][h][w][3], flows [n][2][h][w]; partials [n][blocks][2] fp64 = {masked squared error, mask count}
template <typename T>
__global__ __launch_bounds__(NT) void warp_error_kernel(const T* __restrict__ img1, const T* __restrict__ img2, const float* __restrict__ fw,
                                                        const float* __restrict__ bw, int h, int w, double* __restrict__ partial,
                                                        float* __restrict__ warped, unsigned char* __restrict__ mask) {
  __shared__ double red[2][NT];
  const int tid = threadIdx.x, n = blockIdx.y;
  const long long HW = (long long)h * w, p = (long long)blockIdx.x * NT + tid;
  double err = 0.0, cnt = 0.0;
  if (p < HW) {
    const int x = (int)(p % w), y = (int)(p / w);
    const float* f = fw + (long long)n * 2 * HW;
    const float* g = bw + (long long)n * 2 * HW;
    const float fx = f[p], fy = f[HW + p], sx = (float)x + fx, sy = (float)y + fy;
    const Bilin b = bilin(sx, sy);
    const float bx = sample(g, h, w, w, 1, b), by = sample(g + HW, h, w, w, 1, b);
    const double dx = (double)fx + (double)bx, dy = (double)fy + (double)by;
    const double d = dx * dx + dy * dy;
    const double thr = 0.01 * ((double)fx * fx + (double)fy * fy + (double)bx * bx + (double)by * by) + 0.5;
    const bool valid = d < thr;
    const bool inside = sx >= 0.f && sx <= (float)(w - 1) && sy >= 0.f && sy <= (float)(h - 1);
    const T* i1 = img1 + ((long long)n * HW + p) * 3;
    const T* i2 = img2 + (long long)n * HW * 3;
    double e = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float wv = sample_img(i2, h, w, c, b);
      const float df = pix_value(i1 + c) - wv;
      e += (double)df * (double)df;
      if (warped) warped[((long long)n * HW + p) * 3 + c] = wv;
    }
    if (mask) mask[(long long)n * HW + p] = (unsigned char)((valid ? 1 : 0) | (inside ? 2 : 0));
    if (valid && inside) {
      err = e;
      cnt = 1.0;
    }
  }
  red[0][tid] = err;
  red[1][tid] = cnt;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* o = partial + ((long long)n * gridDim.x + blockIdx.x) * 2;
    o[0] = red[0][0];
    o[1] = red[1][0];
  }
}

__global__ __launch_bounds__(NT) void warp_error_sum_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
  __shared__ double red[2][NT];
  const int tid = threadIdx.x, n = blockIdx.x;
  const double* p = partial + (long long)n * blocks * 2;
  double a = 0.0, b = 0.0;
  for (int i = tid; i < blocks; i += NT) {
    a += p[2 * i];
    b += p[2 * i + 1];
  }
  red[0][tid] = a;
  red[1][tid] = b;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[2 * n] = red[0][0];
    out[2 * n + 1] = red[1][0];
  }
}

inline unsigned blocks_for(long long total) { return (unsigned)((total + NT - 1) / NT); }
constexpr long long MAX_ELEMS = (long long)NT * 0x7fffffffLL;      // one-dimensional grids of NT-thread blocks

}  // namespace

// ------------------------------------------------------------- C entries -------------------------------------------------------------
static size_t inorm_ws(int n, int h, int w, int c) {
  const long long S = ((long long)h * w + IN_SLICE - 1) / IN_SLICE;
  return (size_t)((long long)n * c * S * 2 * sizeof(double) + (long long)n * c * 2 * sizeof(float));
}

extern "C" size_t dove_instance_norm_f32_workspace_bytes(int n, int h, int w, int c) {
  return (n > 0 && h > 0 && w > 0 && c > 0) ? inorm_ws(n, h, w, c) : 0;
}

extern "C" int dove_instance_norm_f32(const float* x, int n, int h, int w, int c, const float* resid, int relu, float eps, void* ws,
                                      size_t ws_bytes, float* out, void* stream) {
  DOVE_CHECK_ARG(x && out && ws, "dove_instance_norm_f32: null x / out / ws");
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0 && n <= 65535, "dove_instance_norm_f32: n (<= 65535), h, w, c must be positive");
  DOVE_CHECK_ARG((long long)h * w < (1LL << 31) && (long long)n * h * w * c < MAX_ELEMS, "dove_instance_norm_f32: tensor too large");
  DOVE_CHECK_ARG(ws_bytes >= inorm_ws(n, h, w, c), "dove_instance_norm_f32: workspace of %zu bytes, %zu needed", ws_bytes,
                 inorm_ws(n, h, w, c));
  DOVE_CHECK_ARG(eps > 0.f, "dove_instance_norm_f32: eps must be positive");
  const int HW = h * w, S = (HW + IN_SLICE - 1) / IN_SLICE, planes = n * c;
  double* part = (double*)ws;
  float* stats = (float*)(part + (long long)planes * S * 2);
  hipLaunchKernelGGL(inorm_partial_kernel, dim3(S, (c + 31) / 32, n), dim3(NT), 0, (hipStream_t)stream, x, HW, c, S, part);
  hipLaunchKernelGGL(inorm_finalize_kernel, dim3(blocks_for(planes)), dim3(NT), 0, (hipStream_t)stream, part, HW, S, planes, eps, stats);
  const long long total = (long long)n * HW * c;
  hipLaunchKernelGGL(inorm_apply_kernel, dim3(blocks_for(total)), dim3(NT), 0, (hipStream_t)stream, x, stats, resid, relu, HW, c, total, out);
  DOVE_CHECK_LAUNCH("dove_instance_norm_f32");
  return DOVE_OK;
}

extern "C" int dove_avgpool2_f32(const float* x, long long planes, int h, int w, float* out, void* stream) {
  DOVE_CHECK_ARG(x && out, "dove_avgpool2_f32: null x / out");
  DOVE_CHECK_ARG(planes > 0 && h >= 2 && w >= 2, "dove_avgpool2_f32: planes must be positive and h, w at least 2");
  const long long total = planes * (h >> 1) * (w >> 1);
  DOVE_CHECK_ARG(total < MAX_ELEMS, "dove_avgpool2_f32: tensor too large");
  hipLaunchKernelGGL(avgpool2_kernel, dim3(blocks_for(total)), dim3(NT), 0, (hipStream_t)stream, x, h, w, total, out);
  DOVE_CHECK_LAUNCH("dove_avgpool2_f32");
  return DOVE_OK;
}

extern "C" int dove_corr_lookup_f32(const float* level0, const float* level1, const float* level2, const float* level3, const float* coords,
                                    long long ldc, int add_grid, int n, int h, int w, float* out, void* stream) {
  DOVE_CHECK_ARG(level0 && level1 && level2 && level3 && coords && out, "dove_corr_lookup_f32: null level / coords / out");
  DOVE_CHECK_ARG(n > 0 && (h >> 3) > 0 && (w >> 3) > 0, "dove_corr_lookup_f32: n must be positive and h, w at least 8 (got %d x %d)", h, w);
  DOVE_CHECK_ARG(ldc >= 2, "dove_corr_lookup_f32: ldc %lld < 2", ldc);
  const long long total = (long long)n * h * w * LOOKUP_CH;
  DOVE_CHECK_ARG(total < MAX_ELEMS, "dove_corr_lookup_f32: tensor too large");
  Levels lv = {{level0, level1, level2, level3}};
  hipLaunchKernelGGL(corr_lookup_kernel, dim3(blocks_for(total)), dim3(NT), 0, (hipStream_t)stream, lv, coords, ldc, add_grid, h, w, total,
                     out);
  DOVE_CHECK_LAUNCH("dove_corr_lookup_f32");
  return DOVE_OK;
}

extern "C" int dove_gru_gate_f32(const float* r, long long ldr, const float* hx, long long ld, int ch_h, int ch, long long npix, float* rhx,
                                 void* stream) {
  DOVE_CHECK_ARG(r && hx && rhx, "dove_gru_gate_f32: null r / hx / rhx");
  DOVE_CHECK_ARG(npix > 0 && ch_h > 0 && ch >= ch_h && ld >= ch && ldr >= ch_h, "dove_gru_gate_f32: need 0 < ch_h <= ch <= ld, ldr >= ch_h");
  DOVE_CHECK_ARG(npix * ch < MAX_ELEMS, "dove_gru_gate_f32: tensor too large");
  hipLaunchKernelGGL(gru_gate_kernel, dim3(blocks_for(npix * ch)), dim3(NT), 0, (hipStream_t)stream, r, ldr, hx, ld, ch_h, ch, npix * ch, rhx);
  DOVE_CHECK_LAUNCH("dove_gru_gate_f32");
  return DOVE_OK;
}

extern "C" int dove_gru_update_f32(const float* z, long long ldz, const float* q, long long ldq, float* hx, long long ld, int ch_h,
                                   long long npix, void* stream) {
  DOVE_CHECK_ARG(z && q && hx, "dove_gru_update_f32: null z / q / hx");
  DOVE_CHECK_ARG(npix > 0 && ch_h > 0 && ld >= ch_h && ldz >= ch_h && ldq >= ch_h, "dove_gru_update_f32: need 0 < ch_h <= ld, ldz, ldq");
  DOVE_CHECK_ARG(npix * ch_h < MAX_ELEMS, "dove_gru_update_f32: tensor too large");
  hipLaunchKernelGGL(gru_update_kernel, dim3(blocks_for(npix * ch_h)), dim3(NT), 0, (hipStream_t)stream, z, ldz, q, ldq, hx, ld, ch_h,
                     npix * ch_h);
  DOVE_CHECK_LAUNCH("dove_gru_update_f32");
  return DOVE_OK;
}

extern "C" int dove_add_f32(const float* a, long long lda, const float* b, long long ldb, float* out, long long ldo, int ch, long long npix,
                            int relu, void* stream) {
  DOVE_CHECK_ARG(a && b && out, "dove_add_f32: null a / b / out");
  DOVE_CHECK_ARG(npix > 0 && ch > 0 && lda >= ch && ldb >= ch && ldo >= ch, "dove_add_f32: need 0 < ch <= lda, ldb, ldo");
  DOVE_CHECK_ARG(npix * ch < MAX_ELEMS, "dove_add_f32: tensor too large");
  hipLaunchKernelGGL(add_kernel, dim3(blocks_for(npix * ch)), dim3(NT), 0, (hipStream_t)stream, a, lda, b, ldb, out, ldo, ch, relu, npix * ch);
  DOVE_CHECK_LAUNCH("dove_add_f32");
  return DOVE_OK;
}

extern "C" int dove_convex_upsample_f32(const float* flow, long long ldf, const float* mask, int n, int h, int w, float* out, void* stream) {
  DOVE_CHECK_ARG(flow && mask && out, "dove_convex_upsample_f32: null flow / mask / out");
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0 && ldf >= 2, "dove_convex_upsample_f32: n, h, w must be positive and ldf at least 2");
  const long long total = (long long)n * h * w * 64;
  DOVE_CHECK_ARG(total < MAX_ELEMS, "dove_convex_upsample_f32: tensor too large");
  hipLaunchKernelGGL(convex_up_kernel, dim3(blocks_for(total)), dim3(NT), 0, (hipStream_t)stream, flow, ldf, mask, h, w, total, out);
  DOVE_CHECK_LAUNCH("dove_convex_upsample_f32");
  return DOVE_OK;
}

static size_t warp_ws(int n, int h, int w) { return (size_t)n * (((size_t)h * w + NT - 1) / NT) * 2 * sizeof(double); }

extern "C" size_t dove_flow_warp_error_workspace_bytes(int n, int h, int w) { return (n > 0 && h > 0 && w > 0) ? warp_ws(n, h, w) : 0; }

extern "C" int dove_flow_warp_error(const void* img1, const void* img2, int dtype, const float* flow_fw, const float* flow_bw, int n, int h,
                                    int w, void* ws, size_t ws_bytes, double* out, float* warped, unsigned char* mask, void* stream) {
  DOVE_CHECK_ARG(img1 && img2 && flow_fw && flow_bw && ws && out, "dove_flow_warp_error: null image / flow / ws / out");
  DOVE_CHECK_ARG(dtype == DOVE_F32 || dtype == DOVE_U8, "dove_flow_warp_error: dtype %d (DOVE_F32 or DOVE_U8)", dtype);
  DOVE_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && (long long)h * w < (1LL << 31),
                 "dove_flow_warp_error: n (<= 65535), h, w must be positive");
  DOVE_CHECK_ARG(ws_bytes >= warp_ws(n, h, w), "dove_flow_warp_error: workspace of %zu bytes, %zu needed", ws_bytes, warp_ws(n, h, w));
  const int blocks = (int)(((long long)h * w + NT - 1) / NT);
  if (dtype == DOVE_U8)
    hipLaunchKernelGGL(warp_error_kernel<unsigned char>, dim3(blocks, n), dim3(NT), 0, (hipStream_t)stream, (const unsigned char*)img1,
                       (const unsigned char*)img2, flow_fw, flow_bw, h, w, (double*)ws, warped, mask);
  else
    hipLaunchKernelGGL(warp_error_kernel<float>, dim3(blocks, n), dim3(NT), 0, (hipStream_t)stream, (const float*)img1, (const float*)img2,
                       flow_fw, flow_bw, h, w, (double*)ws, warped, mask);
  hipLaunchKernelGGL(warp_error_sum_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, (const double*)ws, blocks, out);
  DOVE_CHECK_LAUNCH("dove_flow_warp_error");
  return DOVE_OK;
}
