// Full-reference image metrics (PSNR, SSIM) of the reference's evaluation step (eval_metrics.py / pyiqa 'psnr' and 'ssim') on the GPU.
//
// One tile launch computes, per workgroup, the PSNR squared-error sum of its core pixels and the SSIM map sum of its outputs; a finishing
// launch reduces those partials per image, in a fixed order, into fp64 {PSNR dB, SSIM}.  No float atomics: two calls are bitwise identical.
//
// Definitions (INTEGRATION.md 'Metrics'): values in [0,1], uint8 read as u/255.
//   PSNR = 10 log10(1 / (mse + 1e-8)), mse over C, H, W (or over the float Y of eval_metrics.py's rgb_to_y).
//   SSIM: luma Y = rint(255 (0.299 R + 0.587 G + 0.114 B)) (3 channels) or rint(255 v) (1 channel); 11x11 Gaussian window, sigma 1.5,
//   'valid' filtering; C1 = (0.01*255)^2, C2 = (0.03*255)^2; map = l * relu(cs); SSIM = mean of the (H-10) x (W-10) map.
// The luma and rgb_to_y expressions are evaluated in fp64 without contraction, in the order written above, so rint() sees the same value
// as a float64 restatement (ties included).  The window sums run in fp64: E[x^2] - mu^2 of 0..255 values cancels most fp32 digits.
#include "common.h"
#include "../../include/dove_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TW = 64;                    // SSIM outputs per tile row: one per lane
constexpr int TH = 32;                    // SSIM output rows per tile: 4 waves x RW
constexpr int RW = 8;                     // output rows per wave (vertical pass in registers)
constexpr int WIN = 11, HALO = WIN - 1;
constexpr int LW = TW + HALO, LH = TH + HALO;
constexpr int NT = 256;
constexpr int PER = (LH * LW + NT - 1) / NT;   // staged elements per thread

struct Window {                           // normalised 1-D Gaussian g[0..5] (g[10-i] = g[i])
  double g[6];
};

struct View {
  const void* data;
  int dtype;
  long long sn, sc, sh, sw;
};

// element bits of one view for the whole tile: one dtype per call, so the unrolled loads carry no branch between them and stay in
// flight together (a per-element dtype branch makes the compiler wait for each load inside its branch)
template <int DT>
__device__ __forceinline__ void load_tile(const View& v, long long base, int i0, int j0, int H, int W, int cols, long long sc,
                                          uint32_t (&raw)[PER][3]) {
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const int e = threadIdx.x + it * NT, lr = e / cols, lc = e - lr * cols;
    const int y = min(i0 + lr, H - 1), x = min(j0 + lc, W - 1);  // clamped into the image: every load is in bounds
    const long long o = base + (long long)y * v.sh + (long long)x * v.sw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (DT == DOVE_U8) raw[it][c] = ((const uint8_t*)v.data)[o + c * sc];
      else if (DT == DOVE_BF16) raw[it][c] = ((const bf16_t*)v.data)[o + c * sc];
      else raw[it][c] = ((const uint32_t*)v.data)[o + c * sc];
    }
  }
}

__device__ __forceinline__ void load_view(const View& v, long long base, int i0, int j0, int H, int W, int cols, long long sc,
                                          uint32_t (&raw)[PER][3]) {
  if (v.dtype == DOVE_U8) load_tile<DOVE_U8>(v, base, i0, j0, H, W, cols, sc, raw);
  else if (v.dtype == DOVE_BF16) load_tile<DOVE_BF16>(v, base, i0, j0, H, W, cols, sc, raw);
  else load_tile<DOVE_F32>(v, base, i0, j0, H, W, cols, sc, raw);
}

// element bits -> value in [0,1] in fp64; u8 goes through a table of u / 255.0 (an IEEE fp64 division per element costs more than the
// window pass)
__device__ __forceinline__ double unit(uint32_t raw, int dtype, const double* u8_scale) {
  if (dtype == DOVE_U8) return u8_scale[raw];
  if (dtype == DOVE_BF16) return (double)bf2f((bf16_t)raw);
  return (double)__uint_as_float(raw);
}

// eval_metrics.py rgb_to_y: y = 0.257 r + 0.504 g + 0.098 b + 0.0625
__device__ __forceinline__ double rgb_to_y(double r, double g, double b) { return 0.257 * r + 0.504 * g + 0.098 * b + 0.0625; }
// pyiqa's Y channel on data range 255 (rgb2yiq row 0) is luma255() of common.h, shared with niqe.hip

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// grid: one workgroup per (image, tile row, tile column).  ws: [n][tiles][2] 8-byte slots {PSNR error sum, SSIM map sum}; the error sum
// is a u64 integer when `exact` (both inputs uint8, no rgb_to_y: exact_error_sum()), an fp64 otherwise.
__global__ void __launch_bounds__(NT) fr_metrics_tile_kernel(View p, View r, int C, int H, int W, int flags, bool exact, int tiles_x,
                                                             int tiles_y, Window win, double* __restrict__ ws) {
  __shared__ float sx[LH][LW + 1], sy[LH][LW + 1];
  __shared__ double red_d[NT / 64][2];
  __shared__ unsigned long long red_u[NT / 64];
  __shared__ double u8_scale[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = tiles_x * tiles_y;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int i0 = (t / tiles_x) * TH, j0 = (t % tiles_x) * TW;
  const bool do_psnr = flags & DOVE_METRIC_PSNR, do_ssim = flags & DOVE_METRIC_SSIM, to_y = flags & DOVE_METRIC_RGB_TO_Y;
  const long long pn = (long long)n * p.sn, rn = (long long)n * r.sn;

  u8_scale[tid] = (double)tid / 255.0;                           // NT == 256
  __syncthreads();

  // ---- stage: luma of the (TH+10) x (TW+10) halo into LDS; PSNR error of the TH x TW core ----
  // Two phases: every load of the tile is issued first (addresses clamped into the image, so no load sits behind a branch), then the
  // values are converted.  One workgroup per CU runs at a time (the window pass needs 256 VGPRs), so a load -> use -> load chain per
  // element would expose the memory latency once per element.
  const int rows = do_ssim ? LH : TH, cols = do_ssim ? LW : TW;
  const long long pc = C == 3 ? p.sc : 0, rc = C == 3 ? r.sc : 0;     // 1 channel: the three loads read the same element
  uint32_t ra[PER][3], rb[PER][3];
  load_view(p, pn, i0, j0, H, W, cols, pc, ra);
  load_view(r, rn, i0, j0, H, W, cols, rc, rb);
  unsigned long long err_u = 0;
  double err_d = 0.0;
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const int e = tid + it * NT, lr = e / cols, lc = e - lr * cols;
    const int y = i0 + lr, x = j0 + lc;
    float lx = 0.f, ly = 0.f;
    if (e < rows * cols && y < H && x < W) {
      const bool core = lr < TH && lc < TW;
      if (exact) {
        const int a0 = (int)ra[it][0], a1 = (int)ra[it][1], a2 = (int)ra[it][2];
        const int b0 = (int)rb[it][0], b1 = (int)rb[it][1], b2 = (int)rb[it][2];
        if (core && do_psnr)
          err_u += (unsigned)((a0 - b0) * (a0 - b0)) + (C == 3 ? (unsigned)((a1 - b1) * (a1 - b1) + (a2 - b2) * (a2 - b2)) : 0u);
        if (!do_ssim) {
        } else if (C == 3) {
          lx = (float)luma255(u8_scale[a0], u8_scale[a1], u8_scale[a2]);
          ly = (float)luma255(u8_scale[b0], u8_scale[b1], u8_scale[b2]);
        } else {
          lx = (float)rint(255.0 * u8_scale[a0]);
          ly = (float)rint(255.0 * u8_scale[b0]);
        }
      } else {
        double a0 = unit(ra[it][0], p.dtype, u8_scale), a1 = unit(ra[it][1], p.dtype, u8_scale), a2 = unit(ra[it][2], p.dtype, u8_scale);
        double b0 = unit(rb[it][0], r.dtype, u8_scale), b1 = unit(rb[it][1], r.dtype, u8_scale), b2 = unit(rb[it][2], r.dtype, u8_scale);
        if (to_y) {                                              // C == 3 (checked on the host): PSNR and SSIM see the float y
          a0 = rgb_to_y(a0, a1, a2);
          b0 = rgb_to_y(b0, b1, b2);
        }
        const bool rgb = C == 3 && !to_y;
        if (core && do_psnr) {
          const double d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2;
          err_d += rgb ? d0 * d0 + d1 * d1 + d2 * d2 : d0 * d0;
        }
        if (!do_ssim) {
        } else if (rgb) {
          lx = (float)luma255(a0, a1, a2);
          ly = (float)luma255(b0, b1, b2);
        } else {
          lx = (float)rint(255.0 * a0);
          ly = (float)rint(255.0 * b0);
        }
      }
    }
    if (do_ssim && e < rows * cols) { sx[lr][lc] = lx; sy[lr][lc] = ly; }
  }

  // ---- SSIM: horizontal 11-tap pass per input row (lane = output column), vertical pass accumulated in registers ----
  double ssim_sum = 0.0;
  if (do_ssim) {
    __syncthreads();
    const double g0 = win.g[0], g1 = win.g[1], g2 = win.g[2], g3 = win.g[3], g4 = win.g[4], g5 = win.g[5];
    const double G[WIN] = {g0, g1, g2, g3, g4, g5, g4, g3, g2, g1, g0};
    double acc[RW][5];
#pragma unroll
    for (int i = 0; i < RW; ++i)
#pragma unroll
      for (int m = 0; m < 5; ++m) acc[i][m] = 0.0;
    const int r0 = wave * RW;
#pragma unroll
    for (int rr = 0; rr < RW + HALO; ++rr) {
      float a[WIN], b[WIN];
#pragma unroll
      for (int k = 0; k < WIN; ++k) { a[k] = sx[r0 + rr][lane + k]; b[k] = sy[r0 + rr][lane + k]; }
      // symmetric taps: the pair sums of integers <= 255 (and of their products <= 65025) are exact in fp32
      double h[5];
      h[0] = g5 * (double)a[5];
      h[1] = g5 * (double)b[5];
      h[2] = g5 * (double)(a[5] * a[5]);
      h[3] = g5 * (double)(b[5] * b[5]);
      h[4] = g5 * (double)(a[5] * b[5]);
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const double gk = G[k];
        const float pa = a[k] + a[10 - k], pb = b[k] + b[10 - k];
        const float paa = a[k] * a[k] + a[10 - k] * a[10 - k], pbb = b[k] * b[k] + b[10 - k] * b[10 - k];
        const float pab = a[k] * b[k] + a[10 - k] * b[10 - k];
        h[0] = fma(gk, (double)pa, h[0]);
        h[1] = fma(gk, (double)pb, h[1]);
        h[2] = fma(gk, (double)paa, h[2]);
        h[3] = fma(gk, (double)pbb, h[3]);
        h[4] = fma(gk, (double)pab, h[4]);
      }
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        const int i = rr - k;                                    // input row r0+rr is tap k of output row r0+i
        if (i >= 0 && i < RW) {
#pragma unroll
          for (int m = 0; m < 5; ++m) acc[i][m] = fma(G[k], h[m], acc[i][m]);
        }
      }
    }
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const int x = j0 + lane;
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const int y = i0 + r0 + i;
      if (y < H - HALO && x < W - HALO) {
        const double mx = acc[i][0], my = acc[i][1];
        const double mxx = mx * mx, myy = my * my, mxy = mx * my;
        const double sxx = acc[i][2] - mxx, syy = acc[i][3] - myy, sxy = acc[i][4] - mxy;
        const double nl = 2.0 * mxy + C1, dl = mxx + myy + C1;
        const double nc = 2.0 * sxy + C2, dc = sxx + syy + C2;
        ssim_sum += nc > 0.0 ? (nl * nc) / (dl * dc) : 0.0;       // l * relu(cs), one division (dc >= C2 > 0)
      }
    }
  }

  // ---- workgroup sums in a fixed order: lanes (butterfly), then waves 0..3 ----
  ssim_sum = wave_sum_d(ssim_sum);
  if (exact) err_u = wave_sum_u64(err_u); else err_d = wave_sum_d(err_d);
  if (lane == 0) { red_d[wave][0] = err_d; red_d[wave][1] = ssim_sum; red_u[wave] = err_u; }
  __syncthreads();
  if (tid == 0) {
    double e = 0.0, s = 0.0;
    unsigned long long eu = 0;
    for (int w = 0; w < NT / 64; ++w) { e += red_d[w][0]; s += red_d[w][1]; eu += red_u[w]; }
    double* slot = ws + 2 * ((long long)n * tiles + t);
    slot[0] = exact ? __longlong_as_double((long long)eu) : e;
    slot[1] = s;
  }
}

// one workgroup per image: the image's tile partials in a fixed order (strided per thread, then a tree), then {PSNR, SSIM} in fp64
__global__ void __launch_bounds__(NT) fr_metrics_finish_kernel(const double* __restrict__ ws, int tiles, int C, int H, int W, int flags,
                                                               bool exact, double* __restrict__ out) {
  __shared__ double se[NT], ss[NT];
  __shared__ unsigned long long su[NT];
  const int n = blockIdx.x, tid = threadIdx.x;
  const bool to_y = flags & DOVE_METRIC_RGB_TO_Y;
  const double* part = ws + 2 * (long long)n * tiles;
  double e = 0.0, s = 0.0;
  unsigned long long eu = 0;
  for (int t = tid; t < tiles; t += NT) {
    if (exact) eu += (unsigned long long)__double_as_longlong(part[2 * t]); else e += part[2 * t];
    s += part[2 * t + 1];
  }
  se[tid] = e; ss[tid] = s; su[tid] = eu;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (tid < h) { se[tid] += se[tid + h]; ss[tid] += ss[tid + h]; su[tid] += su[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    const double count = (double)(to_y ? 1 : C) * H * W;
    const double mse = exact ? (double)su[0] / 65025.0 / count : se[0] / count;
    out[2 * n] = (flags & DOVE_METRIC_PSNR) ? 10.0 * log10(1.0 / (mse + 1e-8)) : __builtin_nan("");
    out[2 * n + 1] = (flags & DOVE_METRIC_SSIM) ? ss[0] / ((double)(H - HALO) * (W - HALO)) : __builtin_nan("");
  }
}

int tile_count(int h, int w) { return ((h + TH - 1) / TH) * ((w + TW - 1) / TW); }

// the PSNR error sum is an exact integer (u64 partials) for two uint8 inputs read as they are; the one rule both kernels follow
bool exact_error_sum(int pred_dtype, int ref_dtype, int flags) {
  return pred_dtype == DOVE_U8 && ref_dtype == DOVE_U8 && !(flags & DOVE_METRIC_RGB_TO_Y);
}

}  // namespace

extern "C" size_t dove_fr_metrics_workspace_bytes(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)n * tile_count(h, w) * 2 * sizeof(double);
}

extern "C" int dove_fr_metrics(const dove_image_view* pred, const dove_image_view* ref, int n, int channels, int h, int w, int flags,
                               void* ws, size_t ws_bytes, double* out, void* stream) {
  // argument checks first, the null-pointer check last: a call that is wrong in any way never reaches a launch
  DOVE_CHECK_ARG(pred && ref, "fr_metrics: null view");
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0, "fr_metrics: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(channels == 1 || channels == 3, "fr_metrics: channels must be 1 or 3, got %d", channels);
  DOVE_CHECK_ARG((flags & ~(DOVE_METRIC_PSNR | DOVE_METRIC_SSIM | DOVE_METRIC_RGB_TO_Y)) == 0 &&
                     (flags & (DOVE_METRIC_PSNR | DOVE_METRIC_SSIM)) != 0,
                 "fr_metrics: flags 0x%x must ask for PSNR (1) and/or SSIM (2), optionally with rgb_to_y (4)", flags);
  DOVE_CHECK_ARG(!(flags & DOVE_METRIC_RGB_TO_Y) || channels == 3, "fr_metrics: rgb_to_y needs 3-channel input");
  DOVE_CHECK_ARG(!(flags & DOVE_METRIC_SSIM) || (h >= WIN && w >= WIN),
                 "fr_metrics: SSIM needs H and W >= 11 (the 11x11 window is applied 'valid'), got %d x %d", h, w);
  DOVE_CHECK_ARG(pred->dtype >= DOVE_F32 && pred->dtype <= DOVE_U8 && ref->dtype >= DOVE_F32 && ref->dtype <= DOVE_U8,
                 "fr_metrics: bad dtype %d / %d (0 f32, 1 bf16, 2 u8)", pred->dtype, ref->dtype);
  const size_t need = dove_fr_metrics_workspace_bytes(n, h, w);
  DOVE_CHECK_ARG(ws_bytes >= need, "fr_metrics: workspace of %zu bytes is too small, need %zu (dove_fr_metrics_workspace_bytes)", ws_bytes,
                 need);
  DOVE_CHECK_ARG(pred->data && ref->data && out && ws, "fr_metrics: null pointer");
  Window win;
  double sum = 0.0;
  for (int i = 0; i < WIN; ++i) sum += exp(-(double)((i - 5) * (i - 5)) / 4.5);
  for (int i = 0; i < 6; ++i) win.g[i] = exp(-(double)((i - 5) * (i - 5)) / 4.5) / sum;
  const View p{pred->data, pred->dtype, pred->sn, pred->sc, pred->sh, pred->sw};
  const View r{ref->data, ref->dtype, ref->sn, ref->sc, ref->sh, ref->sw};
  const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
  const long long blocks = (long long)n * tiles_x * tiles_y;
  DOVE_CHECK_ARG(blocks < (1LL << 31), "fr_metrics: %lld tiles exceed one launch", blocks);
  const bool exact = exact_error_sum(pred->dtype, ref->dtype, flags);
  hipLaunchKernelGGL(fr_metrics_tile_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, p, r, channels, h, w, flags, exact,
                     tiles_x, tiles_y, win, (double*)ws);
  DOVE_CHECK_LAUNCH("dove_fr_metrics (tiles)");
  hipLaunchKernelGGL(fr_metrics_finish_kernel, dim3((unsigned)n), dim3(NT), 0, (hipStream_t)stream, (const double*)ws, tiles_x * tiles_y,
                     channels, h, w, flags, exact, out);
  DOVE_CHECK_LAUNCH("dove_fr_metrics (finish)");
  return DOVE_OK;
}
