// Colour fix of SR frames against their upscaled input (the reference's finetune/scripts/color_fix_util.py: the StableSR colour fix) on
// the GPU.  content = the restored frame, style = the upscaled low-quality frame; [n,3,h,w] strided views, every frame on its own.
//
// Definitions, values in [0,1] after the per-input affine  v = scale * raw + bias  (uint8 raw = u / 255):
//   wavelet: B_r(x) = the 3x3 kernel [1,2,1]^T [1,2,1] / 16 with dilation r; a tap outside the image reads the CLAMPED coordinate of that
//            level's input.  low5 = B_16 B_8 B_4 B_2 B_1.  out = content + low5(style - content)   (one pyramid, on the difference: equal
//            by linearity to the reference's (content - low5(content)) + low5(style)).
//   adain:   per frame and channel mean and std = sqrt(var + 1e-5), var unbiased (divisor h*w - 1);
//            out = (content - mean_c) / std_c * std_s + mean_s.
//
// wavelet level structure (docs/kernels.md): three launches over 64 x 32 tiles, all three channels of a tile in one workgroup.
//   1. levels 1, 2, 4 fused in LDS (halo 7) from the two inputs -> fp32 plane A
//   2. level 8: nine clamped loads per output from plane A      -> fp32 plane B
//   3. level 16: the same from plane B, + content               -> out
// Every level is defined by clamped reads of the level below: "level k outside the image" is level k's border value, never a blur of
// padded data (the invariant that keeps this true inside the fused tile is stated at blur_region).
// Arithmetic is fp32 throughout (no bf16 intermediates).  FMA contraction is switched off for the file; the blur asks for its one fused
// multiply-add by name (tap3), where the product by a power of two is exact and fusing cannot change a bit.
// adain: a statistics launch (fp64 sums per pixel chunk, fixed order) and an apply launch (each workgroup reduces its frame's chunk
// partials in the same fixed order, then out = fma(x, a, b) in fp64 with a = std_s / std_c, b = mean_s - mean_c * a, rounded once).
// No float atomics anywhere: two calls give identical bits.
#include "common.h"
#include "../../include/dove_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int TW = 64, TH = 32;           // output tile: one column per lane, 8 rows per wave

struct View {
  const void* data;
  int dtype;
  long long sn, sc;
  int sh, sw;                              // inside one (n, c) plane every offset fits 32 bits (checked on the host)
  float scale, bias;
};

template <int DT>
__device__ __forceinline__ float load_raw(const void* p, long long o) {
  if (DT == DOVE_U8) return (float)((const uint8_t*)p)[o] / 255.0f;
  if (DT == DOVE_BF16) return bf2f(((const bf16_t*)p)[o]);
  return ((const float*)p)[o];
}

template <int DT>
__device__ __forceinline__ float load_val(const View& v, long long o) {
  return v.scale * load_raw<DT>(v.data, o) + v.bias;
}

__device__ __forceinline__ float load_dyn(const View& v, long long o) {
  if (v.dtype == DOVE_U8) return load_val<DOVE_U8>(v, o);
  if (v.dtype == DOVE_BF16) return load_val<DOVE_BF16>(v, o);
  return load_val<DOVE_F32>(v, o);
}

__device__ __forceinline__ void store_out(const View& o, long long off, float v, bool clamp) {
  if (o.dtype == DOVE_U8) {
    ((uint8_t*)o.data)[off] = (uint8_t)(fminf(fmaxf(v, 0.f), 1.f) * 255.0f);   // trunc(clamp(x,0,1) * 255): dove_postprocess_u8's rule
    return;
  }
  if (clamp) v = fminf(fmaxf(v, 0.f), 1.f);
  if (o.dtype == DOVE_BF16) ((bf16_t*)o.data)[off] = f2bf(v);
  else ((float*)o.data)[off] = v;
}

// Invariant of every LDS level: position q of the tile holds that level's value at the pixel clamp(q) - q clamped into the image per
// axis.  Staging establishes it (every load reads the clamped coordinate); a blur keeps it by evaluating at the CLAMPED centre and
// storing at the unclamped position.  With it the taps of an in-image centre need no clamp of their own: centre +- R either is in the
// image or holds the border value of the level below, which is what a clamped read returns.
//
// level R over the LDS region [OFF, LH - OFF) x [OFF, LW - OFF) from the previous level in src; (by, bx) = image coordinate of src[0].
// put(ly, lx, value) stores.
// [1,2,1] / 4.  The products by 0.25 and 0.5 are exact, so the fused multiply-add rounds exactly as a multiply and an add would.
__device__ __forceinline__ float tap3(float l, float c, float r) { return fmaf(0.5f, c, 0.25f * (l + r)); }

// CLAMPED = false: the whole tile lies inside the image (three tiles in four of a 720p frame) and the centre needs no clamp either
template <int R, int OFF, int LH, int LW, bool CLAMPED, typename Put>
__device__ __forceinline__ void blur_region(const float* src, int by, int bx, int H, int W, Put put) {
  constexpr int RH = LH - 2 * OFF, RW = LW - 2 * OFF;
#pragma unroll 4
  for (int e = threadIdx.x; e < RH * RW; e += NT) {
    const int ry = e / RW, ly = ry + OFF, lx = e - ry * RW + OFF;
    const float* p = CLAMPED ? src + (min(max(by + ly, 0), H - 1) - by) * LW + (min(max(bx + lx, 0), W - 1) - bx) : src + ly * LW + lx;
    const float t = tap3(p[-R * LW - R], p[-R * LW], p[-R * LW + R]);
    const float m = tap3(p[-R], p[0], p[R]);
    const float b = tap3(p[R * LW - R], p[R * LW], p[R * LW + R]);
    put(ly, lx, tap3(t, m, b));
  }
}

template <int R, int OFF, int LH, int LW, typename Put>
__device__ __forceinline__ void blur_region(const float* src, bool inside, int by, int bx, int H, int W, Put put) {
  if (inside) blur_region<R, OFF, LH, LW, false>(src, by, bx, H, W, put);
  else blur_region<R, OFF, LH, LW, true>(src, by, bx, H, W, put);
}

// pre[i] = get(clamped y, clamped x) of tile element threadIdx.x + i * NT: every global load is inside the image.  The values stay in
// registers until commit_tile, so the loads of the next channel fly while the current one is blurred.
template <int LH, int LW, typename Get>
__device__ __forceinline__ void fetch_tile(float (&pre)[(LH * LW + NT - 1) / NT], int by, int bx, int H, int W, Get get) {
#pragma unroll
  for (int i = 0; i < (LH * LW + NT - 1) / NT; ++i) {
    const int e = min((int)threadIdx.x + i * NT, LH * LW - 1), ly = e / LW, lx = e - ly * LW;
    pre[i] = get(min(max(by + ly, 0), H - 1), min(max(bx + lx, 0), W - 1));
  }
}

template <int LH, int LW>
__device__ __forceinline__ void commit_tile(float* dst, const float (&pre)[(LH * LW + NT - 1) / NT]) {
#pragma unroll
  for (int i = 0; i < (LH * LW + NT - 1) / NT; ++i) {
    const int e = threadIdx.x + i * NT;
    if (e < LH * LW) dst[e] = pre[i];
  }
}

template <int DTC, int DTS, int LH, int LW>
__device__ __forceinline__ void fetch_diff(const View& c, const View& s, long long cb, long long sb, float (&pre)[(LH * LW + NT - 1) / NT],
                                           int by, int bx, int H, int W) {
  fetch_tile<LH, LW>(pre, by, bx, H, W, [&](int y, int x) {
    return load_val<DTS>(s, sb + (y * s.sh + x * s.sw)) - load_val<DTC>(c, cb + (y * c.sh + x * c.sw));
  });
}

// one dtype pair per call: the loads of a pass carry no branch between them and stay in flight together
template <int LH, int LW>
__device__ __forceinline__ void fetch_diff_any(const View& c, const View& s, int n, int ch, float (&pre)[(LH * LW + NT - 1) / NT], int by,
                                               int bx, int H, int W) {
  const long long cb = n * c.sn + ch * c.sc, sb = n * s.sn + ch * s.sc;
#define DOVE_CF_PAIR(DC, DS) \
  if (c.dtype == DC && s.dtype == DS) return fetch_diff<DC, DS, LH, LW>(c, s, cb, sb, pre, by, bx, H, W)
  DOVE_CF_PAIR(DOVE_BF16, DOVE_BF16);
  DOVE_CF_PAIR(DOVE_BF16, DOVE_F32);
  DOVE_CF_PAIR(DOVE_BF16, DOVE_U8);
  DOVE_CF_PAIR(DOVE_F32, DOVE_BF16);
  DOVE_CF_PAIR(DOVE_F32, DOVE_F32);
  DOVE_CF_PAIR(DOVE_F32, DOVE_U8);
  DOVE_CF_PAIR(DOVE_U8, DOVE_BF16);
  DOVE_CF_PAIR(DOVE_U8, DOVE_F32);
  DOVE_CF_PAIR(DOVE_U8, DOVE_U8);
#undef DOVE_CF_PAIR
}

struct Tile {
  int n, y0, x0;
};

__device__ __forceinline__ Tile tile_of_block(int tiles_x, int tiles_y) {
  const unsigned b = xcd_remap(blockIdx.x, gridDim.x);          // neighbouring tiles share one XCD's L2: the halos are read from it
  const int tiles = tiles_x * tiles_y;
  const int n = b / tiles, t = b - n * tiles;
  return Tile{n, (t / tiles_x) * TH, (t % tiles_x) * TW};
}

// launch 1: d = style - content, then levels 1, 2, 4 in LDS -> plane [n][3][H][W] fp32
__global__ void __launch_bounds__(NT, 4) wavelet_l124_kernel(View c, View s, int H, int W, int tiles_x, int tiles_y, float* __restrict__ dst) {
  constexpr int HALO = 7, LH = TH + 2 * HALO, LW = TW + 2 * HALO;
  __shared__ float a[LH * LW], b[LH * LW];
  const Tile t = tile_of_block(tiles_x, tiles_y);
  const int by = t.y0 - HALO, bx = t.x0 - HALO;
  const bool inside = by >= 0 && bx >= 0 && by + LH <= H && bx + LW <= W;       // block-uniform
  float pre[(LH * LW + NT - 1) / NT];
  fetch_diff_any<LH, LW>(c, s, t.n, 0, pre, by, bx, H, W);
#pragma unroll 1
  for (int ch = 0; ch < 3; ++ch) {
    commit_tile<LH, LW>(a, pre);
    __syncthreads();
    if (ch < 2) fetch_diff_any<LH, LW>(c, s, t.n, ch + 1, pre, by, bx, H, W);
    blur_region<1, 1, LH, LW>(a, inside, by, bx, H, W, [&](int ly, int lx, float v) { b[ly * LW + lx] = v; });
    __syncthreads();
    blur_region<2, 3, LH, LW>(b, inside, by, bx, H, W, [&](int ly, int lx, float v) { a[ly * LW + lx] = v; });
    __syncthreads();
    float* plane = dst + ((long long)t.n * 3 + ch) * H * W;
    blur_region<4, HALO, LH, LW>(a, inside, by, bx, H, W, [&](int ly, int lx, float v) {
      const int y = by + ly, x = bx + lx;                        // the core of the tile: y >= 0 and x >= 0
      if (y < H && x < W) plane[(long long)y * W + x] = v;
    });
    __syncthreads();                                             // a and b are written again for the next channel
  }
}

// launches 2 and 3: one level of radius R straight from an fp32 plane in global memory (nine clamped loads per output; the rows of a
// tile and of its halo are served by the caches); LAST adds the content and writes the output view.  A wave takes rows
// y0 + wave, y0 + wave + 4, ..., a lane one column.
template <int R, bool LAST>
__global__ void __launch_bounds__(NT) wavelet_level_kernel(const float* __restrict__ src, View c, View o, int clamp, int H, int W,
                                                        int tiles_x, int tiles_y, float* __restrict__ dst) {
  const Tile t = tile_of_block(tiles_x, tiles_y);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = t.x0 + lane;
  if (x >= W) return;
  const int xm = max(x - R, 0), xp = min(x + R, W - 1);
#pragma unroll 1
  for (int ch = 0; ch < 3; ++ch) {
    const float* plane = src + ((long long)t.n * 3 + ch) * H * W;
#pragma unroll 4
    for (int i = 0; i < TH / (NT / 64); ++i) {
      const int y = t.y0 + wave + (NT / 64) * i;
      if (y >= H) break;
      const float* r0 = plane + (long long)max(y - R, 0) * W;
      const float* r1 = plane + (long long)y * W;
      const float* r2 = plane + (long long)min(y + R, H - 1) * W;
      const float low = tap3(tap3(r0[xm], r0[x], r0[xp]), tap3(r1[xm], r1[x], r1[xp]), tap3(r2[xm], r2[x], r2[xp]));
      if (LAST) {
        const float cv = load_dyn(c, t.n * c.sn + ch * c.sc + (y * c.sh + x * c.sw));
        store_out(o, t.n * o.sn + ch * o.sc + (y * o.sh + x * o.sw), cv + low, clamp);
      } else {
        dst[(((long long)t.n * 3 + ch) * H + y) * W + x] = low;
      }
    }
  }
}

// ---- adain ----
// Both launches walk the frame in groups of four pixels of one row (the last group of a row may be shorter).  A group whose view is
// dense along x and aligned is moved with one vector access per channel; any other group goes element by element.  Both ways see the
// same values in the same order, so the result does not depend on the strides.
constexpr int CHUNK = 8192;               // pixels per statistics workgroup (at least)
constexpr int MAX_CHUNKS = 64;            // per frame: what every apply workgroup reduces again (16 threads per sum, 4 partials each)
constexpr int APPLY_GROUPS = 4096;        // pixel groups per apply workgroup: the reduction above is a small part of its work

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

int chunks_of(long long total) {
  const long long p = (total + CHUNK - 1) / CHUNK;
  return (int)(p < 1 ? 1 : (p > MAX_CHUNKS ? MAX_CHUNKS : p));
}

// f[k] = value of pixel k of the group at element offset o (k < cnt; the rest 0)
__device__ __forceinline__ void load_px4(const View& v, long long o, int cnt, float (&f)[4]) {
  bool done = false;
  if (cnt == 4 && v.sw == 1) {
    if (v.dtype == DOVE_BF16) {
      const bf16_t* p = (const bf16_t*)v.data + o;
      if (((uintptr_t)p & 7) == 0) {
        const uint2 r = *(const uint2*)p;
        f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
        f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
        done = true;
      }
    } else if (v.dtype == DOVE_F32) {
      const float* p = (const float*)v.data + o;
      if (((uintptr_t)p & 15) == 0) {
        const float4 r = *(const float4*)p;
        f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w;
        done = true;
      }
    }
  }
  if (done) {
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = v.scale * f[k] + v.bias;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) f[k] = k < cnt ? load_dyn(v, o + k * v.sw) : 0.f;
}

// grid (chunks, n): ws[n][chunk][12] = {sum, sum of squares} x {content, style} x 3 channels in fp64; a thread adds its pixels in
// index order, then lanes (butterfly), then waves 0..3
__global__ void __launch_bounds__(NT) adain_stats_kernel(View c, View s, int H, int W, int chunks, double* __restrict__ ws) {
  __shared__ double red[NT / 64][12];
  const int n = blockIdx.y, p = blockIdx.x;
  const int G = (W + 3) / 4;
  const long long total = (long long)H * G, per = (total + chunks - 1) / chunks;
  const long long lo = p * per, hi = min(total, lo + per);
  double acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.0;
  for (long long g = lo + threadIdx.x; g < hi; g += NT) {
    const int y = (int)(g / G), x = (int)(g - (long long)y * G) * 4, cnt = min(4, W - x);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float cv[4], sv[4];
      load_px4(c, n * c.sn + ch * c.sc + (y * c.sh + x * c.sw), cnt, cv);
      load_px4(s, n * s.sn + ch * s.sc + (y * s.sh + x * s.sw), cnt, sv);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < cnt) {
          const double a = (double)cv[k], b = (double)sv[k];
          acc[4 * ch + 0] += a;
          acc[4 * ch + 1] += a * a;
          acc[4 * ch + 2] += b;
          acc[4 * ch + 3] += b * b;
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const double v = wave_sum_d(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 12) {
    double v = 0.0;
    for (int w = 0; w < NT / 64; ++w) v += red[w][threadIdx.x];
    ws[((long long)n * chunks + p) * 12 + threadIdx.x] = v;
  }
}

__device__ __forceinline__ uint32_t to_u8(float v) { return (uint32_t)(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

// r[ch][k] -> pixel k of the group at (n, y, x)
__device__ __forceinline__ void store_px4(const View& o, long long off, int cnt, const float (&r)[3][4], bool clamp) {
  if (cnt == 4 && o.dtype == DOVE_U8 && o.sc == 1 && o.sw == 3) {                    // [F,H,W,3] frames: 12 bytes in a row
    uint8_t* p = (uint8_t*)o.data + off;
    if (((uintptr_t)p & 3) == 0) {
      uint32_t b[12];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) b[3 * k + ch] = to_u8(r[ch][k]);
#pragma unroll
      for (int q = 0; q < 3; ++q) ((uint32_t*)p)[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
      return;
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) store_out(o, off + ch * o.sc + k * o.sw, r[ch][k], clamp);
}

// grid (group blocks, n): the frame's chunk partials in chunk order -> per channel a, b in fp64; out = x * a + b
__global__ void __launch_bounds__(NT) adain_apply_kernel(View c, View o, int clamp, int H, int W, int chunks,
                                                         const double* __restrict__ ws) {
  __shared__ double part[16][12];
  __shared__ double sums[12];
  __shared__ double ab[3][2];
  const int n = blockIdx.y;
  {                                                              // fixed order: partials j, j + 16, j + 32, j + 48, then j = 0..15
    const int j = threadIdx.x >> 4, k = threadIdx.x & 15;
    if (k < 12) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < MAX_CHUNKS / 16; ++q) {
        const int p = j + 16 * q;
        v += p < chunks ? ws[((long long)n * chunks + p) * 12 + k] : 0.0;
      }
      part[j][k] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < 12) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) v += part[j][threadIdx.x];
    sums[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double N = (double)H * (double)W;
    const double* q = sums + 4 * threadIdx.x;
    const double mc = q[0] / N, ms = q[2] / N;
    const double vc = fmax((q[1] - q[0] * mc) / (N - 1.0), 0.0), vs = fmax((q[3] - q[2] * ms) / (N - 1.0), 0.0);
    const double a = sqrt(vs + 1e-5) / sqrt(vc + 1e-5);
    ab[threadIdx.x][0] = a;
    ab[threadIdx.x][1] = ms - mc * a;
  }
  __syncthreads();
  const int G = (W + 3) / 4;
  const long long total = (long long)H * G, lo = (long long)blockIdx.x * APPLY_GROUPS;
#pragma unroll 2
  for (int it = 0; it < APPLY_GROUPS / NT; ++it) {
    const long long g = lo + it * NT + threadIdx.x;
    if (g >= total) break;
    const int y = (int)(g / G), x = (int)(g - (long long)y * G) * 4, cnt = min(4, W - x);
    float r[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float cv[4];
      load_px4(c, n * c.sn + ch * c.sc + (y * c.sh + x * c.sw), cnt, cv);
#pragma unroll
      for (int k = 0; k < 4; ++k) r[ch][k] = (float)fma((double)cv[k], ab[ch][0], ab[ch][1]);
    }
    store_px4(o, n * o.sn + (y * o.sh + x * o.sw), cnt, r, clamp);
  }
}

// the kernels address inside one (n, c) plane with 32-bit offsets
bool plane_fits(const dove_image_view* v, int h, int w) {
  const long long lim = 1LL << 31, ah = v->sh < 0 ? -v->sh : v->sh, aw = v->sw < 0 ? -v->sw : v->sw;
  return ah < lim && aw < lim && (h - 1) * ah + (w - 1) * aw < lim;
}

bool good_dtype(int d) { return d == DOVE_F32 || d == DOVE_BF16 || d == DOVE_U8; }

}  // namespace

extern "C" size_t dove_color_fix_workspace_bytes(int mode, int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  if (mode == DOVE_COLORFIX_WAVELET) return (size_t)2 * n * 3 * h * w * sizeof(float);          // planes A and B
  if (mode == DOVE_COLORFIX_ADAIN) return (size_t)n * chunks_of((long long)h * w) * 12 * sizeof(double);
  return 0;
}

extern "C" int dove_color_fix(const dove_image_view* content, float c_scale, float c_bias, const dove_image_view* style, float s_scale,
                              float s_bias, int n, int h, int w, int mode, int flags, const dove_image_view* out, void* ws,
                              size_t ws_bytes, void* stream) {
  // argument checks first, the null-pointer check last: a call that is wrong in any way never reaches a launch
  DOVE_CHECK_ARG(content && style && out, "color_fix: null view");
  DOVE_CHECK_ARG(mode == DOVE_COLORFIX_WAVELET || mode == DOVE_COLORFIX_ADAIN, "color_fix: bad mode %d (1 wavelet, 2 adain)", mode);
  DOVE_CHECK_ARG((flags & ~DOVE_COLORFIX_CLAMP) == 0, "color_fix: bad flags 0x%x (1 = clamp the result to [0,1])", flags);
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0, "color_fix: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(mode != DOVE_COLORFIX_ADAIN || (long long)h * w >= 2,
                 "color_fix: adain needs at least 2 pixels per frame (the unbiased variance of one value is undefined), got %d x %d", h, w);
  DOVE_CHECK_ARG(good_dtype(content->dtype) && good_dtype(style->dtype) && good_dtype(out->dtype),
                 "color_fix: bad dtype %d / %d / %d (0 f32, 1 bf16, 2 u8)", content->dtype, style->dtype, out->dtype);
  const size_t need = dove_color_fix_workspace_bytes(mode, n, h, w);
  DOVE_CHECK_ARG(ws_bytes >= need, "color_fix: workspace of %zu bytes is too small, need %zu (dove_color_fix_workspace_bytes)", ws_bytes,
                 need);
  const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
  const long long blocks = (long long)n * tiles_x * tiles_y;
  DOVE_CHECK_ARG(blocks < (1LL << 31) && n < 65536, "color_fix: n=%d frames of %d x %d exceed one launch", n, h, w);
  DOVE_CHECK_ARG(content->data && style->data && out->data && ws, "color_fix: null pointer");
  DOVE_CHECK_ARG(plane_fits(content, h, w) && plane_fits(style, h, w) && plane_fits(out, h, w),
                 "color_fix: one %d x %d plane of a view spans 2^31 elements or more", h, w);
  const View c{content->data, content->dtype, content->sn, content->sc, (int)content->sh, (int)content->sw, c_scale, c_bias};
  const View s{style->data, style->dtype, style->sn, style->sc, (int)style->sh, (int)style->sw, s_scale, s_bias};
  const View o{out->data, out->dtype, out->sn, out->sc, (int)out->sh, (int)out->sw, 1.f, 0.f};
  const int clamp = flags & DOVE_COLORFIX_CLAMP;
  hipStream_t st = (hipStream_t)stream;
  if (mode == DOVE_COLORFIX_WAVELET) {
    float* A = (float*)ws;
    float* B = A + (size_t)n * 3 * h * w;
    hipLaunchKernelGGL(wavelet_l124_kernel, dim3((unsigned)blocks), dim3(NT), 0, st, c, s, h, w, tiles_x, tiles_y, A);
    DOVE_CHECK_LAUNCH("dove_color_fix (wavelet levels 1-4)");
    hipLaunchKernelGGL((wavelet_level_kernel<8, false>), dim3((unsigned)blocks), dim3(NT), 0, st, (const float*)A, c, o, clamp, h, w,
                       tiles_x, tiles_y, B);
    DOVE_CHECK_LAUNCH("dove_color_fix (wavelet level 8)");
    hipLaunchKernelGGL((wavelet_level_kernel<16, true>), dim3((unsigned)blocks), dim3(NT), 0, st, (const float*)B, c, o, clamp, h, w,
                       tiles_x, tiles_y, (float*)nullptr);
    DOVE_CHECK_LAUNCH("dove_color_fix (wavelet level 16)");
  } else {
    const long long total = (long long)h * w;
    const int chunks = chunks_of(total);
    hipLaunchKernelGGL(adain_stats_kernel, dim3(chunks, n), dim3(NT), 0, st, c, s, h, w, chunks, (double*)ws);
    DOVE_CHECK_LAUNCH("dove_color_fix (adain statistics)");
    const long long ablocks = ((long long)h * ((w + 3) / 4) + APPLY_GROUPS - 1) / APPLY_GROUPS;
    DOVE_CHECK_ARG(ablocks < (1LL << 31), "color_fix: %d x %d exceeds one launch", h, w);
    hipLaunchKernelGGL(adain_apply_kernel, dim3((unsigned)ablocks, n), dim3(NT), 0, st, c, o, clamp, h, w, chunks, (const double*)ws);
    DOVE_CHECK_LAUNCH("dove_color_fix (adain apply)");
  }
  return DOVE_OK;
}
