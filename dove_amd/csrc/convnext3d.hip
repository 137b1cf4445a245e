// DOVER's aesthetic branch (include/dove_hip.h has the contract; tests/dover_ref.py is the definition): what an inflated
// ConvNeXt-Tiny needs beside the Linears (dove_resnet_conv_f32's 1 x 1 walk), dove_layernorm_f32, dove_gelu_f32, dove_swin3d_patch_merge_f32
// and dove_vqa_head_f64.  Activations are channels-last fp32 maps [B][D][H][W][C]; no atomics; repeated calls give identical bits; a sample's
// values do not depend on the batch it is in.
//
// dwconv3d_kernel<TW>: depthwise Conv3d, kernel (3,7,7), zero padding (1,3,3), stride 1, exact fp32.  Every output is ONE fmaf chain that
//   starts from the bias and takes the taps in (kd, kh, kw) order, kd outermost, each index ascending (cross-correlation, as torch's conv3d:
//   tap (kd, kh, kw) reads input (d + kd - 1, h + kh - 3, w + kw - 3)).  A tap whose frame d + kd - 1 lies outside the map is skipped; a tap
//   outside the map in h or w is an FMA with a staged 0, which leaves the same bits.
//   A workgroup owns one output frame (b, d), a TH x TW tile of it and a block of 32 channels (8 float4 lanes).  Per kd it stages the
//   (TH + 6) x (TW + 6) halo tile of frame d + kd - 1 and the 49 taps of the channel block in LDS with 16-byte accesses.  A thread owns one
//   tile row and one float4 of channels: per kh it reads the TW + 6 inputs of its row once into registers and slides the 7 taps over them, so
//   an output costs (TW + 6) / TW * 21 LDS reads instead of 147 (measured times: docs/kernels.md).  LDS rows are (TW + 6) * 8 float4
//   slots, padded to 8 modulo 16 slots: the four 16-lane groups of a ds_read_b128 (two tile rows of one half-row each) then cover the 256-byte
//   bank row exactly once.  TW is 7 or 8, whichever wastes fewer columns of W (8 on a tie); TH = ceil(H / ceil(H / 16)): dove_dwconv3d_tile.
// vqa_resized_view_kernel: one thread per output pixel (t, y, x) of the [t][oh][ow] view: frame frames[t], resampled with two separable tap
//   tables (per output index a first source index, a tap count and normalised fp64 weights, built on the host), the inner sum over x, the outer
//   over y, in fp64 on X (the u8 value itself, or 255.0 v for f32 / bf16), then (sum - mean_c) / std_c without contraction, rounded once.
//   Source coordinates and the frame index are clamped into the clip, so a bad table cannot read outside it.  cols = 1 writes the rows of the
//   (2, 4, 4) patch GEMM in dove_vqa_fragments_f32's column order.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int DW_CB4 = 8, DW_MAX_TH = 16, DW_TAPS = 49, DW_NT = DW_MAX_TH * DW_CB4;

inline unsigned blocks_for(long long total, int nt) { return (unsigned)((total + nt - 1) / nt); }

struct Norm3 {
  double mean[3], std[3];
};

struct Taps {
  const int* tab;      // [out][2]: first source index, tap count
  const double* w;     // [out][max]
  int max;
};

// ------------------------------------------------------------ depthwise 3 x 7 x 7 ------------------------------------------------------------
constexpr int dw_row_slots(int tw) { return (tw + 6) * DW_CB4 + (((tw + 6) * DW_CB4) % 16 == 0 ? 8 : 0); }

inline void dw_tile(int h, int w, int* th, int* tw) {
  const int nh = (h + DW_MAX_TH - 1) / DW_MAX_TH;
  *th = (h + nh - 1) / nh;
  *tw = ((w + 6) / 7) * 7 < ((w + 7) / 8) * 8 ? 7 : 8;
}

template <int TW>
__global__ __launch_bounds__(DW_NT) void dwconv3d_kernel(const float* __restrict__ x, const float* __restrict__ wgt,
                                                         const float* __restrict__ bias, int D, int H, int W, int C, int TH, int ntw,
                                                         float* __restrict__ out) {
  constexpr int COLS = TW + 6, ROW = dw_row_slots(TW);
  extern __shared__ __attribute__((aligned(16))) unsigned char dw_lds[];
  f32x4* tile = (f32x4*)dw_lds;                       // [TH + 6][ROW]
  f32x4* wl = tile + (TH + 6) * ROW;                  // [49][8]
  const long long bd = blockIdx.x;
  const int d = (int)(bd % D);
  const int y0 = (int)(blockIdx.y / ntw) * TH, x0 = (int)(blockIdx.y % ntw) * TW, cb = blockIdx.z * DW_CB4;
  const int tid = threadIdx.x, nthreads = blockDim.x, l = tid & (DW_CB4 - 1), ty = tid >> 3;
  const bool cok = (cb + l) * 4 < C;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[TW];
  {
    const f32x4 b4 = cok ? *(const f32x4*)(bias + (cb + l) * 4) : zero;
#pragma unroll
    for (int i = 0; i < TW; ++i) acc[i] = b4;
  }
  for (int kd = 0; kd < 3; ++kd) {
    const int dz = d + kd - 1;
    if (dz < 0 || dz >= D) continue;                  // the same for the whole workgroup
    __syncthreads();                                  // the previous frame's reads are done
    const float* src = x + (bd + (kd - 1)) * H * W * C;
    for (int i = tid; i < (TH + 6) * COLS * DW_CB4; i += nthreads) {
      const int li = i & (DW_CB4 - 1), col = (i >> 3) % COLS, r = (i >> 3) / COLS;
      const int gy = y0 - 3 + r, gx = x0 - 3 + col;
      f32x4 v = zero;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W && (cb + li) * 4 < C) v = *(const f32x4*)(src + ((long long)gy * W + gx) * C + (cb + li) * 4);
      tile[r * ROW + col * DW_CB4 + li] = v;
    }
    for (int i = tid; i < DW_TAPS * DW_CB4; i += nthreads) {
      const int li = i & (DW_CB4 - 1);
      wl[i] = (cb + li) * 4 < C ? *(const f32x4*)(wgt + (long long)(kd * DW_TAPS + (i >> 3)) * C + (cb + li) * 4) : zero;
    }
    __syncthreads();
    if (ty < TH) {
#pragma unroll
      for (int kh = 0; kh < 7; ++kh) {
        const f32x4* rowp = tile + (ty + kh) * ROW + l;
        const f32x4* wp = wl + kh * 7 * DW_CB4 + l;
        f32x4 in[COLS], w[7];
#pragma unroll
        for (int j = 0; j < COLS; ++j) in[j] = rowp[j * DW_CB4];
#pragma unroll
        for (int k = 0; k < 7; ++k) w[k] = wp[k * DW_CB4];
#pragma unroll
        for (int xo = 0; xo < TW; ++xo)
#pragma unroll
          for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[xo][e] = __builtin_fmaf(in[xo + k][e], w[k][e], acc[xo][e]);
      }
    }
  }
  const int y = y0 + ty;
  if (ty < TH && y < H && cok) {
    float* dst = out + ((bd * H + y) * W + x0) * C + (cb + l) * 4;
#pragma unroll
    for (int xo = 0; xo < TW; ++xo)
      if (x0 + xo < W) *(f32x4*)(dst + (long long)xo * C) = acc[xo];
  }
}

// --------------------------------------------------------------- resized view ---------------------------------------------------------------
__device__ __forceinline__ double normalised(double x, double mean, double std) {
#pragma clang fp contract(off)
  return (x - mean) / std;
}

__global__ __launch_bounds__(NT) void vqa_resized_view_kernel(dove_image_view v, int F, int H, int W, const int* __restrict__ frames, Taps ty,
                                                              Taps tx, int oh, int ow, Norm3 nm, int cols, long long total,
                                                              float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % ow), y = (int)((idx / ow) % oh), t = (int)(idx / ((long long)ow * oh));
  const int f = min(max(frames[t], 0), F - 1);
  const int fy = ty.tab[2 * y], ny = min(max(ty.tab[2 * y + 1], 0), ty.max), fx = tx.tab[2 * x], nx = min(max(tx.tab[2 * x + 1], 0), tx.max);
  const double* wy = ty.w + (long long)y * ty.max;
  const double* wx = tx.w + (long long)x * tx.max;
  double s[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < ny; ++j) {
    const int sy = min(max(fy + j, 0), H - 1);
    double r[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < nx; ++i) {
      const int sx = min(max(fx + i, 0), W - 1);
      const long long base = (long long)f * v.sn + (long long)sy * v.sh + (long long)sx * v.sw;
      const double wi = wx[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long long off = base + c * v.sc;
        double X;
        if (v.dtype == DOVE_U8) X = (double)((const uint8_t*)v.data)[off];
        else if (v.dtype == DOVE_BF16) X = 255.0 * (double)bf2f(((const bf16_t*)v.data)[off]);
        else X = 255.0 * (double)((const float*)v.data)[off];
        r[c] += wi * X;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += wy[j] * r[c];
  }
  float r3[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) r3[c] = (float)normalised(s[c], nm.mean[c], nm.std[c]);
  if (!cols) {
    float* p = out + idx * 3;
    p[0] = r3[0];
    p[1] = r3[1];
    p[2] = r3[2];
  } else {
    const long long row = ((long long)(t >> 1) * (oh >> 2) + (y >> 2)) * (ow >> 2) + (x >> 2);
    float* p = out + row * 96 + (t & 1) * 16 + (y & 3) * 4 + (x & 3);
    p[0] = r3[0];
    p[32] = r3[1];
    p[64] = r3[2];
  }
}

}  // namespace

// ------------------------------------------------------------- C entries -------------------------------------------------------------
extern "C" void dove_dwconv3d_tile(int h, int w, int* th, int* tw) {
  int a = 0, b = 0;
  if (h > 0 && w > 0) dw_tile(h, w, &a, &b);
  if (th) *th = a;
  if (tw) *tw = b;
}

extern "C" int dove_dwconv3d_f32(const float* x, int b, int d, int h, int w, int c, const float* weight, const float* bias, float* out,
                                 void* stream) {
  DOVE_CHECK_ARG(x && weight && bias && out && x != out, "dove_dwconv3d_f32: null x / weight / bias / out, or out aliasing x");
  DOVE_CHECK_ARG(b > 0 && d > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0,
                 "dove_dwconv3d_f32: b %d, d %d, %d x %d, c %d (positive, c a multiple of 4)", b, d, h, w, c);
  DOVE_CHECK_ARG((((uintptr_t)x | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)out) & 15) == 0,
                 "dove_dwconv3d_f32: x, weight, bias and out must be 16-byte aligned");
  const long long maps = (long long)b * d;
  const long long bytes = maps * h * w * c * 4;
  DOVE_CHECK_ARG(!((const char*)out < (const char*)x + bytes && (const char*)x < (const char*)out + bytes), "dove_dwconv3d_f32: out overlaps x");
  int th, tw;
  dw_tile(h, w, &th, &tw);
  const long long tiles = (long long)((h + th - 1) / th) * ((w + tw - 1) / tw), cblocks = (c / 4 + DW_CB4 - 1) / DW_CB4;
  DOVE_CHECK_ARG(maps <= 0x7fffffffLL && tiles <= 65535 && cblocks <= 65535, "dove_dwconv3d_f32: %lld maps, %lld tiles, %lld channel blocks exceed the grid",
                 maps, tiles, cblocks);
  const int ntw = (w + tw - 1) / tw, threads = (th * DW_CB4 + 63) / 64 * 64;
  const dim3 grid((unsigned)maps, (unsigned)tiles, (unsigned)cblocks);
  const size_t lds = ((size_t)(th + 6) * dw_row_slots(tw) + DW_TAPS * DW_CB4) * sizeof(f32x4);      // at most 48512 bytes
  if (tw == 7)
    hipLaunchKernelGGL(dwconv3d_kernel<7>, grid, dim3(threads), lds, (hipStream_t)stream, x, weight, bias, d, h, w, c, th, ntw, out);
  else
    hipLaunchKernelGGL(dwconv3d_kernel<8>, grid, dim3(threads), lds, (hipStream_t)stream, x, weight, bias, d, h, w, c, th, ntw, out);
  DOVE_CHECK_LAUNCH("dove_dwconv3d_f32");
  return DOVE_OK;
}

extern "C" int dove_vqa_resized_view_f32(const dove_image_view* clip, int frames_in, int h, int w, const int* frames, int t, const int* ytab,
                                         const double* yw, int ymax, const int* xtab, const double* xw, int xmax, int oh, int ow,
                                         const double* mean, const double* std, int cols, float* out, void* stream) {
  DOVE_CHECK_ARG(clip && clip->data && frames && ytab && yw && xtab && xw && mean && std && out,
                 "dove_vqa_resized_view_f32: null clip / data / frames / tap tables / mean / std / out");
  DOVE_CHECK_ARG(clip->dtype >= DOVE_F32 && clip->dtype <= DOVE_U8, "dove_vqa_resized_view_f32: bad dtype %d (0 f32, 1 bf16, 2 u8)", clip->dtype);
  DOVE_CHECK_ARG(frames_in > 0 && h > 0 && w > 0 && t > 0 && oh > 0 && ow > 0 && ymax > 0 && xmax > 0 && ymax <= h && xmax <= w,
                 "dove_vqa_resized_view_f32: frames %d, %d x %d, t %d, view %d x %d, taps %d x %d (positive; no more taps than pixels)", frames_in, h, w, t,
                 oh, ow, ymax, xmax);
  DOVE_CHECK_ARG(oh <= 16384 && ow <= 16384, "dove_vqa_resized_view_f32: a view side above 16384");
  DOVE_CHECK_ARG(!cols || (t % 2 == 0 && oh % 4 == 0 && ow % 4 == 0),
                 "dove_vqa_resized_view_f32: the patch rows need an even t and view sides that are multiples of 4 (t %d, %d x %d)", t, oh, ow);
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = mean[c], nm.std[c] = std[c];
    DOVE_CHECK_ARG(std[c] > 0.0, "dove_vqa_resized_view_f32: std[%d] must be positive", c);
  }
  const long long total = (long long)t * oh * ow;
  DOVE_CHECK_ARG(total < (long long)NT * 0x7fffffffLL, "dove_vqa_resized_view_f32: view too large");
  const Taps ty{ytab, yw, ymax}, tx{xtab, xw, xmax};
  hipLaunchKernelGGL(vqa_resized_view_kernel, dim3(blocks_for(total, NT)), dim3(NT), 0, (hipStream_t)stream, *clip, frames_in, h, w, frames, ty, tx,
                     oh, ow, nm, cols, total, out);
  DOVE_CHECK_LAUNCH("dove_vqa_resized_view_f32");
  return DOVE_OK;
}
