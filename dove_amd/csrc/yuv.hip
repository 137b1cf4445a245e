// 8-bit RGB <-> planar YUV for YUV4MPEG2 video I/O (tests/yuv_ref.py is the bit-exact definition).
//
// Integer fixed point, 16 fractional bits.  The 3x3 matrix arrives as rint(c * 65536) from the host (dove_amd/yuv.py builds the tables
// in one place), so the kernels are matrix-agnostic.  A result is rounded once: + half before the final arithmetic shift, then a clamp
// to 0..255.  Everything fits 32 bits: |coefficient row| sums to < 2^17.2 and the largest scale carried is 2^4 (inverse, 4:2:0), so
// |accumulator| < 255 * 2^17.2 * 16 < 2^31.
//
// rgb_to_yuv: one thread owns 2 luma rows x 8 luma columns, i.e. a whole number of 2x2 chroma blocks: chroma is filtered from the
//   un-rounded products in registers and never goes through memory twice.  With w % 8 == 0 the thread stores 8 bytes of Y per row and
//   4 (4:2:0, 4:2:2) or 8 (4:4:4) bytes per chroma row; other widths take byte stores.  A wave covers 512 consecutive luma columns, so
//   loads of a [3,F,H,W] float clip (16 or 32 bytes per lane and channel row when aligned) and all stores are contiguous across lanes.
//   Float samples are quantised as dove_postprocess_u8 does - trunc(clamp(x * 255, 0, 255)) - so the fused route equals
//   postprocess_u8 followed by the u8 route bit for bit.
// yuv_to_rgb: one thread owns 4 pixels of a row (12 output bytes, three 32-bit stores when w % 4 == 0).  The low-resolution input is
//   1/16 of the clip's data; chroma neighbours are byte loads that hit in cache.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int BW = 8;                     // luma columns per thread (rgb_to_yuv)
constexpr int PW = 4;                     // pixels per thread (yuv_to_rgb)

struct Fmt {
  int c[9];
  int off[3];
};

struct View {
  const void* data;
  int dtype;
  long long sn, sc;
  int sh, sw;                             // inside one (n, c) plane every offset fits 32 bits (checked on the host)
};

__device__ __forceinline__ int quant(float v) { return (int)fminf(fmaxf(v * 255.0f, 0.f), 255.f); }   // dove_postprocess_u8's rule

template <int DT>
__device__ __forceinline__ int load_q(const void* p, long long o) {
  if (DT == DOVE_U8) return ((const uint8_t*)p)[o];
  if (DT == DOVE_BF16) return quant(bf2f(((const bf16_t*)p)[o]));
  return quant(((const float*)p)[o]);
}

__device__ __forceinline__ int clamp_u8(int v) { return min(max(v, 0), 255); }

// q[c][k] = quantised sample of channel c at (y, min(x0 + k, W - 1)): edge replication on the right comes with the load.
// base = offset of (n, 0, y, 0).
template <int DT>
__device__ __forceinline__ void load_block(const View& v, long long base, int x0, int W, int (&q)[3][BW]) {
  const bool full = x0 + BW <= W;
  if (DT == DOVE_U8) {
    const uint8_t* p = (const uint8_t*)v.data + base + (long long)x0 * v.sw;
    if (full && v.sw == 3 && v.sc == 1 && ((uintptr_t)p & 7) == 0) {                  // [F,H,W,3] frames: 24 contiguous bytes
      const uint2 a = ((const uint2*)p)[0], b = ((const uint2*)p)[1], c = ((const uint2*)p)[2];
      const uint32_t wds[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
#pragma unroll
      for (int k = 0; k < BW; ++k)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int byte = k * 3 + ch;
          q[ch][k] = (wds[byte >> 2] >> ((byte & 3) * 8)) & 0xff;
        }
      return;
    }
  } else if (full && v.sw == 1) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const long long o = base + ch * v.sc + x0;
      if (DT == DOVE_BF16) {
        const bf16_t* p = (const bf16_t*)v.data + o;
        if (((uintptr_t)p & 15) == 0) {
          float f[8];
          unpack8(*(const uint4*)p, f);
#pragma unroll
          for (int k = 0; k < BW; ++k) q[ch][k] = quant(f[k]);
        } else {
#pragma unroll
          for (int k = 0; k < BW; ++k) q[ch][k] = quant(bf2f(p[k]));
        }
      } else {
        const float* p = (const float*)v.data + o;
        if (((uintptr_t)p & 15) == 0) {
          const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
          const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
          for (int k = 0; k < BW; ++k) q[ch][k] = quant(f[k]);
        } else {
#pragma unroll
          for (int k = 0; k < BW; ++k) q[ch][k] = quant(p[k]);
        }
      }
    }
    return;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int k = 0; k < BW; ++k) q[ch][k] = load_q<DT>(v.data, base + ch * v.sc + (long long)min(x0 + k, W - 1) * v.sw);
}

// Four values of 0..255 -> one word, by byte selection (v_perm_b32: selector 0-3 = a byte of the second operand, 4-7 = of the first,
// 0x0c = zero).  Only the LOW byte of each value is read.  A shift-and-or form lets the compiler fuse ">> 16, clamp" of two values into
// v_ashr_pk_u8_i32 and or the pair in as if its upper half were zero; on the MI355X that half keeps the register's old bits, which
// showed up as stray bits in every third byte of a word.
__device__ __forceinline__ uint32_t pack4(const int* b) {
  return __builtin_amdgcn_perm((uint32_t)b[1], (uint32_t)b[0], 0x0c0c0400u) | __builtin_amdgcn_perm((uint32_t)b[3], (uint32_t)b[2], 0x04000c0cu);
}

// CNT bytes (4 or 8) to p; VEC: p is CNT-aligned and all CNT are inside the row, else only the first `valid` are stored, one by one
template <int CNT, bool VEC>
__device__ __forceinline__ void store_bytes(uint8_t* p, const int* b, int valid) {
  if (VEC) {
    if (CNT == 8) *(uint2*)p = make_uint2(pack4(b), pack4(b + 4));
    else *(uint32_t*)p = pack4(b);
  } else {
#pragma unroll
    for (int k = 0; k < CNT; ++k)
      if (k < valid) p[k] = (uint8_t)b[k];
  }
}

template <int DT, int CH, bool VEC>
__global__ __launch_bounds__(NT) void rgb_to_yuv_kernel(View v, Fmt f, long long total, int H, int W, int bx, int by,
                                                        uint8_t* __restrict__ out, long long fbytes) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  const int ix = (int)(t % bx), iy = (int)((t / bx) % by);
  const long long fr = t / ((long long)bx * by);
  const int x0 = ix * BW, y0 = iy * 2;
  const int valid = min(BW, W - x0);
  const int cw = CH == DOVE_YUV_444 ? W : (W + 1) / 2;
  const int chh = CH == DOVE_YUV_420 ? (H + 1) / 2 : H;
  uint8_t* Yp = out + fr * fbytes;
  uint8_t* Up = Yp + (long long)H * W;
  uint8_t* Vp = Up + (long long)chh * cw;

  int cu[2][BW], cv[2][BW];               // un-rounded chroma products of the two rows
  int lu[2] = {0, 0}, lv[2] = {0, 0};     // ... and of the pixel left of the block (4:2:2 filter tap)
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = min(y0 + r, H - 1);     // an odd H replicates its last row into the 2x2 mean
    const long long base = fr * v.sn + (long long)y * v.sh;
    int q[3][BW];
    load_block<DT>(v, base, x0, W, q);
    int yy[BW];
#pragma unroll
    for (int k = 0; k < BW; ++k) {
      yy[k] = clamp_u8((f.c[0] * q[0][k] + f.c[1] * q[1][k] + f.c[2] * q[2][k] + (f.off[0] << 16) + (1 << 15)) >> 16);
      cu[r][k] = f.c[3] * q[0][k] + f.c[4] * q[1][k] + f.c[5] * q[2][k];
      cv[r][k] = f.c[6] * q[0][k] + f.c[7] * q[1][k] + f.c[8] * q[2][k];
    }
    if (y0 + r < H) store_bytes<8, VEC>(Yp + (long long)y * W + x0, yy, valid);
    if (CH == DOVE_YUV_422) {
      const long long lo = base + (long long)max(x0 - 1, 0) * v.sw;
      const int r0 = load_q<DT>(v.data, lo), g0 = load_q<DT>(v.data, lo + v.sc), b0 = load_q<DT>(v.data, lo + 2 * v.sc);
      lu[r] = f.c[3] * r0 + f.c[4] * g0 + f.c[5] * b0;
      lv[r] = f.c[6] * r0 + f.c[7] * g0 + f.c[8] * b0;
    }
  }
  if (CH == DOVE_YUV_MONO) return;
  const int ou16 = (f.off[1] << 16) + (1 << 15), ov16 = (f.off[2] << 16) + (1 << 15);
  const int ou18 = (f.off[1] << 18) + (1 << 17), ov18 = (f.off[2] << 18) + (1 << 17);
  if (CH == DOVE_YUV_444) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (y0 + r >= H) break;
      int u[BW], w[BW];
#pragma unroll
      for (int k = 0; k < BW; ++k) {
        u[k] = clamp_u8((cu[r][k] + ou16) >> 16);
        w[k] = clamp_u8((cv[r][k] + ov16) >> 16);
      }
      const long long o = (long long)(y0 + r) * W + x0;
      store_bytes<8, VEC>(Up + o, u, valid);
      store_bytes<8, VEC>(Vp + o, w, valid);
    }
  } else if (CH == DOVE_YUV_422) {
    const int cvalid = (valid + 1) / 2;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (y0 + r >= H) break;
      int u[BW / 2], w[BW / 2];
#pragma unroll
      for (int j = 0; j < BW / 2; ++j) {    // [1 2 1] at even x; columns past W - 1 hold the replicated edge already
        const int ul = j == 0 ? lu[r] : cu[r][2 * j - 1], vl = j == 0 ? lv[r] : cv[r][2 * j - 1];
        u[j] = clamp_u8((ul + 2 * cu[r][2 * j] + cu[r][2 * j + 1] + ou18) >> 18);
        w[j] = clamp_u8((vl + 2 * cv[r][2 * j] + cv[r][2 * j + 1] + ov18) >> 18);
      }
      const long long o = (long long)(y0 + r) * cw + x0 / 2;
      store_bytes<4, VEC>(Up + o, u, cvalid);
      store_bytes<4, VEC>(Vp + o, w, cvalid);
    }
  } else {
    const int cvalid = (valid + 1) / 2;
    int u[BW / 2], w[BW / 2];
#pragma unroll
    for (int j = 0; j < BW / 2; ++j) {
      u[j] = clamp_u8((cu[0][2 * j] + cu[0][2 * j + 1] + cu[1][2 * j] + cu[1][2 * j + 1] + ou18) >> 18);
      w[j] = clamp_u8((cv[0][2 * j] + cv[0][2 * j + 1] + cv[1][2 * j] + cv[1][2 * j + 1] + ov18) >> 18);
    }
    const long long o = (long long)iy * cw + x0 / 2;
    store_bytes<4, VEC>(Up + o, u, cvalid);
    store_bytes<4, VEC>(Vp + o, w, cvalid);
  }
}

template <int CH, bool CENTRE_H, bool VEC>
__global__ __launch_bounds__(NT) void yuv_to_rgb_kernel(const uint8_t* __restrict__ yuv, Fmt f, long long total, int H, int W, int bx,
                                                        long long fbytes, uint8_t* __restrict__ out) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  const int ix = (int)(t % bx), y = (int)((t / bx) % H);
  const long long fr = t / ((long long)bx * H);
  const int x0 = ix * PW;
  const int valid = min(PW, W - x0);
  const int cw = CH == DOVE_YUV_444 ? W : (W + 1) / 2;
  const int chh = CH == DOVE_YUV_420 ? (H + 1) / 2 : H;
  const uint8_t* Yp = yuv + fr * fbytes;
  const uint8_t* Up = Yp + (long long)H * W;
  const uint8_t* Vp = Up + (long long)chh * cw;
  constexpr int S = CH == DOVE_YUV_420 ? 4 : CH == DOVE_YUV_422 ? 2 : 0;     // the upsampled chroma carries 2^S

  int yy[PW];
  if (VEC) {
    const uint32_t wd = *(const uint32_t*)(Yp + (long long)y * W + x0);
#pragma unroll
    for (int k = 0; k < PW; ++k) yy[k] = (wd >> (8 * k)) & 0xff;
  } else {
#pragma unroll
    for (int k = 0; k < PW; ++k) yy[k] = Yp[(long long)y * W + min(x0 + k, W - 1)];
  }
  // chroma rows: 4:2:0 is centre-sited vertically in every variant - 3:1 towards the nearer row, the other one clamped
  const int j = CH == DOVE_YUV_420 ? y >> 1 : y;
  const int oj = CH == DOVE_YUV_420 ? min(max((y & 1) ? j + 1 : j - 1, 0), chh - 1) : j;
  int rgb[PW * 3];
#pragma unroll
  for (int k = 0; k < PW; ++k) {
    const int x = min(x0 + k, W - 1);
    int r, g, b;
    if (CH == DOVE_YUV_MONO) {
      r = g = b = clamp_u8((f.c[0] * (yy[k] - f.off[0]) + (1 << 15)) >> 16);
    } else {
      int us, vs;
      if (CH == DOVE_YUV_444) {
        us = Up[(long long)y * W + x];
        vs = Vp[(long long)y * W + x];
      } else {
        const int i = x >> 1;
        int o, wa, wb;
        if (CH == DOVE_YUV_420 && CENTRE_H) {
          o = min(max((x & 1) ? i + 1 : i - 1, 0), cw - 1);
          wa = 3;
          wb = 1;
        } else {                             // left co-sited: even x sits on sample i, odd x half way to i + 1
          o = min(i + 1, cw - 1);
          wa = (x & 1) ? 2 : 4;
          wb = 4 - wa;
        }
        const long long ra = (long long)j * cw;
        us = wa * Up[ra + i] + wb * Up[ra + o];
        vs = wa * Vp[ra + i] + wb * Vp[ra + o];
        if (CH == DOVE_YUV_420) {
          const long long rb = (long long)oj * cw;
          us = 3 * us + wa * Up[rb + i] + wb * Up[rb + o];
          vs = 3 * vs + wa * Vp[rb + i] + wb * Vp[rb + o];
        }
      }
      const int ys = (yy[k] - f.off[0]) * (1 << S), ud = us - f.off[1] * (1 << S), vd = vs - f.off[2] * (1 << S);
      r = clamp_u8((f.c[0] * ys + f.c[1] * ud + f.c[2] * vd + (1 << (15 + S))) >> (16 + S));
      g = clamp_u8((f.c[3] * ys + f.c[4] * ud + f.c[5] * vd + (1 << (15 + S))) >> (16 + S));
      b = clamp_u8((f.c[6] * ys + f.c[7] * ud + f.c[8] * vd + (1 << (15 + S))) >> (16 + S));
    }
    rgb[k * 3] = r;
    rgb[k * 3 + 1] = g;
    rgb[k * 3 + 2] = b;
  }
  uint8_t* o = out + (((long long)fr * H + y) * W + x0) * 3;
  if (VEC) {
    ((uint32_t*)o)[0] = pack4(rgb);
    ((uint32_t*)o)[1] = pack4(rgb + 4);
    ((uint32_t*)o)[2] = pack4(rgb + 8);
  } else {
#pragma unroll
    for (int k = 0; k < PW * 3; ++k)
      if (k < valid * 3) o[k] = (uint8_t)rgb[k];
  }
}

bool plane_fits(const dove_image_view* v, int h, int w) {
  const long long lim = 1LL << 31, ah = v->sh < 0 ? -v->sh : v->sh, aw = v->sw < 0 ? -v->sw : v->sw;
  return ah < lim && aw < lim && (h - 1) * ah + (w - 1) * aw < lim;
}

bool good_chroma(int c) { return c == DOVE_YUV_444 || c == DOVE_YUV_422 || c == DOVE_YUV_420 || c == DOVE_YUV_MONO; }

// the 32-bit accumulators hold |coef| <= 2^18 per entry (the largest real one is 2.12 * 65536) and offsets of 0..255
bool good_format(const dove_yuv_format* f) {
  for (int i = 0; i < 9; ++i)
    if (f->coef[i] > (1 << 18) || f->coef[i] < -(1 << 18)) return false;
  for (int i = 0; i < 3; ++i)
    if (f->offset[i] < 0 || f->offset[i] > 255) return false;
  return true;
}

Fmt make_fmt(const dove_yuv_format* f) {
  Fmt m;
  for (int i = 0; i < 9; ++i) m.c[i] = f->coef[i];
  for (int i = 0; i < 3; ++i) m.off[i] = f->offset[i];
  return m;
}

template <int DT, int CH>
void launch_fwd(bool vec, unsigned blocks, hipStream_t st, const View& v, const Fmt& f, long long total, int h, int w, int bx, int by,
                uint8_t* out, long long fbytes) {
  if (vec) hipLaunchKernelGGL((rgb_to_yuv_kernel<DT, CH, true>), dim3(blocks), dim3(NT), 0, st, v, f, total, h, w, bx, by, out, fbytes);
  else hipLaunchKernelGGL((rgb_to_yuv_kernel<DT, CH, false>), dim3(blocks), dim3(NT), 0, st, v, f, total, h, w, bx, by, out, fbytes);
}

template <int DT>
void launch_fwd_dt(int chroma, bool vec, unsigned blocks, hipStream_t st, const View& v, const Fmt& f, long long total, int h, int w,
                   int bx, int by, uint8_t* out, long long fbytes) {
  switch (chroma) {
    case DOVE_YUV_444: launch_fwd<DT, DOVE_YUV_444>(vec, blocks, st, v, f, total, h, w, bx, by, out, fbytes); break;
    case DOVE_YUV_422: launch_fwd<DT, DOVE_YUV_422>(vec, blocks, st, v, f, total, h, w, bx, by, out, fbytes); break;
    case DOVE_YUV_420: launch_fwd<DT, DOVE_YUV_420>(vec, blocks, st, v, f, total, h, w, bx, by, out, fbytes); break;
    default: launch_fwd<DT, DOVE_YUV_MONO>(vec, blocks, st, v, f, total, h, w, bx, by, out, fbytes); break;
  }
}

template <int CH, bool CENTRE_H>
void launch_inv(bool vec, unsigned blocks, hipStream_t st, const uint8_t* yuv, const Fmt& f, long long total, int h, int w, int bx,
                long long fbytes, uint8_t* out) {
  if (vec) hipLaunchKernelGGL((yuv_to_rgb_kernel<CH, CENTRE_H, true>), dim3(blocks), dim3(NT), 0, st, yuv, f, total, h, w, bx, fbytes, out);
  else hipLaunchKernelGGL((yuv_to_rgb_kernel<CH, CENTRE_H, false>), dim3(blocks), dim3(NT), 0, st, yuv, f, total, h, w, bx, fbytes, out);
}

}  // namespace

extern "C" size_t dove_yuv_frame_bytes(int h, int w, int chroma) {
  if (h <= 0 || w <= 0 || !good_chroma(chroma)) return 0;
  const size_t luma = (size_t)h * w, cw = ((size_t)w + 1) / 2, ch = ((size_t)h + 1) / 2;
  if (chroma == DOVE_YUV_444) return 3 * luma;
  if (chroma == DOVE_YUV_422) return luma + 2 * (size_t)h * cw;
  if (chroma == DOVE_YUV_420) return luma + 2 * ch * cw;
  return luma;
}

extern "C" int dove_rgb_to_yuv_u8(const dove_image_view* rgb, int n, int h, int w, const dove_yuv_format* fmt, void* out, void* stream) {
  DOVE_CHECK_ARG(rgb && fmt, "rgb_to_yuv: null view or format");
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0, "rgb_to_yuv: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(good_chroma(fmt->chroma), "rgb_to_yuv: bad chroma %d (0 444, 1 422, 2 420, 3 mono)", fmt->chroma);
  DOVE_CHECK_ARG(good_format(fmt), "rgb_to_yuv: coefficients must be within +-2^18 and offsets within 0..255");
  DOVE_CHECK_ARG(rgb->dtype == DOVE_F32 || rgb->dtype == DOVE_BF16 || rgb->dtype == DOVE_U8, "rgb_to_yuv: bad dtype %d (0 f32, 1 bf16, 2 u8)",
                 rgb->dtype);
  DOVE_CHECK_ARG(plane_fits(rgb, h, w), "rgb_to_yuv: one %d x %d plane of the view spans 2^31 elements or more", h, w);
  const int bx = (w + BW - 1) / BW, by = (h + 1) / 2;
  const long long total = (long long)n * bx * by, blocks = (total + NT - 1) / NT;
  DOVE_CHECK_ARG(blocks < (1LL << 31), "rgb_to_yuv: n=%d frames of %d x %d exceed one launch", n, h, w);
  DOVE_CHECK_ARG(rgb->data && out, "rgb_to_yuv: null pointer");
  const View v{rgb->data, rgb->dtype, rgb->sn, rgb->sc, (int)rgb->sh, (int)rgb->sw};
  const Fmt f = make_fmt(fmt);
  const long long fbytes = (long long)dove_yuv_frame_bytes(h, w, fmt->chroma);
  const bool vec = w % BW == 0 && ((uintptr_t)out & 7) == 0;          // then every plane row and every frame starts 8-byte aligned
  hipStream_t st = (hipStream_t)stream;
  if (rgb->dtype == DOVE_U8) launch_fwd_dt<DOVE_U8>(fmt->chroma, vec, (unsigned)blocks, st, v, f, total, h, w, bx, by, (uint8_t*)out, fbytes);
  else if (rgb->dtype == DOVE_BF16) launch_fwd_dt<DOVE_BF16>(fmt->chroma, vec, (unsigned)blocks, st, v, f, total, h, w, bx, by, (uint8_t*)out, fbytes);
  else launch_fwd_dt<DOVE_F32>(fmt->chroma, vec, (unsigned)blocks, st, v, f, total, h, w, bx, by, (uint8_t*)out, fbytes);
  DOVE_CHECK_LAUNCH("dove_rgb_to_yuv_u8");
  return DOVE_OK;
}

extern "C" int dove_yuv_to_rgb_u8(const void* yuv, int n, int h, int w, const dove_yuv_format* fmt, void* out, void* stream) {
  DOVE_CHECK_ARG(fmt, "yuv_to_rgb: null format");
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0, "yuv_to_rgb: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(good_chroma(fmt->chroma), "yuv_to_rgb: bad chroma %d (0 444, 1 422, 2 420, 3 mono)", fmt->chroma);
  DOVE_CHECK_ARG(fmt->siting_h == DOVE_YUV_SITING_LEFT || fmt->siting_h == DOVE_YUV_SITING_CENTRE, "yuv_to_rgb: bad siting_h %d (0 left, 1 centre)",
                 fmt->siting_h);
  DOVE_CHECK_ARG(good_format(fmt), "yuv_to_rgb: coefficients must be within +-2^18 and offsets within 0..255");
  const int bx = (w + PW - 1) / PW;
  const long long total = (long long)n * bx * h, blocks = (total + NT - 1) / NT;
  DOVE_CHECK_ARG(blocks < (1LL << 31), "yuv_to_rgb: n=%d frames of %d x %d exceed one launch", n, h, w);
  DOVE_CHECK_ARG(yuv && out, "yuv_to_rgb: null pointer");
  const Fmt f = make_fmt(fmt);
  const long long fbytes = (long long)dove_yuv_frame_bytes(h, w, fmt->chroma);
  const bool vec = w % PW == 0 && fbytes % 4 == 0 && ((uintptr_t)yuv & 3) == 0 && ((uintptr_t)out & 3) == 0;
  const uint8_t* src = (const uint8_t*)yuv;
  uint8_t* dst = (uint8_t*)out;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)blocks;
  switch (fmt->chroma) {
    case DOVE_YUV_444: launch_inv<DOVE_YUV_444, false>(vec, nb, st, src, f, total, h, w, bx, fbytes, dst); break;
    case DOVE_YUV_422: launch_inv<DOVE_YUV_422, false>(vec, nb, st, src, f, total, h, w, bx, fbytes, dst); break;
    case DOVE_YUV_420:
      if (fmt->siting_h == DOVE_YUV_SITING_CENTRE) launch_inv<DOVE_YUV_420, true>(vec, nb, st, src, f, total, h, w, bx, fbytes, dst);
      else launch_inv<DOVE_YUV_420, false>(vec, nb, st, src, f, total, h, w, bx, fbytes, dst);
      break;
    default: launch_inv<DOVE_YUV_MONO, false>(vec, nb, st, src, f, total, h, w, bx, fbytes, dst); break;
  }
  DOVE_CHECK_LAUNCH("dove_yuv_to_rgb_u8");
  return DOVE_OK;
}
