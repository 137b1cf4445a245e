// FasterVQA / FAST-VQA (include/dove_hip.h has the contract): what a Video Swin-T with gated relative position bias needs
// beside the Linears (dove_resnet_conv_f32's 1 x 1 walk with tokens as pixels), dove_layernorm_f32 and dove_gelu_f32.  Activations are
// channels-last fp32 token maps [B][D][H][W][C]; no atomics; repeated calls give identical bits; a sample's values do not depend on the
// batch it is in (every sum below belongs to one (window, head) problem or one clip).
//
// vqa_fragments_kernel: one thread per output pixel.  Output pixel (t, y, x) of the fragment canvas [T][gh fh][gw fw] is source pixel
//   (offsets[i][j][g] + (y % fh, x % fw)) of frame frames[t], with (i, j) = (y / fh, x / fw) and g = t / frames_per_group; coordinates are
//   clamped into the clip, so a bad table cannot read outside it.  Value: (X - mean_c) / std_c in fp64 without contraction, rounded once,
//   with X the u8 value itself, or 255.0 v for f32 / bf16.  cols = 0 writes the canvas [T][Hc][Wc][3]; cols = 1 writes the same values as the
//   rows of the (2, 4, 4)-stride-(2, 4, 4) patch embedding's GEMM: row ((t / 2) Hc / 4 + y / 4) Wc / 4 + x / 4, column c 32 + (t % 2) 16 +
//   (y % 4) 4 + x % 4, the order of a flattened Conv3d weight [out][3][2][4][4].
// swin3d_window_gather_kernel / swin3d_window_scatter_kernel: one thread per four channels.  The padded map is [Dp][Hp][Wp] (multiples of the
//   window); window token (window a, slot n) sits at padded position p = a * window + n per axis and reads map position (p + shift) % padded
//   (torch.roll by -shift), zero where that lies in the pad.  The scatter is the inverse on the D x H x W crop, plus the shortcut.
// swin3d_patch_merge_kernel: out[b][d][h2][w2][j C + c] = x[b][d][2 h2 + (j & 1)][2 w2 + (j >> 1)][c], zero outside the map.
// swin3d_window_attention_kernel: one workgroup per (window, head), head width 32, any window length N <= 392, fp32 on
//   v_mfma_f32_32x32x2_f32.  K (padded to 33 dwords per row) and V of the window, and the window's per-token fragment and shift-region ids,
//   stay in LDS.  A wave owns tiles of 32 query rows.  Per tile of 32 keys it computes S^T = K Q^T (keys down, queries across: a lane holds
//   one query and 16 of the 32 keys), s = (q . k) scale + table[index[query][key]][head] (table_b where the two tokens' fragment ids differ
//   and table_b is given) + (-100 where their region ids differ); keys >= N score -inf.  The head's column of each table is staged in LDS
//   too and the second table is reached by adding its offset to the index: the choice between the tables is integer arithmetic per lane.  (A
//   per-lane choice between the two table POINTERS was compiled, by the hipcc of ROCm 7.0, into one wave-wide pointer for 15 of the 16 score
//   registers, found as a wrong result on the GPU; the LDS copy also turns two global gathers per score into one.)
//   The softmax is the two-pass one: pass 1 walks every key tile for the true row maximum, pass 2 recomputes the scores (the same instructions, the same bits), p = expf(s - max) with the
//   accurate expf, the row sum in key-tile order (registers ascending, then the other half-wave), and O^T += V^T P^T with P^T in registers.
//   out = O / sum.  Nothing of size N x N is stored.
// vqa_head_kernel: one 1024-thread block per clip, fp64.  A wave owns tokens w, w + 16, ...: per token and hidden unit j, a_j = w1_j . f + b1_j
//   (lane c, c + 64, ..., fixed butterfly), score = sum_j w2_j gelu(a_j) (exact erf, j ascending) + b2; the wave adds its tokens in order, the
//   16 partials are added in wave order and divided by the token count.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int WA_D = 32, WA_T = 32, WA_LDK = WA_D + 1, WA_MAX_N = 392, WA_MAX_WAVES = 4, WA_MAX_LDS = 160 * 1024;
constexpr int HEAD_NT = 1024, HEAD_MAX_HID = 256;

inline unsigned blocks_for(long long total, int nt) { return (unsigned)((total + nt - 1) / nt); }

struct Norm3 {
  double mean[3], std[3];
};

struct WinGeo {
  int D, H, W, C, wd, wh, ww, sd, sh, sw, Dp, Hp, Wp;
};

// --------------------------------------------------------------- fragment gather ---------------------------------------------------------------
__device__ __forceinline__ double normalised(double x, double mean, double std) {
#pragma clang fp contract(off)
  return (x - mean) / std;
}

__global__ __launch_bounds__(NT) void vqa_fragments_kernel(dove_image_view v, int F, int H, int W, const int* __restrict__ frames,
                                                           const int* __restrict__ offsets, int gh, int gw, int fh, int fw, int tg, int fpg,
                                                           Norm3 nm, int cols, long long total, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int Hc = gh * fh, Wc = gw * fw;
  const int x = (int)(idx % Wc), y = (int)((idx / Wc) % Hc), t = (int)(idx / ((long long)Wc * Hc));
  const int i = y / fh, j = x / fw, g = min(t / fpg, tg - 1);
  const int* o = offsets + ((long long)(i * gw + j) * tg + g) * 2;
  const int sy = min(max(o[0] + y % fh, 0), H - 1), sx = min(max(o[1] + x % fw, 0), W - 1), f = min(max(frames[t], 0), F - 1);
  const long long base = (long long)f * v.sn + (long long)sy * v.sh + (long long)sx * v.sw;
  float r[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long off = base + c * v.sc;
    double X;
    if (v.dtype == DOVE_U8) X = (double)((const uint8_t*)v.data)[off];
    else if (v.dtype == DOVE_BF16) X = 255.0 * (double)bf2f(((const bf16_t*)v.data)[off]);
    else X = 255.0 * (double)((const float*)v.data)[off];
    r[c] = (float)normalised(X, nm.mean[c], nm.std[c]);
  }
  if (!cols) {
    float* p = out + idx * 3;
    p[0] = r[0];
    p[1] = r[1];
    p[2] = r[2];
  } else {
    const long long row = ((long long)(t >> 1) * (Hc >> 2) + (y >> 2)) * (Wc >> 2) + (x >> 2);
    float* p = out + row * 96 + (t & 1) * 16 + (y & 3) * 4 + (x & 3);
    p[0] = r[0];
    p[32] = r[1];
    p[64] = r[2];
  }
}

// ------------------------------------------------------- window partition and its inverse -------------------------------------------------------
__global__ __launch_bounds__(NT) void swin3d_window_gather_kernel(const float* __restrict__ x, WinGeo g, long long total,
                                                                  float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int C4 = g.C >> 2, N = g.wd * g.wh * g.ww, nh = g.Hp / g.wh, nw = g.Wp / g.ww, nW = (g.Dp / g.wd) * nh * nw;
  const int c4 = (int)(idx % C4), n = (int)((idx / C4) % N), a = (int)((idx / ((long long)C4 * N)) % nW);
  const long long b = idx / ((long long)C4 * N * nW);
  const int pd = ((a / (nh * nw)) * g.wd + n / (g.wh * g.ww) + g.sd) % g.Dp;
  const int ph = (((a / nw) % nh) * g.wh + (n / g.ww) % g.wh + g.sh) % g.Hp;
  const int pw = ((a % nw) * g.ww + n % g.ww + g.sw) % g.Wp;
  f32x4 val = {0.f, 0.f, 0.f, 0.f};
  if (pd < g.D && ph < g.H && pw < g.W) val = *(const f32x4*)(x + ((((b * g.D + pd) * g.H + ph) * g.W + pw) * g.C + 4 * c4));
  *(f32x4*)(out + idx * 4) = val;
}

__global__ __launch_bounds__(NT) void swin3d_window_scatter_kernel(const float* __restrict__ win, const float* shortcut, WinGeo g,
                                                                   long long total, float* out) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int C4 = g.C >> 2, N = g.wd * g.wh * g.ww, nh = g.Hp / g.wh, nw = g.Wp / g.ww, nW = (g.Dp / g.wd) * nh * nw;
  const int c4 = (int)(idx % C4), w = (int)((idx / C4) % g.W), h = (int)((idx / ((long long)C4 * g.W)) % g.H);
  const int d = (int)((idx / ((long long)C4 * g.W * g.H)) % g.D);
  const long long b = idx / ((long long)C4 * g.W * g.H * g.D);
  const int pd = (d - g.sd + g.Dp) % g.Dp, ph = (h - g.sh + g.Hp) % g.Hp, pw = (w - g.sw + g.Wp) % g.Wp;
  const int a = ((pd / g.wd) * nh + ph / g.wh) * nw + pw / g.ww, n = ((pd % g.wd) * g.wh + ph % g.wh) * g.ww + pw % g.ww;
  const f32x4 t = *(const f32x4*)(win + ((b * nW + a) * N + n) * g.C + 4 * c4);
  const f32x4 s = *(const f32x4*)(shortcut + idx * 4);
  const f32x4 r = {s[0] + t[0], s[1] + t[1], s[2] + t[2], s[3] + t[3]};
  *(f32x4*)(out + idx * 4) = r;
}

__global__ __launch_bounds__(NT) void swin3d_patch_merge_kernel(const float* __restrict__ x, int H, int W, int C, long long total,
                                                                float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int C4 = C >> 2, H2 = (H + 1) >> 1, W2 = (W + 1) >> 1;
  const int c4 = (int)(idx % C4), j = (int)((idx / C4) & 3), w2 = (int)((idx / (4LL * C4)) % W2), h2 = (int)((idx / (4LL * C4 * W2)) % H2);
  const long long bd = idx / (4LL * C4 * W2 * H2);
  const int h = 2 * h2 + (j & 1), w = 2 * w2 + (j >> 1);
  f32x4 val = {0.f, 0.f, 0.f, 0.f};
  if (h < H && w < W) val = *(const f32x4*)(x + ((bd * H + h) * W + w) * C + 4 * c4);
  *(f32x4*)(out + idx * 4) = val;
}

// --------------------------------------------------------------- window attention ---------------------------------------------------------------
struct WaArgs {
  const float *q, *k, *v;
  long long ld;
  int N, heads;
  float scale;
  const float *table_a, *table_b;
  int table_rows;
  const int *index, *frag, *region;
  int id_windows;
  float* out;
  long long ldo;
};

__global__ __launch_bounds__(WA_MAX_WAVES * 64) void swin3d_window_attention_kernel(WaArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int N = p.N, Npad = (N + WA_T - 1) / WA_T * WA_T;
  float* Ks = smem;
  float* Vs = Ks + Npad * WA_LDK;
  int* fragS = (int*)(Vs + Npad * WA_D);
  int* regS = fragS + Npad;
  float* tabS = (float*)(regS + Npad);               // this head's column of table_a, then of table_b
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5, nwaves = blockDim.x >> 6;
  const int head = blockIdx.y, col0 = head * WA_D;
  const long long base = (long long)blockIdx.x * N;
  const long long idw = (long long)(blockIdx.x % p.id_windows) * N;

  for (int e = tid; e < Npad * (WA_D / 4); e += blockDim.x) {
    const int row = e >> 3, c4 = (e & 7) * 4;
    f32x4 kk = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
    if (row < N) {
      const long long off = (base + row) * p.ld + col0 + c4;
      kk = *(const f32x4*)(p.k + off);
      vv = *(const f32x4*)(p.v + off);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) Ks[row * WA_LDK + c4 + i] = kk[i];
    *(f32x4*)(Vs + row * WA_D + c4) = vv;
  }
  for (int row = tid; row < Npad; row += blockDim.x) {
    fragS[row] = (p.frag && row < N) ? p.frag[idw + row] : 0;
    regS[row] = (p.region && row < N) ? p.region[idw + row] : 0;
  }
  const int second = p.table_b ? p.table_rows : 0;   // where the second table's column starts; 0: every pair reads the first
  for (int i = tid; i < p.table_rows; i += blockDim.x) {
    tabS[i] = p.table_a[(long long)i * p.heads + head];
    if (second) tabS[second + i] = p.table_b[(long long)i * p.heads + head];
  }
  __syncthreads();

  const int tiles = Npad / WA_T;
  for (int qt = wave; qt < tiles; qt += nwaves) {   // wave-uniform: every lane of a wave issues the same MFMAs
    const int qrow = qt * WA_T + l31, qr = min(qrow, N - 1);
    float qf[WA_D / 2];                              // Q[qrow][2 s + half]: the B operand of S^T = K Q^T
    {
      const float* qp = p.q + (base + qr) * p.ld + col0 + half;
#pragma unroll
      for (int s = 0; s < WA_D / 2; ++s) qf[s] = qrow < N ? qp[2 * s] : 0.f;
    }
    const int fq = fragS[qr], rq = regS[qr];
    const int* irow = p.index + (long long)qr * N;

    // this lane: query l31 of the tile, keys kt 32 + (r & 3) + 8 (r >> 2) + 4 half
    auto scores = [&](int kt) {
      f32x16 sa;
#pragma unroll
      for (int r = 0; r < 16; ++r) sa[r] = 0.f;
      const float* kp = Ks + (kt * WA_T + l31) * WA_LDK + half;
#pragma unroll
      for (int s = 0; s < WA_D / 2; ++s) sa = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * s], qf[s], sa, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * WA_T + (r & 3) + 8 * (r >> 2) + 4 * half;
        float s = -INFINITY;
        if (key < N) {
          const int id = min(max(irow[key], 0), p.table_rows - 1);
          const int other = fragS[key] != fq;        // the choice is arithmetic on the index, never a choice between two pointers
          s = sa[r] * p.scale + tabS[id + other * second];
          if (regS[key] != rq) s += -100.f;
        }
        sa[r] = s;
      }
      return sa;
    };

    float mx = -INFINITY;
    for (int kt = 0; kt < tiles; ++kt) {
      const f32x16 sa = scores(kt);
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sa[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));              // finite: key 0 exists and the mask is finite

    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    float sum = 0.f;
    for (int kt = 0; kt < tiles; ++kt) {
      f32x16 sa = scores(kt);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sa[r] = expf(sa[r] - mx);
        sum += sa[r];
      }
      // O^T[d][query] += V^T[d][key] P^T[key][query]: the two keys of step r are this half's and the other half's register r
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* vp = Vs + (kt * WA_T + (r & 3) + 8 * (r >> 2) + 4 * half) * WA_D + l31;
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[0], sa[r], o, 0, 0, 0);
      }
    }
    sum += __shfl_xor(sum, 32);
    if (qrow < N) {
      float* op = p.out + (base + qrow) * p.ldo + col0 + 4 * half;
#pragma unroll
      for (int g = 0; g < 4; ++g) {                  // d = 8 g + 4 half + (0 .. 3)
        const f32x4 a = {o[4 * g] / sum, o[4 * g + 1] / sum, o[4 * g + 2] / sum, o[4 * g + 3] / sum};
        *(f32x4*)(op + 8 * g) = a;
      }
    }
  }
}

// --------------------------------------------------------------------- head ---------------------------------------------------------------------
__global__ __launch_bounds__(HEAD_NT) void vqa_head_kernel(const float* __restrict__ feat, long long ld, int tokens, int dim,
                                                           const float* __restrict__ w1, const float* __restrict__ b1, int hid,
                                                           const float* __restrict__ w2, const float* __restrict__ b2, double* __restrict__ out) {
  __shared__ double part[HEAD_NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* clip = feat + (long long)blockIdx.x * tokens * ld;
  double acc = 0.0;
  for (int t = wave; t < tokens; t += HEAD_NT / 64) {
    const float* f = clip + (long long)t * ld;
    double score = 0.0;
    for (int j = 0; j < hid; ++j) {
      double s = 0.0;
      for (int c = lane; c < dim; c += 64) s += (double)w1[(long long)j * dim + c] * (double)f[c];
      const double a = wave_sum_f64(s) + (double)b1[j];
      score += (double)w2[j] * (0.5 * a * (1.0 + erf(a * 0.70710678118654752440)));
    }
    acc += score + (double)b2[0];
  }
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < HEAD_NT / 64; ++w) s += part[w];
    out[blockIdx.x] = s / (double)tokens;
  }
}

int check_geo(const char* what, const int* dims, const int* window, const int* shift, int c, WinGeo* g) {
  DOVE_CHECK_ARG(dims && window && shift, "%s: null dims / window / shift", what);
  g->D = dims[0], g->H = dims[1], g->W = dims[2], g->C = c;
  g->wd = window[0], g->wh = window[1], g->ww = window[2];
  g->sd = shift[0], g->sh = shift[1], g->sw = shift[2];
  DOVE_CHECK_ARG(g->D > 0 && g->H > 0 && g->W > 0 && c > 0 && c % 4 == 0, "%s: map %d x %d x %d, c %d (positive, c a multiple of 4)", what, g->D,
                 g->H, g->W, c);
  DOVE_CHECK_ARG(g->wd > 0 && g->wh > 0 && g->ww > 0 && g->sd >= 0 && g->sd < g->wd && g->sh >= 0 && g->sh < g->wh && g->sw >= 0 && g->sw < g->ww,
                 "%s: window %d x %d x %d, shift %d, %d, %d (0 <= shift < window)", what, g->wd, g->wh, g->ww, g->sd, g->sh, g->sw);
  g->Dp = (g->D + g->wd - 1) / g->wd * g->wd;
  g->Hp = (g->H + g->wh - 1) / g->wh * g->wh;
  g->Wp = (g->W + g->ww - 1) / g->ww * g->ww;
  return DOVE_OK;
}

}  // namespace

// ------------------------------------------------------------- C entries -------------------------------------------------------------
extern "C" int dove_vqa_fragments_f32(const dove_image_view* clip, int frames_in, int h, int w, const int* frames, int t, const int* offsets,
                                      int gh, int gw, int fh, int fw, int t_groups, const double* mean, const double* std, int cols, float* out,
                                      void* stream) {
  DOVE_CHECK_ARG(clip && clip->data && frames && offsets && mean && std && out, "dove_vqa_fragments_f32: null clip / data / frames / offsets / mean / std / out");
  DOVE_CHECK_ARG(clip->dtype >= DOVE_F32 && clip->dtype <= DOVE_U8, "dove_vqa_fragments_f32: bad dtype %d (0 f32, 1 bf16, 2 u8)", clip->dtype);
  DOVE_CHECK_ARG(frames_in > 0 && h > 0 && w > 0 && t > 0 && gh > 0 && gw > 0 && fh > 0 && fw > 0 && t_groups > 0 && t % t_groups == 0,
                 "dove_vqa_fragments_f32: frames %d, %d x %d, t %d, grid %d x %d of %d x %d, t_groups %d (positive; t a multiple of t_groups)",
                 frames_in, h, w, t, gh, gw, fh, fw, t_groups);
  DOVE_CHECK_ARG((long long)gh * fh <= 16384 && (long long)gw * fw <= 16384, "dove_vqa_fragments_f32: a canvas side above 16384");
  DOVE_CHECK_ARG(!cols || (t % 2 == 0 && (gh * fh) % 4 == 0 && (gw * fw) % 4 == 0),
                 "dove_vqa_fragments_f32: the patch rows need an even t and canvas sides that are multiples of 4 (t %d, %d x %d)", t, gh * fh, gw * fw);
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = mean[c], nm.std[c] = std[c];
    DOVE_CHECK_ARG(std[c] > 0.0, "dove_vqa_fragments_f32: std[%d] must be positive", c);
  }
  const long long total = (long long)t * gh * fh * gw * fw;
  DOVE_CHECK_ARG(total < (long long)NT * 0x7fffffffLL, "dove_vqa_fragments_f32: clip too large");
  hipLaunchKernelGGL(vqa_fragments_kernel, dim3(blocks_for(total, NT)), dim3(NT), 0, (hipStream_t)stream, *clip, frames_in, h, w, frames, offsets,
                     gh, gw, fh, fw, t_groups, t / t_groups, nm, cols, total, out);
  DOVE_CHECK_LAUNCH("dove_vqa_fragments_f32");
  return DOVE_OK;
}

extern "C" int dove_swin3d_window_gather_f32(const float* x, int b, const int* dims, int c, const int* window, const int* shift, float* out,
                                             void* stream) {
  WinGeo g;
  if (int rc = check_geo("dove_swin3d_window_gather_f32", dims, window, shift, c, &g)) return rc;
  DOVE_CHECK_ARG(x && out && x != out && b > 0, "dove_swin3d_window_gather_f32: null or aliased x / out, or b %d", b);
  DOVE_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "dove_swin3d_window_gather_f32: x and out must be 16-byte aligned");
  const long long total = (long long)b * g.Dp * g.Hp * g.Wp * (c / 4);
  DOVE_CHECK_ARG(total < (long long)NT * 0x7fffffffLL, "dove_swin3d_window_gather_f32: batch too large");
  hipLaunchKernelGGL(swin3d_window_gather_kernel, dim3(blocks_for(total, NT)), dim3(NT), 0, (hipStream_t)stream, x, g, total, out);
  DOVE_CHECK_LAUNCH("dove_swin3d_window_gather_f32");
  return DOVE_OK;
}

extern "C" int dove_swin3d_window_scatter_f32(const float* windows, const float* shortcut, int b, const int* dims, int c, const int* window,
                                              const int* shift, float* out, void* stream) {
  WinGeo g;
  if (int rc = check_geo("dove_swin3d_window_scatter_f32", dims, window, shift, c, &g)) return rc;
  DOVE_CHECK_ARG(windows && shortcut && out && windows != out && b > 0, "dove_swin3d_window_scatter_f32: null windows / shortcut / out, out aliasing windows, or b %d", b);
  DOVE_CHECK_ARG((((uintptr_t)windows | (uintptr_t)shortcut | (uintptr_t)out) & 15) == 0,
                 "dove_swin3d_window_scatter_f32: windows, shortcut and out must be 16-byte aligned");
  const long long total = (long long)b * g.D * g.H * g.W * (c / 4);
  DOVE_CHECK_ARG(total < (long long)NT * 0x7fffffffLL, "dove_swin3d_window_scatter_f32: batch too large");
  hipLaunchKernelGGL(swin3d_window_scatter_kernel, dim3(blocks_for(total, NT)), dim3(NT), 0, (hipStream_t)stream, windows, shortcut, g, total, out);
  DOVE_CHECK_LAUNCH("dove_swin3d_window_scatter_f32");
  return DOVE_OK;
}

extern "C" int dove_swin3d_patch_merge_f32(const float* x, long long maps, int h, int w, int c, float* out, void* stream) {
  DOVE_CHECK_ARG(x && out && x != out && maps > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0,
                 "dove_swin3d_patch_merge_f32: null or aliased x / out, or maps %lld, %d x %d, c %d (positive, c a multiple of 4)", maps, h, w, c);
  DOVE_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "dove_swin3d_patch_merge_f32: x and out must be 16-byte aligned");
  const long long total = maps * ((h + 1) / 2) * ((w + 1) / 2) * c;      // 4 chunks of c / 4 float4s per output pixel
  DOVE_CHECK_ARG(total < (long long)NT * 0x7fffffffLL, "dove_swin3d_patch_merge_f32: batch too large");
  hipLaunchKernelGGL(swin3d_patch_merge_kernel, dim3(blocks_for(total, NT)), dim3(NT), 0, (hipStream_t)stream, x, h, w, c, total, out);
  DOVE_CHECK_LAUNCH("dove_swin3d_patch_merge_f32");
  return DOVE_OK;
}

extern "C" void dove_swin3d_attention_tiles(int* q_tile, int* kv_tile, int* max_n) {
  if (q_tile) *q_tile = WA_T;
  if (kv_tile) *kv_tile = WA_T;
  if (max_n) *max_n = WA_MAX_N;
}

extern "C" int dove_swin3d_window_attention_f32(const float* q, const float* k, const float* v, long long ld, long long windows, int n, int heads,
                                                float scale, const float* table_a, const float* table_b, int table_rows, const int* index,
                                                const int* frag, const int* region, int id_windows, float* out, long long ldo, void* stream) {
  DOVE_CHECK_ARG(q && k && v && table_a && index && out, "dove_swin3d_window_attention_f32: null q / k / v / table_a / index / out");
  DOVE_CHECK_ARG(windows > 0 && windows <= 0x7fffffffLL && n >= 1 && n <= WA_MAX_N && heads > 0 && heads <= 65535 && table_rows > 0,
                 "dove_swin3d_window_attention_f32: windows %lld, n %d (1 .. %d), heads %d (1 .. 65535), table_rows %d", windows, n, WA_MAX_N, heads,
                 table_rows);
  DOVE_CHECK_ARG(ld >= (long long)heads * WA_D && ldo >= (long long)heads * WA_D && ld % 4 == 0 && ldo % 4 == 0,
                 "dove_swin3d_window_attention_f32: ld %lld and ldo %lld must hold %d heads of 32 and be multiples of 4", ld, ldo, heads);
  DOVE_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0,
                 "dove_swin3d_window_attention_f32: q, k, v, out must be 16-byte aligned");
  DOVE_CHECK_ARG(!table_b || frag, "dove_swin3d_window_attention_f32: a second table needs the fragment ids");
  DOVE_CHECK_ARG((!frag && !region) || (id_windows > 0 && windows % id_windows == 0),
                 "dove_swin3d_window_attention_f32: id_windows %d must divide windows %lld", id_windows, windows);
  const int npad = (n + WA_T - 1) / WA_T * WA_T, tiles = npad / WA_T, waves = tiles < WA_MAX_WAVES ? tiles : WA_MAX_WAVES;
  const size_t lds = (size_t)npad * (WA_LDK + WA_D) * sizeof(float) + (size_t)npad * 2 * sizeof(int) +
                     (size_t)table_rows * (table_b ? 2 : 1) * sizeof(float);
  DOVE_CHECK_ARG(lds <= WA_MAX_LDS, "dove_swin3d_window_attention_f32: a window of %d tokens and %d tables of %d rows need %zu bytes of LDS (limit %d)",
                 n, table_b ? 2 : 1, table_rows, lds, WA_MAX_LDS);
  static PerDeviceOnce attr_set;
  if (auto once_ = attr_set.guard())
    (void)hipFuncSetAttribute((const void*)swin3d_window_attention_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WA_MAX_LDS);
  WaArgs a{q, k, v, ld, n, heads, scale, table_a, table_b, table_rows, index, frag, region, (frag || region) ? id_windows : 1, out, ldo};
  hipLaunchKernelGGL(swin3d_window_attention_kernel, dim3((unsigned)windows, (unsigned)heads), dim3(64 * waves), lds, (hipStream_t)stream, a);
  DOVE_CHECK_LAUNCH("dove_swin3d_window_attention_f32");
  return DOVE_OK;
}

extern "C" int dove_vqa_head_f64(const float* features, long long ld, int clips, int tokens, int dim, const float* w1, const float* b1, int hidden,
                                 const float* w2, const float* b2, double* out, void* stream) {
  DOVE_CHECK_ARG(features && w1 && b1 && w2 && b2 && out, "dove_vqa_head_f64: null features / w1 / b1 / w2 / b2 / out");
  DOVE_CHECK_ARG(clips > 0 && tokens > 0 && dim > 0 && ld >= dim && hidden >= 1 && hidden <= HEAD_MAX_HID,
                 "dove_vqa_head_f64: clips %d, tokens %d, dim %d, ld %lld, hidden %d (1 .. %d)", clips, tokens, dim, ld, hidden, HEAD_MAX_HID);
  hipLaunchKernelGGL(vqa_head_kernel, dim3((unsigned)clips), dim3(HEAD_NT), 0, (hipStream_t)stream, features, ld, tokens, dim, w1, b1, hidden, w2,
                     b2, out);
  DOVE_CHECK_LAUNCH("dove_vqa_head_f64");
  return DOVE_OK;
}
