// The fp32 convolution of RAFT, LPIPS / DISTS, CLIP-IQA and MUSIQ (include/dove_hip.h has the contract): every
// kernel, the one dispatch and the one launch behind dove_conv2d_f32, dove_corr_volume_f32, dove_convnet_conv_f32 and dove_resnet_conv_f32.
// Activations are channels-last fp32 [n][h][w][c] with a pixel stride that may exceed c, so a conv reads or fills a slice of a wider buffer;
// weights are [kh][kw][cin][cout].  Everything is an implicit GEMM on v_mfma_f32_32x32x2_f32 with M = n * ho * wo output pixels, N = cout and
// K = kh * kw * cin ordered tap-major then channel.  Every output is one k-ordered fmaf chain whatever the walk, the tile it falls in and the
// batch (no split-K); the bias is added after the chain, then the residual, the activation last.  So all walks give the same bits, and the
// dispatch below is free to choose by speed alone.  M and N are ragged everywhere: zeros are loaded and nothing is stored outside.
//
// conv_f32_kernel<WT> (GENERAL): any kernel side, stride, padding and channel count.  One 256-thread block owns a 64 x 64 tile; K advances 32
//   at a time through LDS (A [64][33], B [32][96]: both fragment reads are conflict-free); each of the four waves owns one 32 x 32
//   accumulator.  K is ragged too.  The only walk with scale / shift, sigmoid / tanh and out_mul.  WT = true reads the "weights" transposed,
//   [cout][K] with blockIdx.z as the pair: the all-pairs correlation of dove_corr_volume_f32 (a 1 x 1 conv whose weights are the second
//   feature map).
// tile_body<TN, MODE>: the 128 x TN tile of the walks that read 16 bytes at a time (vector_eligible: cin % 32 == 0, cout % 4 == 0,
//   ldx % 4 == 0, 16-byte aligned x and w), stride 1.  The four waves form a 2 x 2 grid of 64 x TN/2 quarters, 2 x TN/64 accumulators each.
//   K advances 32 at a time = 32 channels of one tap, so an A row is one contiguous 128-byte run of the input; a row's pixel offset and its
//   tap-validity mask are computed once, and the tap and channel counters advance by additions (no division in the loop).  LDS is
//   double-buffered: the global loads of step k + 1 are issued before the MFMAs of step k and land in the other buffer after them, with one
//   barrier per step.  Its instantiations:
//     pointwise_f32_kernel<128 | 64, MODE_1X1> (POINTWISE): k = 1, a plain GEMM; TN = 128 for cout >= 128 and 64 below.
//     pointwise_f32_kernel<128 | 64, MODE_POOL> (POINTWISE, pool 2): the A loader keeps the four input pixels of an output pixel in flight
//       and stages ((a + b) + (c + d)) * 0.25f: the conv of the 2 x 2 average (floor sizes) without the pooled map ever being written.
//     convnet3x3_f32_kernel = <128, MODE_3X3> (FAST): k = 3, pad 1, cout >= 128; a 9-bit tap mask per row.
//     convnet3x3_n64_f32_kernel = <64, MODE_3X3> (N64): the same for cout in {32, 64}, so no MFMA multiplies an empty half tile.
//   Only the pointwise modes have a residual (it may be out: each element is read and written by the same thread); the branch is compiled
//   out of the 3 x 3 modes, which keeps their epilogue free of per-element loads and branches.
//   LDS banks: fragments are read with ds_read_b32, whose bank is (dword address) mod 32 within each 32-lane half.
//     A [128][33]: lane l of a half reads row r0 + l, column 2 s + half: dword 33 (r0 + l) + k, bank (const + l) mod 32: 32 different banks.
//       Without the pad column the stride would be 32 and all 32 lanes would fall on one bank.
//     B [32][TN]: lane l of a half reads row 2 s + half, column c0 + l: consecutive dwords, 32 different banks for TN = 64 as for 128,
//       since a row is a multiple of 32 dwords and the lanes walk along it; no pad is needed.
//     A is filled with ds_write_b32: a half holds 4 rows r..r+3 x 8 chunks q, dword 33 row + 4 q + e -> bank (const + (l >> 3) + 4 (l & 7))
//       mod 32, again all different.  B is filled with 16-byte writes of consecutive dwords.
// Each extern "C" entry copies its public struct into one description (Conv), adds the refusals that are its own, and names the walks it
// allows; pick_walk chooses among them and launch_conv is the only place that fills ConvP / TileP and launches.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int BM = 64, BN = 64, BK = 32, LDA = BK + 1, LDB = BN + 32;      // conv_f32_kernel
constexpr int TM = 128, TK = 32, TLDA = TK + 1;                            // tile_body
constexpr int tile_lds(int tn) { return 2 * (TM * TLDA + TK * tn) * (int)sizeof(float); }   // 66,560 bytes for 128, 50,176 for 64: dynamic

// ------------------------------------------------------- the general 64 x 64 walk -------------------------------------------------------
struct ConvP {
  const float* x; const float* w; const float* bias; const float* scale; const float* shift; float* out;
  int H, W, Cin, Ho, Wo, Cout, kw, stride, ph, pw, act, K;
  long long M, ldx, ldo, ldwk, ldwn, bx, bw, bo;
  float mul;
};

__device__ __forceinline__ float activate(float v, int act) {
  if (act == DOVE_ACT_RELU) return fmaxf(v, 0.f);
  // sigmoid and tanh in fp64: their own rounding stays below the accumulated error of the sum that feeds them
  if (act == DOVE_ACT_SIGMOID) return (float)(1.0 / (1.0 + exp(-(double)v)));
  if (act == DOVE_ACT_TANH) return (float)tanh((double)v);
  return v;
}

template <bool WT>
__global__ __launch_bounds__(NT) void conv_f32_kernel(ConvP p) {
  __shared__ float As[BM * LDA];
  __shared__ float Bs[BK * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const float* x = p.x + blockIdx.z * p.bx;
  const float* w = p.w + blockIdx.z * p.bw;
  float* out = p.out + blockIdx.z * p.bo;

  // A loader: this thread fills column ak of rows ar + 8 j
  const int ak = tid & 31, ar = tid >> 5;
  long long pbase[8];
  int iy0[8], ix0[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long long m = m0 + ar + 8 * j;
    if (m < p.M) {
      const long long img = m / ((long long)p.Ho * p.Wo);
      const int r = (int)(m - img * p.Ho * p.Wo), oy = r / p.Wo, ox = r - oy * p.Wo;
      pbase[j] = img * p.H * p.W;
      iy0[j] = oy * p.stride - p.ph;
      ix0[j] = ox * p.stride - p.pw;
    } else {
      pbase[j] = 0;
      iy0[j] = -(1 << 28);                     // every tap of a row past M falls outside the image
      ix0[j] = 0;
    }
  }
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;

  for (int k0 = 0; k0 < p.K; k0 += BK) {
    float av[8], bv[8];
    {
      const int k = k0 + ak;
      const bool kv = k < p.K;
      const int tap = kv ? k / p.Cin : 0, ci = k - tap * p.Cin, ky = tap / p.kw, kx = tap - ky * p.kw;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int iy = iy0[j] + ky, ix = ix0[j] + kx;
        const bool ok = kv && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        av[j] = ok ? x[(pbase[j] + (long long)iy * p.W + ix) * p.ldx + ci] : 0.f;
      }
    }
    if (!WT) {                                 // weights [K][cout]: lanes along cout
      const int bn = tid & 63, bk = tid >> 6;
      const bool nv = n0 + bn < p.Cout;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = k0 + bk + 4 * j;
        bv[j] = (nv && k < p.K) ? w[(long long)k * p.ldwk + (long long)(n0 + bn) * p.ldwn] : 0.f;
      }
    } else {                                   // "weights" [cout][K] (the second feature map): lanes along K
      const bool kv = k0 + ak < p.K;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = n0 + ar + 8 * j;
        bv[j] = (kv && n < p.Cout) ? w[(long long)(k0 + ak) * p.ldwk + (long long)n * p.ldwn] : 0.f;
      }
    }
    __syncthreads();                           // the previous tile's fragment reads are done
#pragma unroll
    for (int j = 0; j < 8; ++j) As[(ar + 8 * j) * LDA + ak] = av[j];
    if (!WT) {
#pragma unroll
      for (int j = 0; j < 8; ++j) Bs[((tid >> 6) + 4 * j) * LDB + (tid & 63)] = bv[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) Bs[ak * LDB + ar + 8 * j] = bv[j];
    }
    __syncthreads();
    const float* ap = As + (wm + (lane & 31)) * LDA + (lane >> 5);
    const float* bp = Bs + (lane >> 5) * LDB + wn + (lane & 31);
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], bp[2 * s * LDB], acc, 0, 0, 0);
  }

  const int n = n0 + wn + (lane & 31);
  if (n >= p.Cout) return;
  const float b = p.bias ? p.bias[n] : 0.f;
  const float sc = p.scale ? p.scale[n] : 1.f, sh = p.scale ? p.shift[n] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (m >= p.M) continue;
    float v = acc[r] + b;
    if (p.scale) v = fmaf(v, sc, sh);
    v = activate(v, p.act);
    if (p.mul != 1.f) v *= p.mul;
    out[m * p.ldo + n] = v;
  }
}

// ------------------------------------------------- the 128 x TN tile: 1 x 1, pooled 1 x 1, 3 x 3 -------------------------------------------------
struct TileP {
  const float* x; const float* w; const float* bias; const float* res; float* out;
  int H, W, Cin, Cout, relu;                   // H, W: the output map (the pooled map under pool-on-load)
  int Hi, Wi;                                  // MODE_POOL: the input map, H = Hi / 2, W = Wi / 2
  long long M, ldx, ldr, ldo;
};

enum { MODE_1X1 = 0, MODE_POOL = 1, MODE_3X3 = 2 };

template <int TN, int MODE>
__device__ __forceinline__ void tile_body(const TileP& p) {
  constexpr int F_A = TM * TLDA, F_B = TK * TN;
  constexpr int BQ = TN / 4, BROWS = NT / BQ, NBJ = TK / BROWS;   // B loader: chunk bq of K rows br + BROWS j
  constexpr int WN = TN / 2, NJ = WN / 32;                        // a wave's columns and accumulators across
  constexpr int NP = MODE == MODE_POOL ? 4 : 1;                   // input pixels a row keeps in flight
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const As = smem;                      // [2][TM][TLDA]
  float* const Bs = smem + 2 * F_A;            // [2][TK][TN]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * TM;
  const int n0 = blockIdx.y * TN;

  // A loader: this thread reads the 16-byte chunk aq of rows ar + 32 j
  const int aq = tid & 7, ar = tid >> 3;
  const int bq = tid % BQ, br = tid / BQ;
  long long poff[4];
  unsigned vmask[4];                           // MODE_3X3: the valid taps; otherwise bit 0 = the row exists
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long m = m0 + ar + 32 * j;
    poff[j] = 0;
    vmask[j] = 0;
    if (m < p.M) {
      poff[j] = m * p.ldx + aq * 4;
      vmask[j] = 1u;
      if (MODE != MODE_1X1) {
        const long long hw = (long long)p.H * p.W, img = m / hw;
        const int r = (int)(m - img * hw), oy = r / p.W, ox = r - oy * p.W;
        if (MODE == MODE_POOL) poff[j] = ((img * p.Hi + 2 * oy) * p.Wi + 2 * ox) * p.ldx + aq * 4;   // the upper left of the four
        if (MODE == MODE_3X3) vmask[j] = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int iy = oy + t / 3 - 1, ix = ox + t % 3 - 1;
          if (MODE == MODE_3X3 && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) vmask[j] |= 1u << t;
        }
      }
    }
  }
  const bool bvalid = n0 + bq * 4 < p.Cout;    // cout % 4 == 0: a chunk is inside or outside as a whole
  const float* wp = p.w + (long long)br * p.Cout + n0 + bq * 4;

  f32x16 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * WN, l31 = lane & 31, half = lane >> 5;

  // K walk state: tap (ky, kx) and the first channel ci of the step, advanced by additions
  int tap = 0, kx = 0, ci = 0;
  long long toff = MODE == MODE_3X3 ? -((long long)p.W + 1) * p.ldx : 0;   // pixel offset of tap (ky - 1, kx - 1), in floats
  const long long wstep = (long long)TK * p.Cout, prow = (long long)p.Wi * p.ldx;
  f32x4 av[4][NP], bv[NBJ];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  auto load = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (MODE == MODE_3X3) {
        av[j][0] = ((vmask[j] >> tap) & 1u) ? *(const f32x4*)(p.x + poff[j] + toff + ci) : zero4;
      } else {
        const float* s = p.x + poff[j] + ci;
        av[j][0] = vmask[j] ? *(const f32x4*)s : zero4;
        if constexpr (MODE == MODE_POOL) {     // the other three pixels of the 2 x 2 window stay in flight with it
          av[j][1] = vmask[j] ? *(const f32x4*)(s + p.ldx) : zero4;
          av[j][2] = vmask[j] ? *(const f32x4*)(s + prow) : zero4;
          av[j][3] = vmask[j] ? *(const f32x4*)(s + prow + p.ldx) : zero4;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NBJ; ++j) bv[j] = bvalid ? *(const f32x4*)(wp + (long long)(BROWS * j) * p.Cout) : zero4;
    wp += wstep;
    ci += TK;
    if (MODE == MODE_3X3 && ci == p.Cin) {
      ci = 0;
      ++tap;
      toff += p.ldx;
      if (++kx == 3) {
        kx = 0;
        toff += ((long long)p.W - 3) * p.ldx;
      }
    }
  };
  auto stage = [&](int buf) {
    float* a = As + buf * F_A;
    float* b = Bs + buf * F_B;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float* d = a + (ar + 32 * j) * TLDA + aq * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (MODE == MODE_POOL) d[e] = ((av[j][0][e] + av[j][1][e]) + (av[j][2][e] + av[j][3][e])) * 0.25f;
        else d[e] = av[j][0][e];
      }
    }
#pragma unroll
    for (int j = 0; j < NBJ; ++j) *(f32x4*)(b + (br + BROWS * j) * TN + bq * 4) = bv[j];
  };

  const int KT = (MODE == MODE_3X3 ? 9 : 1) * (p.Cin / TK);
  load();
  stage(0);
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < KT) load();                   // in flight under this step's MFMAs
    const float* a0 = As + buf * F_A + (wm + l31) * TLDA + half;
    const float* a1 = a0 + 32 * TLDA;
    const float* b0 = Bs + buf * F_B + half * TN + wn + l31;
#pragma unroll
    for (int s = 0; s < TK / 2; ++s) {
      const float x0 = a0[2 * s], x1 = a1[2 * s];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float y = b0[2 * s * TN + 32 * j];
        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, y, acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, y, acc[1][j], 0, 0, 0);
      }
    }
    if (kt + 1 < KT) stage(buf ^ 1);           // the other buffer: its readers finished before the barrier that ended step kt - 1
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = n0 + wn + 32 * j + l31;
    if (n >= p.Cout) continue;
    const float b = p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= p.M) continue;
        float v = acc[i][j][r] + b;
        if (MODE != MODE_3X3 && p.res) v += p.res[m * p.ldr + n];   // the dispatch refuses a residual outside the pointwise walk
        if (p.relu) v = fmaxf(v, 0.f);
        p.out[m * p.ldo + n] = v;
      }
  }
}

template <int TN, int MODE>
__global__ __launch_bounds__(NT) void pointwise_f32_kernel(TileP p) { tile_body<TN, MODE>(p); }

__global__ __launch_bounds__(NT) void convnet3x3_f32_kernel(TileP p) { tile_body<128, MODE_3X3>(p); }

__global__ __launch_bounds__(NT) void convnet3x3_n64_f32_kernel(TileP p) { tile_body<64, MODE_3X3>(p); }

// ------------------------------------------------------------- one description -------------------------------------------------------------
struct Conv {
  const float* x; const float* w; const float* bias; const float* scale; const float* shift; const float* residual; float* out;
  int n, h, w_in, cin, cout, kh, kw, stride, pad_h, pad_w, pool, act;
  float out_mul;
  long long ldx, ldr, ldo;
  const char* entry;                           // the public function, for error messages
};

// the rules are shared with the _kernel_name functions, which refuse silently
#define REFUSE(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      if (report) dove_set_error(__VA_ARGS__);   \
      return false;                              \
    }                                            \
  } while (0)

template <typename A>
bool struct_size_ok(const A* a, const char* entry, bool report) {
  REFUSE(a && a->struct_size == sizeof(A), "%s: struct_size %u is not the library's %zu", entry, a ? a->struct_size : 0u, sizeof(A));
  return true;
}

// what every entry asks of its arguments
bool conv_ok(const Conv& c, bool report) {
  REFUSE(c.x && c.w && c.out, "%s: null x / w / out", c.entry);
  REFUSE(c.n > 0 && c.h > 0 && c.w_in > 0 && c.cin > 0 && c.cout > 0, "%s: n, h, w, cin, cout must be positive", c.entry);
  REFUSE(c.ldx >= c.cin && c.ldo >= c.cout, "%s: ldx %lld < cin %d or ldo %lld < cout %d", c.entry, c.ldx, c.cin, c.ldo, c.cout);
  REFUSE(!c.residual || c.ldr >= c.cout, "%s: ldr %lld < cout %d", c.entry, c.ldr, c.cout);
  return true;
}

// the size limits of dove_convnet_conv_f32 and dove_resnet_conv_f32 (the tile walks index the input with m * ldx)
bool tile_sizes_ok(const Conv& c, bool report) {
  const long long pixels = (long long)c.n * c.h * c.w_in;
  REFUSE(pixels <= 0x7fffffffLL * 32 && pixels * c.ldx < (1LL << 46) && (long long)c.kh * c.kw * c.cin < (1 << 24), "%s: problem too large",
         c.entry);
  return true;
}

inline int out_side(int in, int pool, int pad, int k, int stride) { return (in / pool + 2 * pad - k) / stride + 1; }

// --------------------------------------------------------------- one dispatch ---------------------------------------------------------------
enum Walk : unsigned { WALK_POINTWISE = 1, WALK_N64 = 2, WALK_FAST = 4, WALK_GENERAL = 8 };   // bits: an entry passes the set it allows

const char* walk_name(Walk walk) {
  return walk == WALK_POINTWISE ? "pointwise_f32_kernel" : walk == WALK_N64 ? "convnet3x3_n64_f32_kernel" :
         walk == WALK_FAST ? "convnet3x3_f32_kernel" : "conv_f32_kernel";
}

// the tile walks read x and w 16 bytes at a time, 32 channels per K step
bool vector_eligible(const Conv& c) {
  return c.cin % TK == 0 && c.cout % 4 == 0 && c.ldx % 4 == 0 && ((uintptr_t)c.x & 15) == 0 && ((uintptr_t)c.w & 15) == 0;
}

Walk pick_walk(const Conv& c, unsigned allowed) {
  // the tile walks have a bias, a residual and a ReLU, nothing else
  const bool plain = !c.scale && c.out_mul == 1.f && (c.act == DOVE_ACT_NONE || c.act == DOVE_ACT_RELU);
  if (plain && vector_eligible(c) && c.kh == c.kw && c.stride == 1 && c.pad_h == c.kh / 2 && c.pad_w == c.kw / 2) {
    if (c.kh == 1 && (allowed & WALK_POINTWISE)) return WALK_POINTWISE;
    if (c.kh == 3 && (c.cout == 32 || c.cout == 64) && (allowed & WALK_N64)) return WALK_N64;
    // cout >= 128: below that the 128-wide N tile is partly empty and conv_f32_kernel's 64 x 64 tile is faster (measured on VGG16's
    // 64 -> 64 at 2 x 720 x 1280: 2.51 ms against 1.99 ms; docs/kernels.md)
    if (c.kh == 3 && c.cout >= 128 && (allowed & WALK_FAST)) return WALK_FAST;
  }
  return WALK_GENERAL;
}

// ---------------------------------------------------------------- one launch ----------------------------------------------------------------
int launch_conv(const Conv& c, Walk walk, void* stream) {
  const int Ho = out_side(c.h, c.pool, c.pad_h, c.kh, c.stride), Wo = out_side(c.w_in, c.pool, c.pad_w, c.kw, c.stride);
  const long long M = (long long)c.n * Ho * Wo;
  if (walk == WALK_GENERAL) {                  // never with pool 2 or a residual: the entry that has them refuses both here
    ConvP p;
    p.x = c.x; p.w = c.w; p.bias = c.bias; p.scale = c.scale; p.shift = c.shift; p.out = c.out;
    p.H = c.h; p.W = c.w_in; p.Cin = c.cin; p.Cout = c.cout; p.kw = c.kw; p.stride = c.stride; p.act = c.act;
    p.ph = c.pad_h; p.pw = c.pad_w; p.Ho = Ho; p.Wo = Wo; p.M = M; p.K = c.kh * c.kw * c.cin;
    p.ldx = c.ldx; p.ldo = c.ldo; p.ldwk = c.cout; p.ldwn = 1; p.bx = p.bw = p.bo = 0;
    p.mul = c.out_mul;
    dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((c.cout + BN - 1) / BN), 1);
    hipLaunchKernelGGL(conv_f32_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, p);
  } else {
    TileP p;
    p.x = c.x; p.w = c.w; p.bias = c.bias; p.res = c.residual; p.out = c.out;
    p.H = Ho; p.W = Wo; p.Cin = c.cin; p.Cout = c.cout; p.relu = c.act == DOVE_ACT_RELU;
    p.Hi = c.h; p.Wi = c.w_in;
    p.M = M; p.ldx = c.ldx; p.ldr = c.ldr; p.ldo = c.ldo;
    auto tile = [&](auto kernel, PerDeviceOnce& once, int tn) {
      if (auto once_ = once.guard()) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, tile_lds(tn));
      dim3 grid((unsigned)((M + TM - 1) / TM), (unsigned)((c.cout + tn - 1) / tn), 1);
      hipLaunchKernelGGL(kernel, grid, dim3(NT), tile_lds(tn), (hipStream_t)stream, p);
    };
    static PerDeviceOnce once[6];
    if (walk == WALK_FAST) tile(convnet3x3_f32_kernel, once[0], 128);
    else if (walk == WALK_N64) tile(convnet3x3_n64_f32_kernel, once[1], 64);
    else if (c.pool == 2 && c.cout >= 128) tile(pointwise_f32_kernel<128, MODE_POOL>, once[2], 128);
    else if (c.pool == 2) tile(pointwise_f32_kernel<64, MODE_POOL>, once[3], 64);
    else if (c.cout >= 128) tile(pointwise_f32_kernel<128, MODE_1X1>, once[4], 128);
    else tile(pointwise_f32_kernel<64, MODE_1X1>, once[5], 64);
  }
  DOVE_CHECK_LAUNCH(c.entry);
  return DOVE_OK;
}

// ------------------------------------------------------- the entries' own rules -------------------------------------------------------
bool conv2d_walk(const dove_conv2d_f32_args* a, bool report, Conv& c, Walk& walk) {
  if (!struct_size_ok(a, "dove_conv2d_f32", report)) return false;
  c = Conv{a->x, a->w, a->bias, a->scale, a->shift, nullptr, a->out, a->n, a->h, a->w_in, a->cin, a->cout, a->kh, a->kw, a->stride,
           a->kh / 2, a->kw / 2, 1, a->act, a->out_mul, a->ldx, 0, a->ldo, "dove_conv2d_f32"};
  if (!conv_ok(c, report)) return false;
  REFUSE((c.kh == 1 || c.kh == 3 || c.kh == 5 || c.kh == 7) && (c.kw == 1 || c.kw == 3 || c.kw == 5 || c.kw == 7),
         "%s: kernel %d x %d (sides are 1, 3, 5 or 7)", c.entry, c.kh, c.kw);
  REFUSE(c.stride == 1 || c.stride == 2, "%s: stride %d (1 or 2)", c.entry, c.stride);
  REFUSE(c.act >= DOVE_ACT_NONE && c.act <= DOVE_ACT_TANH, "%s: act %d", c.entry, c.act);
  REFUSE((c.scale == nullptr) == (c.shift == nullptr), "%s: scale and shift come together", c.entry);
  const long long M = (long long)c.n * out_side(c.h, 1, c.pad_h, c.kh, c.stride) * out_side(c.w_in, 1, c.pad_w, c.kw, c.stride);
  REFUSE(M <= 0x7fffffffLL * BM / 2 && (long long)c.n * c.h * c.w_in < (1LL << 40) && (long long)c.kh * c.kw * c.cin < (1 << 24),
         "%s: problem too large", c.entry);
  walk = pick_walk(c, WALK_GENERAL);
  return true;
}

bool convnet_walk(const dove_convnet_conv_f32_args* a, bool report, Conv& c, Walk& walk) {
  if (!struct_size_ok(a, "dove_convnet_conv_f32", report)) return false;
  c = Conv{a->x, a->w, a->bias, nullptr, nullptr, nullptr, a->out, a->n, a->h, a->w_in, a->cin, a->cout, a->kh, a->kw, a->stride,
           a->pad_h, a->pad_w, 1, a->relu ? DOVE_ACT_RELU : DOVE_ACT_NONE, 1.f, a->ldx, 0, a->ldo, "dove_convnet_conv_f32"};
  if (!conv_ok(c, report)) return false;
  REFUSE(c.kh >= 1 && c.kh <= 11 && c.kw >= 1 && c.kw <= 11, "%s: kernel %d x %d (sides are 1 to 11)", c.entry, c.kh, c.kw);
  REFUSE(c.stride >= 1 && c.stride <= 4, "%s: stride %d (1 to 4)", c.entry, c.stride);
  REFUSE(c.pad_h >= 0 && c.pad_h < c.kh && c.pad_w >= 0 && c.pad_w < c.kw, "%s: pad %d x %d must be below the kernel %d x %d", c.entry,
         c.pad_h, c.pad_w, c.kh, c.kw);
  REFUSE(c.h + 2 * c.pad_h >= c.kh && c.w_in + 2 * c.pad_w >= c.kw, "%s: image %d x %d is smaller than the kernel %d x %d", c.entry, c.h,
         c.w_in, c.kh, c.kw);
  if (!tile_sizes_ok(c, report)) return false;
  walk = pick_walk(c, WALK_FAST | WALK_GENERAL);   // a 3 x 3 with cout 32 or 64 stays on conv_f32_kernel here
  return true;
}

bool resnet_walk(const dove_resnet_conv_f32_args* a, bool report, Conv& c, Walk& walk) {
  if (!struct_size_ok(a, "dove_resnet_conv_f32", report)) return false;
  c = Conv{a->x, a->w, a->bias, nullptr, nullptr, a->residual, a->out, a->n, a->h, a->w_in, a->cin, a->cout, a->k, a->k, a->stride,
           a->k / 2, a->k / 2, a->pool, a->relu ? DOVE_ACT_RELU : DOVE_ACT_NONE, 1.f, a->ldx, a->ldr, a->ldo, "dove_resnet_conv_f32"};
  if (!conv_ok(c, report)) return false;
  REFUSE(c.kh == 1 || c.kh == 3, "%s: kernel side %d (1 or 3)", c.entry, c.kh);
  REFUSE(c.stride == 1 || c.stride == 2, "%s: stride %d (1 or 2)", c.entry, c.stride);
  REFUSE(c.pool == 1 || c.pool == 2, "%s: pool %d (1 or 2)", c.entry, c.pool);
  REFUSE(c.pool == 1 || (c.kh == 1 && c.stride == 1), "%s: pool 2 belongs to a 1 x 1 conv of stride 1 (k %d, stride %d)", c.entry, c.kh,
         c.stride);
  REFUSE(c.pool == 1 || (c.h >= 2 && c.w_in >= 2), "%s: image %d x %d is smaller than the 2 x 2 pool", c.entry, c.h, c.w_in);
  if (!tile_sizes_ok(c, report)) return false;
  walk = pick_walk(c, WALK_POINTWISE | WALK_N64 | WALK_FAST | WALK_GENERAL);
  REFUSE(walk == WALK_POINTWISE || (c.pool == 1 && !c.residual),
         "%s: pool 2 and a residual need pointwise_f32_kernel (k 1, stride 1, cin %% 32 == 0, cout %% 4 == 0, ldx %% 4 == 0, "
         "16-byte aligned x and w); got k %d, stride %d, cin %d, cout %d, ldx %lld", c.entry, c.kh, c.stride, c.cin, c.cout, c.ldx);
  return true;
}
#undef REFUSE

}  // namespace

// ------------------------------------------------------------- C entries -------------------------------------------------------------
extern "C" int dove_conv2d_f32(const dove_conv2d_f32_args* a, void* stream) {
  Conv c;
  Walk walk;
  return conv2d_walk(a, true, c, walk) ? launch_conv(c, walk, stream) : DOVE_EINVAL;
}

extern "C" const char* dove_convnet_conv_f32_kernel_name(const dove_convnet_conv_f32_args* a) {
  Conv c;
  Walk walk;
  return convnet_walk(a, false, c, walk) ? walk_name(walk) : "";
}

extern "C" int dove_convnet_conv_f32(const dove_convnet_conv_f32_args* a, void* stream) {
  Conv c;
  Walk walk;
  return convnet_walk(a, true, c, walk) ? launch_conv(c, walk, stream) : DOVE_EINVAL;
}

extern "C" const char* dove_resnet_conv_f32_kernel_name(const dove_resnet_conv_f32_args* a) {
  Conv c;
  Walk walk;
  return resnet_walk(a, false, c, walk) ? walk_name(walk) : "";
}

extern "C" int dove_resnet_conv_f32(const dove_resnet_conv_f32_args* a, void* stream) {
  Conv c;
  Walk walk;
  return resnet_walk(a, true, c, walk) ? launch_conv(c, walk, stream) : DOVE_EINVAL;
}

// The all-pairs correlation keeps its own ConvP: a 1 x 1 conv over h w "pixels" whose weights are the second feature map, read transposed,
// one (fmap1, fmap2) pair per blockIdx.z.
extern "C" int dove_corr_volume_f32(const float* fmap1, const float* fmap2, int n, int h, int w, int c, float scale, float* out,
                                    void* stream) {
  DOVE_CHECK_ARG(fmap1 && fmap2 && out, "dove_corr_volume_f32: null fmap1 / fmap2 / out");
  DOVE_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && c > 0 && (long long)h * w < (1 << 24),
                 "dove_corr_volume_f32: n (<= 65535), h, w, c must be positive and h * w below 2^24");
  const long long hw = (long long)h * w;
  ConvP p;
  p.x = fmap1; p.w = fmap2; p.bias = p.scale = p.shift = nullptr; p.out = out;
  p.H = 1; p.W = (int)hw; p.Cin = c; p.Cout = (int)hw; p.kw = 1; p.stride = 1; p.act = DOVE_ACT_NONE; p.ph = p.pw = 0;
  p.Ho = 1; p.Wo = (int)hw; p.M = hw; p.K = c;
  p.ldx = c; p.ldo = hw; p.ldwk = 1; p.ldwn = c; p.bx = p.bw = hw * c; p.bo = hw * hw;
  p.mul = scale;
  dim3 grid((unsigned)((hw + BM - 1) / BM), (unsigned)((hw + BN - 1) / BN), n);
  hipLaunchKernelGGL(conv_f32_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, p);
  DOVE_CHECK_LAUNCH("dove_corr_volume_f32");
  return DOVE_OK;
}
