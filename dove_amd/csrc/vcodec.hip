// The video-compression step of the degradation pipeline (tests/vcodec_ref.py is the definition, byte for byte): what a
// hybrid motion-compensated transform codec does to the pixels, without a bitstream.  Closed groups of `gop` frames (I, then P frames
// predicted from the previous reconstructed frame), full-search integer motion per 16 x 16 macroblock, the H.264 4x4 core transform and
// quantiser on Y'CbCr 4:2:0, an integer bit-count model, and a per-group QP search against bitrate * frames.
//
// motion_search_kernel: one workgroup per macroblock.  The (16 + 2 search)^2 window of the edge-replicated reference and the current block
//   sit in LDS as packed bytes; a lane owns one displacement, reads five aligned dwords per window row, realigns them to its column with
//   v_alignbyte_b32 and feeds v_sad_u8 four pixels at a time (16 rows x 4 dwords = 64 SADs per candidate).  The window rows are
//   2 search / 4 + 5 dwords apart: with search 7 that is 8, so the 32 lanes of a half-wave (three rows of displacements, four dword columns)
//   touch 12 distinct banks per read and the rest broadcast.  The winner is the minimum of the 64-bit key
//   (cost, |dy| + |dx|, dy + 128, dx + 128): the tie-break order of the definition is the integer order of the key.
// code_kernel: one thread per 4x4 block, 24 of them per macroblock (16 luma, 4 Cb, 4 Cr: its six 8x8 regions), 8 macroblocks per workgroup.
//   Prediction (128, or the luma copy / the chroma four-neighbour mean at the macroblock's vector), forward transform, quantisation, bit
//   count over the zigzag scan, dequantisation, inverse and reconstruction all stay in registers; the reconstruction leaves as four dword
//   stores and the bits as one 64-bit atomic per wave into the frame's counter.
// Rate control stays on the device: a group's (lo, hi, QP) live in the workspace, every pass codes all groups of the call at their own QP
//   frame by frame (frame t of every group in one launch), and rc_update_kernel moves the brackets.  52 QPs close in 6 halvings, so a call is
//   always 6 search passes and the final pass at lo: no readback, no allocation, the same launches for every input.
// Intake and output go through dove_rgb_to_yuv_u8 / dove_yuv_to_rgb_u8 on frames padded to whole macroblocks.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int MB = 16;
constexpr int SEARCH = 7;                   // the round trip's search range and motion-cost weight (vcodec_ref.SEARCH, LAMBDA)
constexpr int LAMBDA = 4;
constexpr int PRED_I = 128;                 // the prediction of an I frame
constexpr int QP_MIN = 0, QP_MAX = 51;
constexpr int QP_PASSES = 6;                // ceil(log2(QP_MAX - QP_MIN + 1)): halvings until lo == hi
constexpr int MAX_SEARCH = 15;              // dove_motion_search_u8 on its own takes 0..15
constexpr int MAX_LAMBDA = 1024;
constexpr int WIN_DWORDS = (MB + 2 * MAX_SEARCH) * (2 * MAX_SEARCH / 4 + 5);
constexpr int MB_PER_WG = 8, BLK_PER_MB = 24, CT = MB_PER_WG * BLK_PER_MB;   // code_kernel: 192 threads, three full waves
// BT.601 limited range as rint(c * 65536) (yuv_ref.int_matrices("bt601", "limited")), 4:2:0 with centre siting both ways
constexpr int YUV_FWD[9] = {16829, 33039, 6416, -9714, -19071, 28784, 28784, -24103, -4681};
constexpr int YUV_INV[9] = {76309, 0, 104597, 76309, -25675, -53279, 76309, 132201, 0};
constexpr int YUV_OFF[3] = {16, 128, 128};
constexpr int SITING = DOVE_YUV_SITING_CENTRE;

// H.264 quantiser / dequantiser rows for QP % 6, columns = coefficient class a (even, even), b (odd, odd), c (the rest)
__constant__ int MF[6][3] = {{13107, 5243, 8066}, {11916, 4660, 7490}, {10082, 4194, 6554}, {9362, 3647, 5825}, {8192, 3355, 5243}, {7282, 2893, 4559}};
__constant__ int VQ[6][3] = {{10, 16, 13}, {11, 18, 14}, {13, 20, 16}, {14, 23, 18}, {16, 25, 20}, {18, 29, 23}};

// raster index (4 row + column) of the k-th coefficient of the 4x4 zigzag scan
constexpr int ZIGZAG[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};

struct GroupState {
  int lo, hi, qp, pad;
};

__device__ __forceinline__ int ue_len(int v) { return 2 * (31 - __clz(v + 1)) + 1; }
__device__ __forceinline__ int se_len(int v) { return ue_len(v > 0 ? 2 * v - 1 : -2 * v); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// four bytes of a plane row at x .. x + 3, every coordinate clamped to the plane, as one little-endian dword
__device__ __forceinline__ uint32_t load4_clamped(const uint8_t* __restrict__ p, int y, int x, int H, int W) {
  const uint8_t* row = p + (long long)clampi(y, 0, H - 1) * W;
  return (uint32_t)row[clampi(x, 0, W - 1)] | ((uint32_t)row[clampi(x + 1, 0, W - 1)] << 8) | ((uint32_t)row[clampi(x + 2, 0, W - 1)] << 16) |
         ((uint32_t)row[clampi(x + 3, 0, W - 1)] << 24);
}

// Frame of a block: blockIdx.y * fstep + f0 (the round trip runs frame t of every group: fstep = gop, f0 = t); its reference is frame + ref_df
// of `ref`.  H x W is the plane both are clamped to; cur_fs / ref_fs are the distances between frames in bytes.
__global__ __launch_bounds__(NT) void motion_search_kernel(const uint8_t* __restrict__ cur, long long cur_fs, const uint8_t* __restrict__ ref,
                                                           long long ref_fs, int fstep, int f0, int ref_df, int n, int H, int W, int mbx, int mbs,
                                                           int search, int lam, int* __restrict__ mv_out, int* __restrict__ sad_out) {
  __shared__ uint32_t win[WIN_DWORDS], blk[MB * 4];
  __shared__ unsigned long long wave_min[NT / 64];
  const int tid = threadIdx.x, mb = blockIdx.x;
  const long long frame = (long long)blockIdx.y * fstep + f0;
  if (frame >= n) return;                                            // the whole workgroup: a short last group
  const int x0 = (mb % mbx) * MB, y0 = (mb / mbx) * MB;
  const int D = 2 * search + 1, rows = MB + 2 * search, rs = 2 * search / 4 + 5;
  const uint8_t* cf = cur + frame * cur_fs;
  const uint8_t* rf = ref + (frame + ref_df) * ref_fs;
  for (int i = tid; i < rows * rs; i += NT) win[i] = load4_clamped(rf, y0 - search + i / rs, x0 - search + (i % rs) * 4, H, W);
  if (tid < MB * 4) blk[tid] = load4_clamped(cf, y0 + (tid >> 2), x0 + (tid & 3) * 4, H, W);
  __syncthreads();
  unsigned long long best = ~0ull;
  for (int c = tid; c < D * D; c += NT) {
    const int dyi = c / D, dxi = c % D, q = dxi >> 2, sh = dxi & 3;
    uint32_t sad = 0;
#pragma unroll 4
    for (int r = 0; r < MB; ++r) {
      const uint32_t* row = win + (r + dyi) * rs + q;
      const uint32_t w0 = row[0], w1 = row[1], w2 = row[2], w3 = row[3], w4 = row[4];
      sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, sh), blk[r * 4], sad);
      sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w2, w1, sh), blk[r * 4 + 1], sad);
      sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w3, w2, sh), blk[r * 4 + 2], sad);
      sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w4, w3, sh), blk[r * 4 + 3], sad);
    }
    const int dy = dyi - search, dx = dxi - search;
    const uint32_t cost = sad + (uint32_t)(lam * (se_len(dx) + se_len(dy)));
    const unsigned long long key = ((unsigned long long)cost << 32) | ((unsigned long long)(abs(dy) + abs(dx)) << 16) |
                                   ((unsigned long long)(dy + 128) << 8) | (unsigned long long)(dx + 128);
    best = key < best ? key : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o);
    best = other < best ? other : best;
  }
  if ((tid & 63) == 0) wave_min[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) best = wave_min[i] < best ? wave_min[i] : best;
    const int dy = (int)((best >> 8) & 0xff) - 128, dx = (int)(best & 0xff) - 128;
    const long long o = frame * mbs + mb;
    *(int2*)(mv_out + 2 * o) = make_int2(dy, dx);
    if (sad_out) sad_out[o] = (int)(best >> 32) - lam * (se_len(dx) + se_len(dy));
  }
}

__device__ __forceinline__ uint32_t pack4(const int* b) {           // four values of 0..255 -> one dword by byte selection (see yuv.hip)
  return __builtin_amdgcn_perm((uint32_t)b[1], (uint32_t)b[0], 0x0c0c0400u) | __builtin_amdgcn_perm((uint32_t)b[3], (uint32_t)b[2], 0x04000c0cu);
}

// Frame t of every group: cur and rec hold n 4:2:0 payloads of PH x PW (multiples of 16), fbytes apart.  mv: [n][mbs] (dy, dx), read when t > 0.
__global__ __launch_bounds__(CT) void code_kernel(const uint8_t* __restrict__ cur, uint8_t* __restrict__ rec, long long fbytes, int gop, int t,
                                                  int n, int PH, int PW, int mbx, int mbs, const int* __restrict__ mv,
                                                  const GroupState* __restrict__ state, unsigned long long* __restrict__ fbits) {
  const int tid = threadIdx.x, b = tid % BLK_PER_MB;
  const long long frame = (long long)blockIdx.y * gop + t;
  if (frame >= n) return;                                            // the whole workgroup
  const long long mbl = (long long)blockIdx.x * MB_PER_WG + tid / BLK_PER_MB;
  const bool active = mbl < mbs, intra = t == 0;
  const int mb = active ? (int)mbl : 0;
  const int qp = state[blockIdx.y].qp;
  // the block's plane: luma blocks 0..15 in raster order, then the four of Cb, then the four of Cr
  const bool luma = b < 16;
  const int j = (b - 16) & 3;
  const int pw = luma ? PW : PW / 2, ph = luma ? PH : PH / 2;
  const long long plane = luma ? 0 : (long long)PH * PW + (b >= 20 ? (long long)(PH / 2) * (PW / 2) : 0);
  const int x0 = luma ? (mb % mbx) * 16 + (b & 3) * 4 : (mb % mbx) * 8 + (j & 1) * 4;
  const int y0 = luma ? (mb / mbx) * 16 + (b >> 2) * 4 : (mb / mbx) * 8 + (j >> 1) * 4;
  const uint8_t* cp = cur + frame * fbytes + plane;
  uint8_t* op = rec + frame * fbytes + plane;

  int pred[16], x[16];
  int dy = 0, dx = 0;
  if (intra) {
#pragma unroll
    for (int i = 0; i < 16; ++i) pred[i] = PRED_I;
  } else {
    const int2 v = *(const int2*)(mv + 2 * (frame * mbs + mb));
    dy = v.x;
    dx = v.y;
    const uint8_t* rp = rec + (frame - 1) * fbytes + plane;
    if (luma) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint8_t* row = rp + (long long)clampi(y0 + r + dy, 0, ph - 1) * pw;
#pragma unroll
        for (int c = 0; c < 4; ++c) pred[r * 4 + c] = row[clampi(x0 + c + dx, 0, pw - 1)];
      }
    } else {                                                         // half the vector: floor and ceil neighbours per axis
      const int fy = dy >> 1, fx = dx >> 1, oy = dy & 1, ox = dx & 1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint8_t* ra = rp + (long long)clampi(y0 + r + fy, 0, ph - 1) * pw;
        const uint8_t* rb = rp + (long long)clampi(y0 + r + fy + oy, 0, ph - 1) * pw;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int xa = clampi(x0 + c + fx, 0, pw - 1), xb = clampi(x0 + c + fx + ox, 0, pw - 1);
          pred[r * 4 + c] = (ra[xa] + ra[xb] + rb[xa] + rb[xb] + 2) >> 2;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t wd = *(const uint32_t*)(cp + (long long)(y0 + r) * pw + x0);
#pragma unroll
    for (int c = 0; c < 4; ++c) x[r * 4 + c] = (int)((wd >> (8 * c)) & 0xff) - pred[r * 4 + c];
  }
  // W = CF X CF^T, CF = [[1,1,1,1],[2,1,-1,-2],[1,-1,-1,1],[1,-2,2,-1]]: rows, then columns (exact in integers, any order)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int a = x[r * 4], bb = x[r * 4 + 1], c = x[r * 4 + 2], d = x[r * 4 + 3];
    x[r * 4] = a + bb + c + d;
    x[r * 4 + 1] = 2 * a + bb - c - 2 * d;
    x[r * 4 + 2] = a - bb - c + d;
    x[r * 4 + 3] = a - 2 * bb + 2 * c - d;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int a = x[c], bb = x[4 + c], cc = x[8 + c], d = x[12 + c];
    x[c] = a + bb + cc + d;
    x[4 + c] = 2 * a + bb - cc - 2 * d;
    x[8 + c] = a - bb - cc + d;
    x[12 + c] = a - 2 * bb + 2 * cc - d;
  }
  const int q6 = qp % 6, qs = qp / 6, qbits = 15 + qs, f = (1 << qbits) / (intra ? 3 : 6);
  const int mf[3] = {MF[q6][0], MF[q6][1], MF[q6][2]}, vq[3] = {VQ[q6][0], VQ[q6][1], VQ[q6][2]};
  int z[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = i >> 2, c = i & 3, cls = (r & 1) == 0 && (c & 1) == 0 ? 0 : (r & 1) == 1 && (c & 1) == 1 ? 1 : 2;
    const int w = x[i], lev = (abs(w) * mf[cls] + f) >> qbits;
    z[i] = w < 0 ? -lev : lev;
    x[i] = (z[i] * vq[cls]) << qs;
  }
  // bits: 1 for an empty block, else 1 + ue(nnz - 1) + sum over the zigzag scan of ue(run) + se(level)
  int nnz = 0, run = 0, bits = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int lev = z[ZIGZAG[k]];
    if (lev != 0) {
      bits += ue_len(run) + se_len(lev);
      run = 0;
      ++nnz;
    } else {
      ++run;
    }
  }
  bits = nnz == 0 ? 1 : 1 + ue_len(nnz - 1) + bits;
  if (!intra && b == 0) bits += se_len(dx) + se_len(dy);
  if (!active) bits = 0;
  // inverse: the butterflies on each row, then on each column, then (t + 32) >> 6
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int w0 = x[r * 4], w1 = x[r * 4 + 1], w2 = x[r * 4 + 2], w3 = x[r * 4 + 3];
    const int e0 = w0 + w2, e1 = w0 - w2, e2 = (w1 >> 1) - w3, e3 = w1 + (w3 >> 1);
    x[r * 4] = e0 + e3;
    x[r * 4 + 1] = e1 + e2;
    x[r * 4 + 2] = e1 - e2;
    x[r * 4 + 3] = e0 - e3;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int w0 = x[c], w1 = x[4 + c], w2 = x[8 + c], w3 = x[12 + c];
    const int e0 = w0 + w2, e1 = w0 - w2, e2 = (w1 >> 1) - w3, e3 = w1 + (w3 >> 1);
    x[c] = e0 + e3;
    x[4 + c] = e1 + e2;
    x[8 + c] = e1 - e2;
    x[12 + c] = e0 - e3;
  }
  if (active) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = clampi(pred[r * 4 + c] + ((x[r * 4 + c] + 32) >> 6), 0, 255);
      *(uint32_t*)(op + (long long)(y0 + r) * pw + x0) = pack4(o);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o);
  if ((tid & 63) == 0 && bits != 0) atomicAdd(fbits + frame, (unsigned long long)bits);
}

__global__ void rc_init_kernel(GroupState* __restrict__ state, int groups, unsigned long long* __restrict__ fbits, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < groups) state[i] = GroupState{QP_MIN, QP_MAX, (QP_MIN + QP_MAX) / 2, 0};
  if (i < n) fbits[i] = 0;
}

// One step of the QP search per group: bits of the group's frames against bitrate * frames; the counters are cleared for the next pass.
__global__ void rc_update_kernel(GroupState* __restrict__ state, int groups, int gop, int n, long long bitrate, unsigned long long* __restrict__ fbits,
                                 int final_pass, int* __restrict__ qp_out, long long* __restrict__ bits_out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= groups) return;
  const int f0 = g * gop, f1 = min(f0 + gop, n);
  long long bits = 0;
  for (int f = f0; f < f1; ++f) {
    bits += (long long)fbits[f];
    fbits[f] = 0;
  }
  GroupState s = state[g];
  if (final_pass) {
    if (qp_out) qp_out[g] = s.qp;
    if (bits_out) bits_out[g] = bits;
    return;
  }
  if (s.lo < s.hi) {
    if (bits <= bitrate * (f1 - f0)) s.hi = s.qp;
    else s.lo = s.qp + 1;
  }
  s.qp = s.lo < s.hi ? (s.lo + s.hi) / 2 : s.lo;
  state[g] = s;
}

// u = trunc(clip(x, 0, 255)) on frames edge-replicated to PH x PW
__global__ __launch_bounds__(NT) void intake_kernel(const float* __restrict__ x, int H, int W, int PH, int PW, long long total, uint8_t* __restrict__ out) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  const int px = (int)(t % PW), py = (int)((t / PW) % PH);
  const long long fr = t / ((long long)PW * PH);
  const float* p = x + ((fr * H + min(py, H - 1)) * W + min(px, W - 1)) * 3;
  uint8_t* o = out + t * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(int)fminf(fmaxf(p[c], 0.f), 255.f);
}

__global__ __launch_bounds__(NT) void crop_kernel(const uint8_t* __restrict__ in, int H, int W, int PH, int PW, long long total, uint8_t* __restrict__ out) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= total) return;
  const int px = (int)(t % W), py = (int)((t / W) % H);
  const long long fr = t / ((long long)W * H);
  const uint8_t* p = in + ((fr * PH + py) * PW + px) * 3;
  uint8_t* o = out + t * 3;
  o[0] = p[0];
  o[1] = p[1];
  o[2] = p[2];
}

bool good_shape(int n, int h, int w) { return n > 0 && h > 0 && w > 0 && (long long)h * w <= (1LL << 28); }

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

struct Layout {
  int ph, pw, mbx, mbs, groups;
  long long fbytes;
  size_t rgb, cur, rec, mv, fbits, state, total;                     // offsets into the workspace
};

Layout layout(int n, int h, int w, int gop) {
  Layout L;
  L.ph = (h + MB - 1) / MB * MB;
  L.pw = (w + MB - 1) / MB * MB;
  L.mbx = L.pw / MB;
  L.mbs = L.mbx * (L.ph / MB);
  L.groups = (n + gop - 1) / gop;
  L.fbytes = (long long)L.ph * L.pw * 3 / 2;
  size_t o = 0;
  L.rgb = o;
  o += align256((size_t)n * L.ph * L.pw * 3);
  L.cur = o;
  o += align256((size_t)n * L.fbytes);
  L.rec = o;
  o += align256((size_t)n * L.fbytes);
  L.mv = o;
  o += align256((size_t)n * L.mbs * 2 * sizeof(int));
  L.fbits = o;
  o += align256((size_t)n * sizeof(unsigned long long));
  L.state = o;
  o += align256((size_t)L.groups * sizeof(GroupState));
  L.total = o;
  return L;
}

dove_yuv_format yuv_format(const int* coef) {
  dove_yuv_format f;
  for (int i = 0; i < 9; ++i) f.coef[i] = coef[i];
  for (int i = 0; i < 3; ++i) f.offset[i] = YUV_OFF[i];
  f.chroma = DOVE_YUV_420;
  f.siting_h = SITING;
  return f;
}

}  // namespace

extern "C" int dove_motion_search_u8(const unsigned char* cur, const unsigned char* ref, int n, int h, int w, int search, int lambda, int* mv_out,
                                     int* sad_out, void* stream) {
  DOVE_CHECK_ARG(good_shape(n, h, w) && n <= 65535, "motion_search: bad shape n=%d h=%d w=%d (n <= 65535)", n, h, w);
  DOVE_CHECK_ARG(search >= 0 && search <= MAX_SEARCH, "motion_search: search %d is not in 0..%d", search, MAX_SEARCH);
  DOVE_CHECK_ARG(lambda >= 0 && lambda <= MAX_LAMBDA, "motion_search: lambda %d is not in 0..%d", lambda, MAX_LAMBDA);
  DOVE_CHECK_ARG(cur && ref && mv_out && sad_out, "motion_search: null pointer");
  const int mbx = (w + MB - 1) / MB, mbs = mbx * ((h + MB - 1) / MB);
  const long long fs = (long long)h * w;
  hipLaunchKernelGGL(motion_search_kernel, dim3((unsigned)mbs, (unsigned)n), dim3(NT), 0, (hipStream_t)stream, cur, fs, ref, fs, 1, 0, 0, n, h, w, mbx,
                     mbs, search, lambda, mv_out, sad_out);
  DOVE_CHECK_LAUNCH("dove_motion_search_u8");
  return DOVE_OK;
}

extern "C" size_t dove_vcodec_workspace_bytes(int n, int h, int w, int gop) {
  return good_shape(n, h, w) && gop > 0 ? layout(n, h, w, gop).total : 0;
}

extern "C" int dove_vcodec_roundtrip(const float* x, int n, int h, int w, long long bitrate, int gop, void* ws, size_t ws_bytes, unsigned char* out,
                                     int* qp_out, long long* bits_out, void* stream) {
  DOVE_CHECK_ARG(good_shape(n, h, w), "vcodec_roundtrip: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(gop > 0, "vcodec_roundtrip: gop %d must be positive", gop);
  DOVE_CHECK_ARG(bitrate >= 0 && bitrate <= (1LL << 40), "vcodec_roundtrip: bitrate %lld is not in 0..2^40 bits per frame", bitrate);
  DOVE_CHECK_ARG(x && out && ws, "vcodec_roundtrip: null pointer");
  const Layout L = layout(n, h, w, gop);
  DOVE_CHECK_ARG(ws_bytes >= L.total, "vcodec_roundtrip: workspace of %zu bytes, needs %zu", ws_bytes, L.total);
  DOVE_CHECK_ARG(((uintptr_t)ws & 255) == 0, "vcodec_roundtrip: the workspace must be 256-byte aligned");
  DOVE_CHECK_ARG(L.groups <= 65535, "vcodec_roundtrip: %d groups of %d frames exceed one launch (65535)", L.groups, gop);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* base = (uint8_t*)ws;
  uint8_t *rgb = base + L.rgb, *cur = base + L.cur, *rec = base + L.rec;
  int* mv = (int*)(base + L.mv);
  unsigned long long* fbits = (unsigned long long*)(base + L.fbits);
  GroupState* state = (GroupState*)(base + L.state);

  const long long padded = (long long)n * L.ph * L.pw, pblocks = (padded + NT - 1) / NT;
  DOVE_CHECK_ARG(pblocks < (1LL << 31), "vcodec_roundtrip: %d frames of %d x %d exceed one launch", n, h, w);
  hipLaunchKernelGGL(intake_kernel, dim3((unsigned)pblocks), dim3(NT), 0, st, x, h, w, L.ph, L.pw, padded, rgb);
  DOVE_CHECK_LAUNCH("dove_vcodec_roundtrip");
  const dove_image_view view{rgb, DOVE_U8, 0, (long long)L.ph * L.pw * 3, 1, (long long)L.pw * 3, 3};
  const dove_yuv_format fwd = yuv_format(YUV_FWD), inv = yuv_format(YUV_INV);
  int rc = dove_rgb_to_yuv_u8(&view, n, L.ph, L.pw, &fwd, cur, stream);
  if (rc != DOVE_OK) return rc;

  const unsigned sblocks = (unsigned)(((n > L.groups ? n : L.groups) + NT - 1) / NT), gblocks = (unsigned)((L.groups + NT - 1) / NT);
  hipLaunchKernelGGL(rc_init_kernel, dim3(sblocks), dim3(NT), 0, st, state, L.groups, fbits, n);
  const int frames = gop < n ? gop : n;
  const dim3 sgrid((unsigned)L.mbs, (unsigned)L.groups), cgrid((unsigned)((L.mbs + MB_PER_WG - 1) / MB_PER_WG), (unsigned)L.groups);
  for (int pass = 0; pass <= QP_PASSES; ++pass) {
    for (int t = 0; t < frames; ++t) {
      if (t > 0)                                                     // the reference is the frame before, reconstructed in this pass
        hipLaunchKernelGGL(motion_search_kernel, sgrid, dim3(NT), 0, st, cur, L.fbytes, rec, L.fbytes, gop, t, -1, n, L.ph, L.pw, L.mbx, L.mbs,
                           SEARCH, LAMBDA, mv, (int*)nullptr);
      hipLaunchKernelGGL(code_kernel, cgrid, dim3(CT), 0, st, cur, rec, L.fbytes, gop, t, n, L.ph, L.pw, L.mbx, L.mbs, mv, state, fbits);
    }
    hipLaunchKernelGGL(rc_update_kernel, dim3(gblocks), dim3(NT), 0, st, state, L.groups, gop, n, bitrate, fbits, pass == QP_PASSES, qp_out, bits_out);
    DOVE_CHECK_LAUNCH("dove_vcodec_roundtrip");
  }
  const bool whole = L.ph == h && L.pw == w;                         // no padding: the inverse conversion writes the result itself
  rc = dove_yuv_to_rgb_u8(rec, n, L.ph, L.pw, &inv, whole ? out : rgb, stream);
  if (rc != DOVE_OK || whole) return rc;
  const long long total = (long long)n * h * w;
  hipLaunchKernelGGL(crop_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, rgb, h, w, L.ph, L.pw, total, out);
  DOVE_CHECK_LAUNCH("dove_vcodec_roundtrip");
  return DOVE_OK;
}
