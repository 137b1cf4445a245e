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
//
// dove_vcodec_roundtrip_tools adds an H.264 tool set (tests/vcodec_tools_ref.py is its definition, byte for byte; tools 0 issues the plain
// codec's launches).  INTRA16: intra16_kernel, one launch per anti-diagonal of macroblocks of an I frame, one wave per macroblock, code_kernel's
//   24 lanes with the V / H / DC candidates and the mode decision in front.  QPEL: qpel_kernel after each integer search, one workgroup per
//   macroblock with the 22 x 22 reference window in LDS, 9 candidates per step scored by one thread per sample; it writes the winner's
//   prediction to a plane code_kernel<true> reads, so the 6-tap filters never share registers with the transform (53 and 77 VGPRs).
//   DEBLOCK: code_kernel<true> leaves a 16-bit non-zero map per macroblock; deblock_kernel<true> walks every sample row across its vertical
//   edges, then deblock_kernel<false> every column across the horizontal ones, one thread per line, sequential along it, in place.
//   No kernel waits on another workgroup: launch order is the only synchronisation, and the bit counters stay integer atomics.
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

// One 4x4 block in registers: x holds cur - pred and leaves as the inverse transform's output before its (t + 32) >> 6.  Forward transform,
// quantisation at qp, bit count over the zigzag scan, dequantisation, inverse.  -> the block's bits; nonzero: any level != 0.
__device__ __forceinline__ int code_block(int* x, int qp, bool intra, bool& nonzero) {
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
  nonzero = nnz != 0;
  return bits;
}

// Frame t of every group: cur and rec hold n 4:2:0 payloads of PH x PW (multiples of 16), fbytes apart.  mv: [n][mbs] (dy, dx), read when t > 0.
// TOOLS (the tool set's frames that INTRA16 does not code): nzmap [n][mbs] takes bit b for every luma block b with a non-zero level; with
// predp the prediction of group g's frame is read from predp + g * fbytes (qpel_kernel wrote it) and mv holds quarter vectors (my, mx).
template <bool TOOLS>
__global__ __launch_bounds__(CT) void code_kernel(const uint8_t* __restrict__ cur, uint8_t* __restrict__ rec, long long fbytes, int gop, int t,
                                                  int n, int PH, int PW, int mbx, int mbs, const int* __restrict__ mv,
                                                  const GroupState* __restrict__ state, unsigned long long* __restrict__ fbits,
                                                  const uint8_t* __restrict__ predp, unsigned short* __restrict__ nzmap) {
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
    if (TOOLS && predp) {
      const uint8_t* pp = predp + (long long)blockIdx.y * fbytes + plane;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t wd = *(const uint32_t*)(pp + (long long)(y0 + r) * pw + x0);
#pragma unroll
        for (int c = 0; c < 4; ++c) pred[r * 4 + c] = (int)((wd >> (8 * c)) & 0xff);
      }
    } else if (luma) {
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
  bool nonzero;
  int bits = code_block(x, qp, intra, nonzero);
  if (!intra && b == 0) bits += se_len(dx) + se_len(dy);
  if (!active) bits = 0;
  if (TOOLS) {
    __shared__ unsigned char nzf[CT];
    nzf[tid] = nonzero;
    __syncthreads();
    if (active && b == 0) {
      unsigned m = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) m |= (unsigned)nzf[tid + i] << i;
      nzmap[frame * mbs + mb] = (unsigned short)m;
    }
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

// ---- the H.264 tool set (tests/vcodec_tools_ref.py is the definition) ------------------------------------------------------------------
// INTRA16: one wave per macroblock of one anti-diagonal of frame 0 of every group; the launches of a frame follow the diagonals, so the
// row above and the column to the left (macroblocks of earlier diagonals) are reconstructed when a macroblock reads them: launch order is
// the only synchronisation.  Lanes 0..23 own the 4x4 blocks as in code_kernel.  Candidates in the order V, H, DC: the luma index is that
// order, the chroma index its reverse (DC = 0, H = 1, V = 2); both winners are the minimum of (SAD + LAMBDA ue_len(index), index).
__global__ __launch_bounds__(64) void intra16_kernel(const uint8_t* __restrict__ cur, uint8_t* __restrict__ rec, long long fbytes, int gop, int n,
                                                     int PH, int PW, int mbx, int mby, int diag, const GroupState* __restrict__ state,
                                                     unsigned long long* __restrict__ fbits) {
  __shared__ int nb[3][2][16];                                       // plane, top / left, sample
  __shared__ int dcv[3], sads[BLK_PER_MB][3];
  const int tid = threadIdx.x, b = tid;
  const long long frame = (long long)blockIdx.y * gop;
  if (frame >= n) return;
  const int mr = max(0, diag - mbx + 1) + (int)blockIdx.x, mc = diag - mr;
  if (mr >= mby || mc < 0) return;                                   // the whole workgroup
  const bool has_top = mr > 0, has_left = mc > 0;
  const int qp = state[blockIdx.y].qp;
  const uint8_t* rf = rec + frame * fbytes;
  const long long cplane = (long long)PH * PW, csize = (long long)(PH / 2) * (PW / 2);
  {                                                                  // lanes 0..15 top luma, 16..31 left luma, 32..47 top chroma, 48..63 left chroma
    const int k = tid & 15, side = (tid >> 4) & 1, chroma = tid >> 5, p = chroma ? 1 + (k >> 3) : 0, i = chroma ? k & 7 : k;
    const int size = chroma ? 8 : 16, pw = chroma ? PW / 2 : PW;
    const uint8_t* pl = rf + (chroma ? cplane + (p == 2 ? csize : 0) : 0);
    int v = 0;
    if (side == 0 && has_top) v = pl[(long long)(mr * size - 1) * pw + mc * size + i];
    if (side == 1 && has_left) v = pl[(long long)(mr * size + i) * pw + mc * size - 1];
    nb[p][side][i] = v;
  }
  __syncthreads();
  if (tid < 3) {
    const int cnt = tid == 0 ? 16 : 8, sh = tid == 0 ? 4 : 3;
    int st = 0, sl = 0;
    for (int i = 0; i < cnt; ++i) {
      st += nb[tid][0][i];
      sl += nb[tid][1][i];
    }
    dcv[tid] = has_top && has_left ? (st + sl + (1 << sh)) >> (sh + 1) : has_top ? (st + (1 << (sh - 1))) >> sh : has_left ? (sl + (1 << (sh - 1))) >> sh : PRED_I;
  }
  __syncthreads();
  const bool act = b < BLK_PER_MB, luma = b < 16;
  const int j = (b - 16) & 3, p = luma ? 0 : b < 20 ? 1 : 2;
  const int pw = luma ? PW : PW / 2;
  const long long plane = luma ? 0 : cplane + (p == 2 ? csize : 0);
  const int bx = luma ? (b & 3) * 4 : (j & 1) * 4, by = luma ? (b >> 2) * 4 : (j >> 1) * 4;      // inside the macroblock's block of the plane
  const int x0 = mc * (luma ? 16 : 8) + bx, y0 = mr * (luma ? 16 : 8) + by;
  int c[16] = {}, x[16];
  if (act) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t wd = *(const uint32_t*)(cur + frame * fbytes + plane + (long long)(y0 + r) * pw + x0);
#pragma unroll
      for (int k = 0; k < 4; ++k) c[r * 4 + k] = (int)((wd >> (8 * k)) & 0xff);
    }
    int sv = 0, sh = 0, sd = 0;
    const int dc = dcv[p];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      sv += abs(c[i] - nb[p][0][bx + (i & 3)]);
      sh += abs(c[i] - nb[p][1][by + (i >> 2)]);
      sd += abs(c[i] - dc);
    }
    sads[b][0] = sv;
    sads[b][1] = sh;
    sads[b][2] = sd;
  }
  __syncthreads();
  int lsad[3] = {0, 0, 0}, csad[3] = {0, 0, 0};
  for (int i = 0; i < 16; ++i)
    for (int k = 0; k < 3; ++k) lsad[k] += sads[i][k];
  for (int i = 16; i < BLK_PER_MB; ++i)
    for (int k = 0; k < 3; ++k) csad[k] += sads[i][k];
  const bool avail[3] = {has_top, has_left, true};
  int lkey = 0x7fffffff, ckey = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!avail[k]) continue;
    lkey = min(lkey, (lsad[k] + LAMBDA * ue_len(k)) * 4 + k);
    ckey = min(ckey, (csad[k] + LAMBDA * ue_len(2 - k)) * 4 + 2 - k);
  }
  const int lmode = lkey & 3, cmode = ckey & 3, cand = luma ? lmode : 2 - cmode;
  int pred[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    pred[i] = cand == 0 ? nb[p][0][bx + (i & 3)] : cand == 1 ? nb[p][1][by + (i >> 2)] : dcv[p];
    x[i] = c[i] - pred[i];
  }
  bool nonzero;
  int bits = code_block(x, qp, true, nonzero);
  if (b == 0) bits += ue_len(lmode) + ue_len(cmode);
  if (!act) bits = 0;                                                // lanes 24..63 own no block
  if (act) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = clampi(pred[r * 4 + k] + ((x[r * 4 + k] + 32) >> 6), 0, 255);
      *(uint32_t*)(rec + frame * fbytes + plane + (long long)(y0 + r) * pw + x0) = pack4(o);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o);
  if (tid == 0) atomicAdd(fbits + frame, (unsigned long long)bits);
}

// QPEL.  The window of a macroblock: the reference around the integer winner, every coordinate clamped; a refined vector stays within
// 3 quarter samples of it, so a base sample lies at window offset 2..3 + 15 and the 6-tap reaches 0..QW - 1.
constexpr int QW = 22, QS = 23;                                      // window side, row stride in ints

__device__ __forceinline__ int tap6(int a, int b, int c, int d, int e, int f) { return a - 5 * b + 20 * (c + d) - 5 * e + f; }
__device__ __forceinline__ int clip255(int v) { return clampi(v, 0, 255); }
__device__ __forceinline__ int row6(const int* w) { return tap6(w[-2], w[-1], w[0], w[1], w[2], w[3]); }                        // b1 at w
__device__ __forceinline__ int col6(const int* w) { return tap6(w[-2 * QS], w[-QS], w[0], w[QS], w[2 * QS], w[3 * QS]); }       // h1 at w
__device__ __forceinline__ int half_b(const int* w) { return clip255((row6(w) + 16) >> 5); }
__device__ __forceinline__ int half_h(const int* w) { return clip255((col6(w) + 16) >> 5); }
__device__ __forceinline__ int half_j(const int* w) {
  return clip255((tap6(row6(w - 2 * QS), row6(w - QS), row6(w), row6(w + QS), row6(w + 2 * QS), row6(w + 3 * QS)) + 512) >> 10);
}
__device__ __forceinline__ int avg2(int a, int b) { return (a + b + 1) >> 1; }

// the luma sample of phase (fy, fx) whose integer sample G sits at w (H.264 8.4.2.2.1's names: b, h, j half samples, m = h one column to the
// right, s = b one row down)
__device__ __forceinline__ int qpel_sample(const int* w, int fy, int fx) {
  switch (fy * 4 + fx) {
    case 0: return w[0];
    case 1: return avg2(w[0], half_b(w));
    case 2: return half_b(w);
    case 3: return avg2(half_b(w), w[1]);
    case 4: return avg2(w[0], half_h(w));
    case 5: return avg2(half_b(w), half_h(w));
    case 6: return avg2(half_b(w), half_j(w));
    case 7: return avg2(half_b(w), half_h(w + 1));
    case 8: return half_h(w);
    case 9: return avg2(half_h(w), half_j(w));
    case 10: return half_j(w);
    case 11: return avg2(half_j(w), half_h(w + 1));
    case 12: return avg2(half_h(w), w[QS]);
    case 13: return avg2(half_h(w), half_b(w + QS));
    case 14: return avg2(half_j(w), half_b(w + QS));
    default: return avg2(half_h(w + 1), half_b(w + QS));
  }
}

// One workgroup per macroblock of frame t of every group, one thread per luma sample.  Two steps of 9 candidates (the centre and its
// neighbours at +-2, then at +-1 quarter samples); a candidate's phase is the same for every thread, so the switch is uniform.  The winner's
// vector goes to mvq and its prediction of the three planes to the group's frame of predp.
__global__ __launch_bounds__(NT) void qpel_kernel(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ rec, long long fbytes, int gop, int t,
                                                  int n, int PH, int PW, int mbx, int mbs, const int* __restrict__ mv, int* __restrict__ mvq,
                                                  uint8_t* __restrict__ predp) {
  __shared__ int win[QW * QS];
  __shared__ int part[2][9][NT / 64];
  const int tid = threadIdx.x, mb = blockIdx.x;
  const long long frame = (long long)blockIdx.y * gop + t;
  if (frame >= n) return;                                            // the whole workgroup
  const int x0 = (mb % mbx) * MB, y0 = (mb / mbx) * MB;
  const int2 iv = *(const int2*)(mv + 2 * (frame * mbs + mb));
  const uint8_t* rf = rec + (frame - 1) * fbytes;
  for (int i = tid; i < QW * QW; i += NT) {
    const int wy = i / QW, wx = i % QW;
    win[wy * QS + wx] = rf[(long long)clampi(y0 + iv.x - 3 + wy, 0, PH - 1) * PW + clampi(x0 + iv.y - 3 + wx, 0, PW - 1)];
  }
  const int py = tid >> 4, px = tid & 15;
  const int c = cur[frame * fbytes + (long long)(y0 + py) * PW + x0 + px];
  __syncthreads();
  int cy = 4 * iv.x, cx = 4 * iv.y;
  for (int step = 0; step < 2; ++step) {
    const int d = 2 - step;
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
      const int my = cy + (k / 3 - 1) * d, mx = cx + (k % 3 - 1) * d;
      int sad = abs(c - qpel_sample(win + (py + 3 + (my >> 2) - iv.x) * QS + px + 3 + (mx >> 2) - iv.y, my & 3, mx & 3));
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sad += __shfl_xor(sad, o);
      if ((tid & 63) == 0) part[step][k][tid >> 6] = sad;
    }
    __syncthreads();
    unsigned long long best = ~0ull;
    for (int k = 0; k < 9; ++k) {
      const int my = cy + (k / 3 - 1) * d, mx = cx + (k % 3 - 1) * d;
      const int sad = part[step][k][0] + part[step][k][1] + part[step][k][2] + part[step][k][3];
      const unsigned long long key = ((unsigned long long)(uint32_t)(sad + LAMBDA * (se_len(mx) + se_len(my))) << 32) |
                                     ((unsigned long long)(abs(my) + abs(mx)) << 20) | ((unsigned long long)(my + 512) << 10) |
                                     (unsigned long long)(mx + 512);
      best = key < best ? key : best;
    }
    cy = (int)((best >> 10) & 1023) - 512;
    cx = (int)(best & 1023) - 512;
  }
  uint8_t* pf = predp + (long long)blockIdx.y * fbytes;
  pf[(long long)(y0 + py) * PW + x0 + px] = (uint8_t)qpel_sample(win + (py + 3 + (cy >> 2) - iv.x) * QS + px + 3 + (cx >> 2) - iv.y, cy & 3, cx & 3);
  if (tid < 128) {                                                   // chroma: the vector in eighths of a chroma sample, bilinear
    const int ch = PH / 2, cw = PW / 2, yy = (y0 >> 1) + ((tid & 63) >> 3), xx = (x0 >> 1) + (tid & 7);
    const long long off = (long long)PH * PW + (tid >= 64 ? (long long)ch * cw : 0);
    const uint8_t* rp = rf + off;
    const int ya = clampi(yy + (cy >> 3), 0, ch - 1), yb = clampi(yy + (cy >> 3) + 1, 0, ch - 1);
    const int xa = clampi(xx + (cx >> 3), 0, cw - 1), xb = clampi(xx + (cx >> 3) + 1, 0, cw - 1);
    const int xf = cx & 7, yf = cy & 7;
    const int A = rp[(long long)ya * cw + xa], B = rp[(long long)ya * cw + xb], C = rp[(long long)yb * cw + xa], D = rp[(long long)yb * cw + xb];
    pf[off + (long long)yy * cw + xx] = (uint8_t)(((8 - xf) * (8 - yf) * A + xf * (8 - yf) * B + (8 - xf) * yf * C + xf * yf * D + 32) >> 6);
  }
  if (tid == 0) *(int2*)(mvq + 2 * (frame * mbs + mb)) = make_int2(cy, cx);
}

// DEBLOCK.  indexA = indexB = QP; the tables are vcodec_tools_ref's (typed from memory of H.264 Tables 8-16 / 8-17, the file is the definition).
__constant__ unsigned char DB_ALPHA[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36,
                                           40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255};
__constant__ unsigned char DB_BETA[52] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9,
                                          10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18};
__constant__ unsigned char DB_TC0[52][3] = {
    {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0},
    {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 1}, {0, 0, 1}, {0, 0, 1}, {0, 0, 1}, {0, 1, 1}, {0, 1, 1}, {1, 1, 1}, {1, 1, 1}, {1, 1, 1},
    {1, 1, 1}, {1, 1, 2}, {1, 1, 2}, {1, 1, 2}, {1, 1, 2}, {1, 2, 3}, {1, 2, 3}, {2, 2, 3}, {2, 2, 4}, {2, 3, 4}, {2, 3, 4}, {3, 3, 5}, {3, 4, 6},
    {3, 4, 6}, {4, 5, 7}, {4, 5, 8}, {4, 6, 9}, {5, 7, 10}, {6, 8, 11}, {6, 8, 13}, {7, 10, 14}, {8, 11, 16}, {9, 12, 18}, {10, 13, 20}, {11, 15, 23},
    {13, 17, 25}};

// bS of the 4-sample luma edge segment in front of 4x4 block (qy, qx): towards (qy, qx - 1) when vert, (qy - 1, qx) otherwise
__device__ __forceinline__ int edge_bs(bool intra, const unsigned short* __restrict__ nz, const int* __restrict__ mv, int mvs, int mbx, int qy, int qx,
                                       bool vert) {
  const int py = vert ? qy : qy - 1, px = vert ? qx - 1 : qx;
  const bool mbedge = ((vert ? qx : qy) & 3) == 0;
  if (intra) return mbedge ? 4 : 3;
  const int mq = (qy >> 2) * mbx + (qx >> 2), mp = (py >> 2) * mbx + (px >> 2);
  if (((nz[mq] >> ((qy & 3) * 4 + (qx & 3))) | (nz[mp] >> ((py & 3) * 4 + (px & 3)))) & 1) return 2;
  if (!mbedge) return 0;
  const int2 a = *(const int2*)(mv + 2 * mq), b = *(const int2*)(mv + 2 * mp);
  return abs(a.x - b.x) * mvs >= 4 || abs(a.y - b.y) * mvs >= 4 ? 1 : 0;
}

// p[0] = p0 (next to the edge) .. p[3], q likewise
__device__ __forceinline__ void filter_edge(int* p, int* q, int bs, bool chroma, int alpha, int beta, const int* tc0v) {
  const int p0 = p[0], p1 = p[1], p2 = p[2], q0 = q[0], q1 = q[1], q2 = q[2];
  if (bs == 0 || abs(p0 - q0) >= alpha || abs(p1 - p0) >= beta || abs(q1 - q0) >= beta) return;
  const bool ap = abs(p2 - p0) < beta, aq = abs(q2 - q0) < beta;
  if (bs < 4) {
    const int tc0 = bs == 1 ? tc0v[0] : bs == 2 ? tc0v[1] : tc0v[2], tc = chroma ? tc0 + 1 : tc0 + ap + aq;
    const int delta = clampi((4 * (q0 - p0) + (p1 - q1) + 4) >> 3, -tc, tc);
    p[0] = clip255(p0 + delta);
    q[0] = clip255(q0 - delta);
    if (chroma) return;
    const int mid = (p0 + q0 + 1) >> 1;
    if (ap) p[1] = p1 + clampi((p2 + mid - 2 * p1) >> 1, -tc0, tc0);
    if (aq) q[1] = q1 + clampi((q2 + mid - 2 * q1) >> 1, -tc0, tc0);
    return;
  }
  const bool small = abs(p0 - q0) < (alpha >> 2) + 2;
  if (!chroma && ap && small) {
    p[0] = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3;
    p[1] = (p2 + p1 + p0 + q0 + 2) >> 2;
    p[2] = (2 * p[3] + 3 * p2 + p1 + p0 + q0 + 4) >> 3;
  } else {
    p[0] = (2 * p1 + p0 + q1 + 2) >> 2;
  }
  if (!chroma && aq && small) {
    q[0] = (q2 + 2 * q1 + 2 * q0 + 2 * p0 + p1 + 4) >> 3;
    q[1] = (q2 + q1 + q0 + p0 + 2) >> 2;
    q[2] = (2 * q[3] + 3 * q2 + q1 + q0 + p0 + 4) >> 3;
  } else {
    q[0] = (2 * q1 + q0 + p1 + 2) >> 2;
  }
}

// One thread per line of a plane of frame t of every group: a sample row (VERT: the vertical edges, left to right) or a sample column (the
// horizontal edges, top to bottom; launched after the VERT pass).  The walk along a line is sequential because an edge reads what the edge
// before it left: the four samples behind an edge stay in registers as the next edge's p side, every group of four is read once and written
// once.  Lines 0 .. L - 1 are luma, then L / 2 of Cb, then L / 2 of Cr.  A chroma edge takes the bS of the luma edge at twice its position.
template <bool VERT>
__global__ __launch_bounds__(64) void deblock_kernel(uint8_t* __restrict__ rec, long long fbytes, int gop, int t, int n, int PH, int PW, int mbx,
                                                     int mbs, const unsigned short* __restrict__ nzmap, const int* __restrict__ mv, int mvs,
                                                     const GroupState* __restrict__ state) {
  const long long frame = (long long)blockIdx.y * gop + t;
  if (frame >= n) return;
  const int qp = state[blockIdx.y].qp;
  const int alpha = DB_ALPHA[qp], beta = DB_BETA[qp];
  if (alpha == 0) return;                                            // QP < 16: no edge passes |p0 - q0| < 0
  const int tc0v[3] = {DB_TC0[qp][0], DB_TC0[qp][1], DB_TC0[qp][2]};
  const int L = VERT ? PH : PW, line = blockIdx.x * 64 + threadIdx.x;
  if (line >= 2 * L) return;
  const bool chroma = line >= L, intra = t == 0;
  const int l = chroma ? (line - L) % (L / 2) : line;
  const int pw = chroma ? PW / 2 : PW, len = VERT ? pw : (chroma ? PH / 2 : PH);
  uint8_t* pl = rec + frame * fbytes + (chroma ? (long long)PH * PW + (line - L >= L / 2 ? (long long)(PH / 2) * (PW / 2) : 0) : 0);
  const long long ls = VERT ? pw : 1, ps = VERT ? 1 : pw;            // strides of a line and of a position along it
  uint8_t* base = pl + l * ls;
  const unsigned short* nz = nzmap + frame * mbs;
  const int* fmv = mv + 2 * frame * mbs;
  auto load4 = [&](int e, int* v) {
    if (VERT) {
      const uint32_t wd = *(const uint32_t*)(base + 4 * e);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (int)((wd >> (8 * i)) & 0xff);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = base[(long long)(4 * e + i) * ps];
    }
  };
  auto store4 = [&](int e, const int* v) {
    if (VERT) {
      *(uint32_t*)(base + 4 * e) = pack4(v);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) base[(long long)(4 * e + i) * ps] = (uint8_t)v[i];
    }
  };
  int a[4], p[4], q[4];
  load4(0, a);
  const int edges = len / 4, along = chroma ? l >> 1 : l >> 2;        // this line's 4x4 luma block row / column (doubled on chroma)
  for (int e = 1; e < edges; ++e) {
    load4(e, q);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = a[3 - i];
    const int across = chroma ? 2 * e : e;                            // the edge's position in 4x4 luma blocks
    const int bs = edge_bs(intra, nz, fmv, mvs, mbx, VERT ? along : across, VERT ? across : along, VERT);
    filter_edge(p, q, bs, chroma, alpha, beta, tc0v);
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = p[3 - i];
    store4(e - 1, a);
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = q[i];
  }
  store4(edges - 1, a);
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
  size_t rgb, cur, rec, mv, fbits, state, pred, mvq, nz, total;      // offsets into the workspace
};

constexpr int ALL_TOOLS = DOVE_VCODEC_INTRA16 | DOVE_VCODEC_QPEL | DOVE_VCODEC_DEBLOCK;

// tools 0 is the layout of dove_vcodec_workspace_bytes; a tool set appends a prediction frame per group, the quarter vectors and the
// macroblocks' non-zero maps
Layout layout(int n, int h, int w, int gop, int tools = 0) {
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
  L.pred = L.mvq = L.nz = o;
  if (tools != 0) {
    o += align256((size_t)L.groups * L.fbytes);
    L.mvq = o;
    o += align256((size_t)n * L.mbs * 2 * sizeof(int));
    L.nz = o;
    o += align256((size_t)n * L.mbs * sizeof(unsigned short));
  }
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

// Both round trips: tools 0 issues exactly the launches of the plain codec.
int roundtrip(const float* x, int n, int h, int w, long long bitrate, int gop, int tools, void* ws, size_t ws_bytes, unsigned char* out, int* qp_out,
              long long* bits_out, void* stream) {
  DOVE_CHECK_ARG(good_shape(n, h, w), "vcodec_roundtrip: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(gop > 0, "vcodec_roundtrip: gop %d must be positive", gop);
  DOVE_CHECK_ARG(bitrate >= 0 && bitrate <= (1LL << 40), "vcodec_roundtrip: bitrate %lld is not in 0..2^40 bits per frame", bitrate);
  DOVE_CHECK_ARG(tools >= 0 && (tools & ~ALL_TOOLS) == 0, "vcodec_roundtrip: tools %d has unknown bits (known: %d)", tools, ALL_TOOLS);
  DOVE_CHECK_ARG(x && out && ws, "vcodec_roundtrip: null pointer");
  const Layout L = layout(n, h, w, gop, tools);
  DOVE_CHECK_ARG(ws_bytes >= L.total, "vcodec_roundtrip: workspace of %zu bytes, needs %zu", ws_bytes, L.total);
  DOVE_CHECK_ARG(((uintptr_t)ws & 255) == 0, "vcodec_roundtrip: the workspace must be 256-byte aligned");
  DOVE_CHECK_ARG(L.groups <= 65535, "vcodec_roundtrip: %d groups of %d frames exceed one launch (65535)", L.groups, gop);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* base = (uint8_t*)ws;
  uint8_t *rgb = base + L.rgb, *cur = base + L.cur, *rec = base + L.rec, *pred = base + L.pred;
  int *mv = (int*)(base + L.mv), *mvq = (int*)(base + L.mvq);
  unsigned short* nz = (unsigned short*)(base + L.nz);
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
  const int frames = gop < n ? gop : n, mby = L.ph / MB;
  const bool intra16 = tools & DOVE_VCODEC_INTRA16, qpel = tools & DOVE_VCODEC_QPEL, deblock = tools & DOVE_VCODEC_DEBLOCK;
  const dim3 sgrid((unsigned)L.mbs, (unsigned)L.groups), cgrid((unsigned)((L.mbs + MB_PER_WG - 1) / MB_PER_WG), (unsigned)L.groups);
  for (int pass = 0; pass <= QP_PASSES; ++pass) {
    for (int t = 0; t < frames; ++t) {
      if (t > 0)                                                     // the reference is the frame before, as this pass left it
        hipLaunchKernelGGL(motion_search_kernel, sgrid, dim3(NT), 0, st, cur, L.fbytes, rec, L.fbytes, gop, t, -1, n, L.ph, L.pw, L.mbx, L.mbs,
                           SEARCH, LAMBDA, mv, (int*)nullptr);
      if (tools == 0) {
        hipLaunchKernelGGL(code_kernel<false>, cgrid, dim3(CT), 0, st, cur, rec, L.fbytes, gop, t, n, L.ph, L.pw, L.mbx, L.mbs, mv, state, fbits,
                           (const uint8_t*)nullptr, (unsigned short*)nullptr);
        continue;
      }
      const bool refined = t > 0 && qpel;
      if (t == 0 && intra16) {
        for (int d = 0; d < L.mbx + mby - 1; ++d) {                  // one launch per anti-diagonal of macroblocks
          const int r0 = d - L.mbx + 1 > 0 ? d - L.mbx + 1 : 0, r1 = d < mby - 1 ? d : mby - 1;
          hipLaunchKernelGGL(intra16_kernel, dim3((unsigned)(r1 - r0 + 1), (unsigned)L.groups), dim3(64), 0, st, cur, rec, L.fbytes, gop, n, L.ph, L.pw,
                             L.mbx, mby, d, state, fbits);
        }
      } else {
        if (refined)
          hipLaunchKernelGGL(qpel_kernel, sgrid, dim3(NT), 0, st, cur, rec, L.fbytes, gop, t, n, L.ph, L.pw, L.mbx, L.mbs, mv, mvq, pred);
        hipLaunchKernelGGL(code_kernel<true>, cgrid, dim3(CT), 0, st, cur, rec, L.fbytes, gop, t, n, L.ph, L.pw, L.mbx, L.mbs, refined ? mvq : mv, state,
                           fbits, refined ? pred : (const uint8_t*)nullptr, nz);
      }
      if (deblock) {                                                 // in place: the filtered frame is the output and the next reference
        const int* dmv = refined ? mvq : mv;
        const int mvs = refined ? 1 : 4;
        hipLaunchKernelGGL(deblock_kernel<true>, dim3((unsigned)((2 * L.ph + 63) / 64), (unsigned)L.groups), dim3(64), 0, st, rec, L.fbytes, gop, t, n,
                           L.ph, L.pw, L.mbx, L.mbs, nz, dmv, mvs, state);
        hipLaunchKernelGGL(deblock_kernel<false>, dim3((unsigned)((2 * L.pw + 63) / 64), (unsigned)L.groups), dim3(64), 0, st, rec, L.fbytes, gop, t, n,
                           L.ph, L.pw, L.mbx, L.mbs, nz, dmv, mvs, state);
      }
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
  return roundtrip(x, n, h, w, bitrate, gop, 0, ws, ws_bytes, out, qp_out, bits_out, stream);
}

extern "C" size_t dove_vcodec_tools_workspace_bytes(int n, int h, int w, int gop, int tools) {
  return good_shape(n, h, w) && gop > 0 && tools >= 0 && (tools & ~ALL_TOOLS) == 0 ? layout(n, h, w, gop, tools).total : 0;
}

extern "C" int dove_vcodec_roundtrip_tools(const float* x, int n, int h, int w, long long bitrate, int gop, int tools, void* ws, size_t ws_bytes,
                                           unsigned char* out, int* qp_out, long long* bits_out, void* stream) {
  return roundtrip(x, n, h, w, bitrate, gop, tools, ws, ws_bytes, out, qp_out, bits_out, stream);
}
