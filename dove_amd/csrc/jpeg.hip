// JPEG encoder on the device (tests/jpeg_ref.py is the byte-exact definition of the file).
//
// A frame becomes a complete baseline JFIF file: SOI, APP0, two DQT, SOF0 (YCbCr, 4:2:0 or 4:4:4), the four Annex-K Huffman tables, DRI,
// SOS, the entropy-coded restart intervals with their RST markers, EOI.  Integer arithmetic only; the only atomics are integer LDS
// atomics (ORs into a bit buffer), so two calls give identical bytes, and no stage looks across frames, so a file does not depend on its
// batch.  The front half restates jpeg_codec_kernel of degrade.hip as far as the quantised level; that kernel is left alone.
//
//   code_kernel    one workgroup per (frame, restart interval of RESTART_MCUS = 8 MCUs; 48 blocks in 4:2:0, 24 in 4:4:4).  Pixels are read
//                  in place from the strided view (float samples quantised as dove_postprocess_u8 does), colour-converted, the chroma
//                  averaged 2x2 (4:2:0), and every 8x8 block goes through the two integer DCT passes and the quantiser; the levels stay in
//                  LDS in zigzag order and never reach HBM.  A wavefront then takes one block at a time, lane = zigzag position: the run of
//                  zeros before a coefficient comes from one ballot, the token (ZRLs, run/size code, value bits) from the code tables in
//                  LDS, the bit offset from a wave scan plus a scan over the block totals, and the bits are ORed into a big-endian LDS bit
//                  buffer.  The buffer holds the worst case: a block is at most 22 + 63 * 26 = 1660 bits (DC: 11-bit code + 11 bits; AC:
//                  16-bit code + 10 bits; a ZRL's 11 bits stand for 16 coefficients); it lies over the DCT's intermediate and the chroma
//                  planes, which are dead by then (19.7 KB of LDS in 4:2:0, 11.2 KB in 4:4:4).  The interval is padded with 1-bits to a byte and
//                  stuffed: every thread counts the 0xFF bytes of its slice, a scan gives the output offsets, and the bytes go to the
//                  interval's slot in the workspace, whose size (twice the unstuffed worst case) is a true bound.
//   scan_kernel    one workgroup per frame: interval offsets (+ 2 per RST marker), the 629-byte header, the file size.
//   gather_kernel  one workgroup per (frame, interval): the slot's bytes into place - the destination is byte-unaligned, so head and tail
//                  bytes are stored singly and whole dwords in between, shifted together from two aligned source dwords - then the RST
//                  marker, or EOI after the last interval.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr int RESTART_MCUS = 8;
constexpr int BLOCK_BITS = 22 + 63 * 26;         // 1660: the most bits one coded block takes
constexpr int BLOCK_BYTES = 208;                 // ceil(1660 / 8); an interval of b blocks is at most ceil(1660 b / 8) <= 208 b bytes
constexpr int HDR_BYTES = 629;
constexpr int CHUNK = 64;                        // frames per launch: their qualities travel as a kernel argument
constexpr int MAX_DIM = 65535;                   // SOF0 carries 16-bit sizes

struct FrameI { int v[CHUNK]; };

struct View {
  const void* data;
  int dtype;
  long long sn, sc, sh, sw;
};

// ITU-T T.81 Annex K: tables K.1 / K.2 in natural order, the zigzag sequence, and the Huffman tables K.3 - K.6 as (codes per length,
// symbols in code order).  Both AC tables end in regular rows - for run r the sizes AC_FIRST[r] .. 10 - which are generated.
constexpr int BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr int AC_HEAD_N[2] = {37, 52};
constexpr uint8_t AC_HEAD[2][52] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
     0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a}};
constexpr uint8_t AC_FIRST[2][16] = {{9, 6, 5, 4, 3, 3, 3, 3, 3, 2, 2, 2, 2, 2, 1, 1}, {11, 11, 11, 5, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2}};

struct AcVals { uint8_t v[2][162]; };

constexpr AcVals make_ac_vals() {
  AcVals a{};
  for (int t = 0; t < 2; ++t) {
    int k = 0;
    for (; k < AC_HEAD_N[t]; ++k) a.v[t][k] = AC_HEAD[t][k];
    for (int r = 0; r < 16; ++r)
      for (int s = AC_FIRST[t][r]; s <= 10; ++s) a.v[t][k++] = (uint8_t)(16 * r + s);
  }
  return a;
}
constexpr AcVals AC_VALS = make_ac_vals();

// symbol -> canonical code | length << 16 (T.81 Annex C)
struct Codes {
  uint32_t dc[2][12], ac[2][256];
};

constexpr Codes make_codes() {
  Codes c{};
  for (int t = 0; t < 2; ++t) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < DC_BITS[t][len - 1]; ++i) c.dc[t][k++] = code++ | ((uint32_t)len << 16);
      code <<= 1;
    }
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < AC_BITS[t][len - 1]; ++i) c.ac[t][AC_VALS.v[t][k++]] = code++ | ((uint32_t)len << 16);
      code <<= 1;
    }
  }
  return c;
}

// The header with quality 50's place left empty: the DQT values (25.., 94..), the size (163..166) and the luma sampling (169) are patched.
constexpr int HDR_Q0 = 25, HDR_Q1 = 94, HDR_SIZE = 163, HDR_SAMP = 169;
struct Header {
  uint8_t b[HDR_BYTES + 3];
  int n;
};

constexpr Header make_header() {
  Header h{};
  int p = 0;
  const uint8_t app0[] = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};      // JFIF 1.01, density 1:1
  for (uint8_t v : app0) h.b[p++] = v;
  for (int t = 0; t < 2; ++t) {
    const uint8_t dqt[] = {0xff, 0xdb, 0, 67, (uint8_t)t};
    for (uint8_t v : dqt) h.b[p++] = v;
    p += 64;
  }
  const uint8_t sof[] = {0xff, 0xc0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1};
  for (uint8_t v : sof) h.b[p++] = v;
  for (int i = 0; i < 4; ++i) {                  // DC luma, AC luma, DC chroma, AC chroma
    const int t = i >> 1, ac = i & 1, n = ac ? 162 : 12;
    const uint8_t dht[] = {0xff, 0xc4, (uint8_t)((n + 19) >> 8), (uint8_t)((n + 19) & 255), (uint8_t)(ac * 16 + t)};
    for (uint8_t v : dht) h.b[p++] = v;
    for (int k = 0; k < 16; ++k) h.b[p++] = ac ? AC_BITS[t][k] : DC_BITS[t][k];
    for (int k = 0; k < n; ++k) h.b[p++] = ac ? AC_VALS.v[t][k] : (uint8_t)k;
  }
  const uint8_t tail[] = {0xff, 0xdd, 0, 4, 0, RESTART_MCUS, 0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  for (uint8_t v : tail) h.b[p++] = v;
  h.n = p;
  return h;
}

struct QBase { int v[2][64]; };
constexpr QBase make_qzz() {                     // the base tables in zigzag order, as DQT carries them
  QBase q{};
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) q.v[t][k] = BASE[t][ZIGZAG[k]];
  return q;
}
constexpr QBase make_qnat() {
  QBase q{};
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) q.v[t][k] = BASE[t][k];
  return q;
}
struct Inv { uint8_t v[64]; };
constexpr Inv make_inv() {                       // natural index -> zigzag position
  Inv z{};
  for (int k = 0; k < 64; ++k) z.v[ZIGZAG[k]] = (uint8_t)k;
  return z;
}

__constant__ Codes CODES = make_codes();
static_assert(make_header().n == HDR_BYTES, "the header's segments do not add up");
__constant__ Header HEADER = make_header();
__constant__ QBase QZZ = make_qzz();
__constant__ QBase QNAT = make_qnat();
__constant__ Inv INV_ZIGZAG = make_inv();
__constant__ int COS[9] = {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799, 0};   // rint(4096 cos(m pi / 16))

struct Job {
  View v;
  int H, W, sub, mcus_x, mcus, S;                // S restart intervals per frame
  int slot;                                      // bytes of one interval's slot in the workspace
  int* isz;                                      // [frames][S] stuffed bytes of each interval
  long long* ioff;                               // [frames][S] offset of each interval in its file
  uint8_t* slots;
  uint8_t* out;
  long long bound;
  long long* sizes;
};

__device__ __forceinline__ int quant(float v) { return (int)fminf(fmaxf(v * 255.0f, 0.f), 255.f); }   // dove_postprocess_u8's rule

template <int DT>
__device__ __forceinline__ int load_q(const void* p, long long o) {
  if (DT == DOVE_U8) return ((const uint8_t*)p)[o];
  if (DT == DOVE_BF16) return quant(bf2f(((const bf16_t*)p)[o]));
  return quant(((const float*)p)[o]);
}

__device__ __forceinline__ int quality_scale(int q) { return q < 50 ? 5000 / q : 200 - 2 * q; }

// exclusive scan of one value per thread; *total = the block's sum.  tmp: NT values in LDS.
__device__ long long block_scan(long long v, long long* tmp, long long* total) {
  const int tid = threadIdx.x;
  tmp[tid] = v;
  __syncthreads();
  for (int o = 1; o < NT; o <<= 1) {
    const long long t = tid >= o ? tmp[tid - o] : 0;
    __syncthreads();
    tmp[tid] += t;
    __syncthreads();
  }
  const long long incl = tmp[tid];
  *total = tmp[NT - 1];
  __syncthreads();
  return incl - v;
}

struct Token {
  unsigned long long zrl;                        // 0..3 ZRL codes, 33 bits at most
  uint32_t code;                                 // Huffman code followed by the value bits, 27 bits at most
  int zrl_len, code_len;
};

__device__ __forceinline__ uint32_t with_value(uint32_t e, int v, int s, int* len) {
  *len = (int)(e >> 16) + s;
  return ((e & 0xffffu) << s) | (uint32_t)(v > 0 ? v : v + (1 << s) - 1);
}

// The token of zigzag position `lane` of one block (a whole wavefront calls this).  zz: the block's levels; pred: the DC predictor.
__device__ __forceinline__ Token token_of(const int16_t* zz, int lane, int pred, const uint32_t* dc, const uint32_t* ac) {
  Token t{0ull, 0u, 0, 0};
  const int v = zz[lane];
  const unsigned long long mask = __ballot(v != 0 || lane == 0);
  if (lane == 0) {
    const int d = v - pred, s = 32 - __clz(d < 0 ? -d : d);
    t.code = with_value(dc[s], d, s, &t.code_len);
  } else if (v != 0) {
    const unsigned long long below = mask & ((1ull << lane) - 1ull);           // bit 0 is always set
    const int run = lane - (63 - __clzll((long long)below)) - 1, s = 32 - __clz(v < 0 ? -v : v);
    const uint32_t z = ac[0xf0];
    for (int i = 0; i < (run >> 4); ++i) {
      t.zrl = (t.zrl << (z >> 16)) | (z & 0xffffu);
      t.zrl_len += (int)(z >> 16);
    }
    t.code = with_value(ac[((run & 15) << 4) | s], v, s, &t.code_len);
  } else if (lane == 63) {
    t.code = ac[0] & 0xffffu;                    // end of block
    t.code_len = (int)(ac[0] >> 16);
  }
  return t;
}

// len <= 33 bits of v at bit `pos` of the big-endian bit buffer
__device__ __forceinline__ void place(uint32_t* buf, unsigned long long v, int len, int pos) {
  if (len == 0) return;
  const int sh = pos & 31, w = pos >> 5;
  const unsigned long long x = v << (64 - sh - len);
  atomicOr(&buf[w], (uint32_t)(x >> 32));
  if ((uint32_t)x) atomicOr(&buf[w + 1], (uint32_t)x);
}

// the block before block b of the same component inside the interval (-1: none, the predictor is 0), and whether b is a luma block
template <int SUB>
__device__ __forceinline__ int prev_block(int b, bool* luma) {
  if (SUB == DOVE_JPEG_444) {
    *luma = b % 3 == 0;
    return b - 3;                                // negative for the first MCU
  }
  const int mcu = b / 6, j = b - mcu * 6;
  *luma = j < 4;
  if (j >= 4) return b - 6;
  if (j > 0) return b - 1;
  return mcu > 0 ? b - 3 : -1;
}

template <int DT, int SUB>
__global__ __launch_bounds__(NT) void code_kernel(Job j, FrameI quality) {
  constexpr int BPM = SUB == DOVE_JPEG_420 ? 6 : 3, MPX = SUB == DOVE_JPEG_420 ? 256 : 64;
  constexpr int MAXB = RESTART_MCUS * BPM, BUFW = (MAXB * BLOCK_BITS + 31) / 32 + 2;
  constexpr int TMP_BYTES = MAXB * 64 * 2, CHROMA_BYTES = SUB == DOVE_JPEG_420 ? 2 * RESTART_MCUS * 256 : 0;
  constexpr int RAW_WORDS = (TMP_BYTES + CHROMA_BYTES > BUFW * 4 ? TMP_BYTES + CHROMA_BYTES : BUFW * 4) / 4;
  __shared__ int16_t blk[MAXB * 64];
  __shared__ uint32_t raw[RAW_WORDS];              // first the DCT's intermediate and the chroma planes, then the bit buffer
  __shared__ int qt[2][64], ct[8][8], blk_bits[MAXB], blk_off[MAXB], wave_ff[NT / 64], total_bits;
  __shared__ uint32_t dc[2][12], ac[2][256];
  int16_t* tmp = (int16_t*)raw;
  uint8_t* chroma = (uint8_t*)raw + TMP_BYTES;
  uint32_t* buf = raw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = blockIdx.x, fr = blockIdx.y;
  const int m0 = m * RESTART_MCUS, nm = min(RESTART_MCUS, j.mcus - m0), nb = nm * BPM;

  if (tid < 128) {
    const int s = quality_scale(quality.v[fr]);
    qt[tid >> 6][tid & 63] = min(max((QNAT.v[tid >> 6][tid & 63] * s + 50) / 100, 1), 255);
  } else if (tid < 192) {
    const int u = (tid >> 3) & 7, xx = tid & 7;
    int mm = ((2 * xx + 1) * u) & 31;
    if (mm > 16) mm = 32 - mm;
    ct[u][xx] = u == 0 ? 2896 : (mm > 8 ? -COS[16 - mm] : COS[mm]);
  }
  for (int i = tid; i < 2 * 256; i += NT) ac[0][i] = CODES.ac[0][i];
  if (tid < 24) dc[0][tid] = CODES.dc[0][tid];

  // pixels -> Y, Cb, Cr (edge replication up to the whole MCU)
  for (int i = tid; i < nm * MPX; i += NT) {
    const int mcu = i / MPX, r = i - mcu * MPX;
    const int py = SUB == DOVE_JPEG_420 ? r >> 4 : r >> 3, px = SUB == DOVE_JPEG_420 ? r & 15 : r & 7;
    const int gm = m0 + mcu, mcy = gm / j.mcus_x, mcx = gm - mcy * j.mcus_x;
    const int side = SUB == DOVE_JPEG_420 ? 16 : 8;
    const int gx = min(mcx * side + px, j.W - 1), gy = min(mcy * side + py, j.H - 1);
    const long long o = (long long)fr * j.v.sn + (long long)gy * j.v.sh + (long long)gx * j.v.sw;
    const int rr = load_q<DT>(j.v.data, o), gg = load_q<DT>(j.v.data, o + j.v.sc), bb = load_q<DT>(j.v.data, o + 2 * j.v.sc);
    const int yy = (19595 * rr + 38470 * gg + 7471 * bb + 32768) >> 16;
    const int cb = (-11059 * rr - 21709 * gg + 32768 * bb + (128 << 16) + 32767) >> 16;
    const int cr = (32768 * rr - 27439 * gg - 5329 * bb + (128 << 16) + 32767) >> 16;
    if (SUB == DOVE_JPEG_420) {
      blk[(mcu * 6 + (py >> 3) * 2 + (px >> 3)) * 64 + (py & 7) * 8 + (px & 7)] = (int16_t)(yy - 128);
      chroma[mcu * 256 + r] = (uint8_t)cb;
      chroma[(RESTART_MCUS + mcu) * 256 + r] = (uint8_t)cr;
    } else {
      blk[(mcu * 3 + 0) * 64 + r] = (int16_t)(yy - 128);
      blk[(mcu * 3 + 1) * 64 + r] = (int16_t)(cb - 128);
      blk[(mcu * 3 + 2) * 64 + r] = (int16_t)(cr - 128);
    }
  }
  __syncthreads();
  if (SUB == DOVE_JPEG_420) {
    for (int i = tid; i < nm * 128; i += NT) {
      const int mcu = i >> 7, comp = (i >> 6) & 1, p = i & 63, cy = p >> 3, cx = p & 7;
      const uint8_t* c = chroma + (comp * RESTART_MCUS + mcu) * 256 + cy * 32 + cx * 2;
      blk[(mcu * 6 + 4 + comp) * 64 + p] = (int16_t)(((c[0] + c[1] + c[16] + c[17] + 1 + (cx & 1)) >> 2) - 128);   // libjpeg's alternating bias
    }
    __syncthreads();
  }
  for (int idx = tid; idx < nb * 64; idx += NT) {      // rows: t[y][u] = sum_x f[y][x] C[u][x], two fractional bits kept
    const int b = idx >> 6, y = (idx >> 3) & 7, u = idx & 7;
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += blk[b * 64 + y * 8 + i] * ct[u][i];
    tmp[b * 64 + y * 8 + u] = (int16_t)((s + 1024) >> 11);
  }
  __syncthreads();
  for (int idx = tid; idx < nb * 64; idx += NT) {      // columns: F[v][u] = sum_y t[y][u] C[v][y] (carries 2^15), then the quantiser
    const int b = idx >> 6, vv = (idx >> 3) & 7, u = idx & 7;
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += tmp[b * 64 + i * 8 + u] * ct[vv][i];
    bool luma;
    prev_block<SUB>(b, &luma);
    const int Q = qt[luma ? 0 : 1][vv * 8 + u], Qs = Q << 15;
    const int mag = ((s < 0 ? -s : s) + (Qs >> 1)) / Qs;        // round half away from zero
    int lev = s < 0 ? -mag : mag;
    lev = (vv | u) == 0 ? min(max(lev, -1024), 1023) : min(max(lev, -1023), 1023);   // what baseline Huffman coding can carry
    blk[b * 64 + INV_ZIGZAG.v[vv * 8 + u]] = (int16_t)lev;     // each block's 64 values were all read before the barrier above
  }
  __syncthreads();
  for (int i = tid; i < BUFW; i += NT) buf[i] = 0;            // tmp and chroma are dead: the barrier after the bit lengths orders this before the ORs

  // bit lengths: a wavefront per block
  for (int b = wave; b < nb; b += NT / 64) {
    bool luma;
    const int pb = prev_block<SUB>(b, &luma), t = luma ? 0 : 1;
    const Token tk = token_of(blk + b * 64, lane, pb < 0 ? 0 : blk[pb * 64], dc[t], ac[t]);
    int bits = tk.zrl_len + tk.code_len;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o);
    if (lane == 0) blk_bits[b] = bits;
  }
  __syncthreads();
  if (wave == 0) {                               // nb <= 48 block totals: one wave scan
    const int v = lane < nb ? blk_bits[lane] : 0;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane < nb) blk_off[lane] = incl - v;
    if (lane == 63) total_bits = incl;           // the interval's bits
  }
  __syncthreads();
  const int T = total_bits, nbytes = (T + 7) >> 3;
  for (int b = wave; b < nb; b += NT / 64) {
    bool luma;
    const int pb = prev_block<SUB>(b, &luma), t = luma ? 0 : 1;
    const Token tk = token_of(blk + b * 64, lane, pb < 0 ? 0 : blk[pb * 64], dc[t], ac[t]);
    const int bits = tk.zrl_len + tk.code_len;
    int incl = bits;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    const int pos = blk_off[b] + incl - bits;
    place(buf, tk.zrl, tk.zrl_len, pos);
    place(buf, tk.code, tk.code_len, pos + tk.zrl_len);
  }
  if (tid == 0) {
    const int pad = nbytes * 8 - T;              // 1-bits up to the byte
    place(buf, (1ull << pad) - 1ull, pad, T);
  }
  __syncthreads();

  // stuffing: 0xFF -> 0xFF 0x00
  const int per = (nbytes + NT - 1) / NT, beg = min(tid * per, nbytes), end = min(beg + per, nbytes);
  int ff = 0;
  for (int i = beg; i < end; ++i) ff += ((buf[i >> 2] >> (24 - 8 * (i & 3))) & 255u) == 255u ? 1 : 0;
  int incl = ff;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wave_ff[wave] = incl;
  __syncthreads();
  int excl = incl - ff, total = 0;
#pragma unroll
  for (int wv = 0; wv < NT / 64; ++wv) {
    excl += wv < wave ? wave_ff[wv] : 0;
    total += wave_ff[wv];
  }
  const long long iv = (long long)fr * j.S + m;
  uint8_t* dst = j.slots + iv * j.slot + beg + excl;         // nbytes + total <= 2 nbytes <= slot - 16
  for (int i = beg; i < end; ++i) {
    const uint32_t v = (buf[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
    *dst++ = (uint8_t)v;
    if (v == 255u) *dst++ = 0;
  }
  if (tid == 0) j.isz[iv] = nbytes + total;
}

__device__ __forceinline__ void put_be16(uint8_t* p, int v) {
  p[0] = (uint8_t)(v >> 8);
  p[1] = (uint8_t)v;
}

__global__ __launch_bounds__(NT) void scan_kernel(Job j, FrameI quality) {
  __shared__ long long stmp[NT];
  const int tid = threadIdx.x;
  const long long fr = blockIdx.x;
  const int* isz = j.isz + fr * j.S;
  long long* ioff = j.ioff + fr * j.S;
  const int per = (j.S + NT - 1) / NT, beg = min(tid * per, j.S), end = min(beg + per, j.S);   // consecutive intervals per thread
  long long mine = 0;
  for (int s = beg; s < end; ++s) mine += isz[s] + 2;
  long long total;
  long long off = HDR_BYTES + block_scan(mine, stmp, &total);
  for (int s = beg; s < end; ++s) {
    ioff[s] = off;
    off += isz[s] + 2;
  }
  const long long carry = HDR_BYTES + total;
  uint8_t* o = j.out + fr * j.bound;
  const int sc = quality_scale(quality.v[fr]);
  for (int i = tid; i < HDR_BYTES; i += NT) {
    uint8_t v = HEADER.b[i];
    if (i >= HDR_Q0 && i < HDR_Q0 + 64) v = (uint8_t)min(max((QZZ.v[0][i - HDR_Q0] * sc + 50) / 100, 1), 255);
    if (i >= HDR_Q1 && i < HDR_Q1 + 64) v = (uint8_t)min(max((QZZ.v[1][i - HDR_Q1] * sc + 50) / 100, 1), 255);
    if (i == HDR_SIZE) v = (uint8_t)(j.H >> 8);
    if (i == HDR_SIZE + 1) v = (uint8_t)j.H;
    if (i == HDR_SIZE + 2) v = (uint8_t)(j.W >> 8);
    if (i == HDR_SIZE + 3) v = (uint8_t)j.W;
    if (i == HDR_SAMP) v = j.sub == DOVE_JPEG_420 ? 0x22 : 0x11;
    o[i] = v;
  }
  if (tid == 0) j.sizes[fr] = carry;             // the last interval's + 2 is EOI
}

__global__ __launch_bounds__(NT) void gather_kernel(Job j) {
  const int tid = threadIdx.x, m = blockIdx.x;
  const long long fr = blockIdx.y, iv = fr * j.S + m;
  const int n = j.isz[iv];
  const uint8_t* src = j.slots + iv * j.slot;    // 16-byte aligned, and readable for 16 bytes past n
  uint8_t* dst = j.out + fr * j.bound + j.ioff[iv];
  const int head = min((int)((4 - ((uintptr_t)dst & 3)) & 3), n);
  if (tid < head) dst[tid] = src[tid];
  const int ndw = (n - head) >> 2, k = head & 3, a0 = head >> 2;
  const uint32_t* sw = (const uint32_t*)src;
  uint32_t* dw = (uint32_t*)(dst + head);
  for (int i = tid; i < ndw; i += NT) {
    const uint32_t lo = sw[a0 + i];
    dw[i] = k ? (lo >> (8 * k)) | (sw[a0 + i + 1] << (32 - 8 * k)) : lo;
  }
  const int done = head + 4 * ndw;
  if (tid < n - done) dst[done + tid] = src[done + tid];
  if (tid == 0) {
    dst[n] = 0xff;
    dst[n + 1] = m < j.S - 1 ? (uint8_t)(0xd0 + (m & 7)) : 0xd9;
  }
}

struct Geom {
  long long mcus_x, mcus, S, blocks;
  int slot;
};

bool good_jpeg_shape(int h, int w, int sub) { return h > 0 && w > 0 && h <= MAX_DIM && w <= MAX_DIM && (sub == DOVE_JPEG_420 || sub == DOVE_JPEG_444); }

Geom geom_of(int h, int w, int sub) {
  const long long side = sub == DOVE_JPEG_420 ? 16 : 8, bpm = sub == DOVE_JPEG_420 ? 6 : 3;
  Geom g;
  g.mcus_x = (w + side - 1) / side;
  g.mcus = g.mcus_x * ((h + side - 1) / side);
  g.S = (g.mcus + RESTART_MCUS - 1) / RESTART_MCUS;
  g.blocks = g.mcus * bpm;
  g.slot = (int)((2 * ((RESTART_MCUS * bpm * BLOCK_BITS + 7) / 8) + 16 + 15) / 16 * 16);
  return g;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Layout { size_t isz, ioff, slots, total; };

Layout layout_of(long long n, const Geom& g) {
  Layout l;
  const size_t iv = (size_t)n * (size_t)g.S;
  l.isz = 0;
  l.ioff = align_up(iv * 4, 256);
  l.slots = align_up(l.ioff + iv * 8, 256);
  l.total = l.slots + iv * (size_t)g.slot;
  return l;
}

bool plane_fits(const dove_image_view* v, int h, int w) {
  const long long lim = 1LL << 31, ah = v->sh < 0 ? -v->sh : v->sh, aw = v->sw < 0 ? -v->sw : v->sw;
  return ah < lim && aw < lim && (h - 1) * ah + (w - 1) * aw < lim;
}

template <int DT>
void launch_code(int sub, dim3 grid, hipStream_t st, const Job& j, const FrameI& q) {
  if (sub == DOVE_JPEG_420) hipLaunchKernelGGL((code_kernel<DT, DOVE_JPEG_420>), grid, dim3(NT), 0, st, j, q);
  else hipLaunchKernelGGL((code_kernel<DT, DOVE_JPEG_444>), grid, dim3(NT), 0, st, j, q);
}

}  // namespace

extern "C" int dove_jpeg_restart_mcus(void) { return RESTART_MCUS; }

// A coded block is at most 1660 bits, so an interval of b blocks is at most ceil(1660 b / 8) <= 208 b bytes with its padding; stuffing
// can at most double that; every interval is followed by a 2-byte marker (RST or EOI); the header is 629 bytes.
extern "C" size_t dove_jpeg_bound(int h, int w, int subsampling) {
  if (!good_jpeg_shape(h, w, subsampling)) return 0;
  const Geom g = geom_of(h, w, subsampling);
  return (size_t)(HDR_BYTES + 2 * BLOCK_BYTES * g.blocks + 2 * g.S);
}

extern "C" size_t dove_jpeg_workspace_bytes(int n, int h, int w, int subsampling) {
  if (n <= 0 || !good_jpeg_shape(h, w, subsampling)) return 0;
  return layout_of(n, geom_of(h, w, subsampling)).total;
}

extern "C" int dove_jpeg_encode(const dove_image_view* img, int n, int h, int w, const int* quality, int subsampling, void* ws, size_t ws_bytes,
                                unsigned char* out, long long* sizes, void* stream) {
  DOVE_CHECK_ARG(img, "jpeg_encode: null view");
  DOVE_CHECK_ARG(subsampling == DOVE_JPEG_420 || subsampling == DOVE_JPEG_444, "jpeg_encode: subsampling must be 0 (4:2:0) or 1 (4:4:4), got %d",
                 subsampling);
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0, "jpeg_encode: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(h <= MAX_DIM && w <= MAX_DIM, "jpeg_encode: a JPEG file holds at most %d x %d pixels, got %d x %d", MAX_DIM, MAX_DIM, h, w);
  DOVE_CHECK_ARG(img->dtype == DOVE_F32 || img->dtype == DOVE_BF16 || img->dtype == DOVE_U8, "jpeg_encode: bad dtype %d (0 f32, 1 bf16, 2 u8)",
                 img->dtype);
  DOVE_CHECK_ARG(plane_fits(img, h, w), "jpeg_encode: one %d x %d plane of the view spans 2^31 elements or more", h, w);
  DOVE_CHECK_ARG(quality, "jpeg_encode: null quality");
  for (int i = 0; i < n; ++i) DOVE_CHECK_ARG(quality[i] >= 1 && quality[i] <= 100, "jpeg_encode: quality[%d] = %d is not in 1..100", i, quality[i]);
  const Geom g = geom_of(h, w, subsampling);
  const Layout l = layout_of(n, g);
  DOVE_CHECK_ARG(ws_bytes >= l.total, "jpeg_encode: workspace of %zu bytes, need %zu (dove_jpeg_workspace_bytes)", ws_bytes, l.total);
  DOVE_CHECK_ARG(img->data && ws && out && sizes, "jpeg_encode: null pointer");
  DOVE_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)sizes & 7) == 0, "jpeg_encode: ws must be 16-byte and sizes 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  Job j{};
  j.v = View{img->data, img->dtype, img->sn, img->sc, img->sh, img->sw};
  j.H = h;
  j.W = w;
  j.sub = subsampling;
  j.mcus_x = (int)g.mcus_x;
  j.mcus = (int)g.mcus;
  j.S = (int)g.S;
  j.slot = g.slot;
  j.bound = (long long)dove_jpeg_bound(h, w, subsampling);
  for (int c0 = 0; c0 < n; c0 += CHUNK) {
    const int cn = n - c0 < CHUNK ? n - c0 : CHUNK;
    FrameI q{};
    for (int i = 0; i < cn; ++i) q.v[i] = quality[c0 + i];
    Job jc = j;
    const long long esz = img->dtype == DOVE_F32 ? 4 : (img->dtype == DOVE_BF16 ? 2 : 1);
    jc.v.data = (const char*)img->data + (long long)c0 * img->sn * esz;
    jc.isz = (int*)((uint8_t*)ws + l.isz) + (long long)c0 * g.S;
    jc.ioff = (long long*)((uint8_t*)ws + l.ioff) + (long long)c0 * g.S;
    jc.slots = (uint8_t*)ws + l.slots + (size_t)c0 * (size_t)g.S * (size_t)g.slot;
    jc.out = out + (size_t)c0 * (size_t)j.bound;
    jc.sizes = sizes + c0;
    const dim3 grid((unsigned)g.S, (unsigned)cn);
    if (img->dtype == DOVE_U8) launch_code<DOVE_U8>(subsampling, grid, st, jc, q);
    else if (img->dtype == DOVE_BF16) launch_code<DOVE_BF16>(subsampling, grid, st, jc, q);
    else launch_code<DOVE_F32>(subsampling, grid, st, jc, q);
    hipLaunchKernelGGL(scan_kernel, dim3((unsigned)cn), dim3(NT), 0, st, jc, q);
    hipLaunchKernelGGL(gather_kernel, grid, dim3(NT), 0, st, jc);
    DOVE_CHECK_LAUNCH("dove_jpeg_encode");
  }
  return DOVE_OK;
}
