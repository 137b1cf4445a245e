// PNG encoder on the device (tests/png_ref.py is the bit-exact definition of the filtered stream).
//
// A frame becomes a complete PNG file: signature, IHDR, one IDAT chunk per segment, IEND.  Integer arithmetic only; the only atomics are
// integer LDS atomics, so two calls give identical bytes, and no stage looks across frames, so a file does not depend on its batch.
//
//   filter_kernel  one workgroup per (frame, row): the five PNG filters from raw pixels, libpng's heuristic (smallest sum of |int8|, ties to
//                  the lower id), then the chosen row is written to the workspace as filter byte + filtered bytes.  Float samples are
//                  quantised as dove_postprocess_u8 does, trunc(clamp(255 x, 0, 255)), so a [3,F,H,W] decoder crop is read in place.
//   build_kernel   one workgroup per (frame, segment of whole rows): histogram of the 256 byte values plus end-of-block, Adler-32 partial
//                  sums, a canonical Huffman code limited to 15 bits (flat 8/9-bit code where the built one would cost more payload bits),
//                  and the dynamic-block header (HLIT = 257, HDIST = 1 with length 0, code-length code limited to 7 bits, no repeat codes).
//   scan_kernel    one workgroup per frame: chunk offsets by a scan over the segments, the ordered Adler-32 combine, signature, IHDR, IEND
//                  and the file size.
//   pack_kernel    one workgroup per (frame, segment): header bits and Huffman codes into place through an LDS bit buffer, the empty stored
//                  block that ends the segment on a byte boundary (00 00 FF FF), the stream's tail after the last segment, and the CRC-32
//                  of the chunk (per-thread slices combined by multiplication with powers of x modulo the CRC polynomial).
//
// dove_zlib_huffman runs the build / scan / pack stages on a plain byte buffer and returns a zlib stream without PNG framing.
#include "common.h"
#include "../../include/dove_hip.h"

namespace {

constexpr int NT = 256;
constexpr long long SEGMENT_BYTES = 32768;       // filtered bytes per segment aimed at; a segment is whole rows (dove_png_segment_rows)
constexpr int NSYM = 257, EOB = 256;             // literals and end-of-block; no length codes are ever used
constexpr int MAXLEN = 15, CL_MAXLEN = 7;
constexpr int SYM_PER_THREAD = 16, CHUNK = NT * SYM_PER_THREAD;
constexpr int PACK_WORDS = (CHUNK * MAXLEN + 7 + 31) / 32 + 1;
constexpr uint32_t ADLER = 65521u, CRC_POLY = 0xEDB88320u;
constexpr int HDR_BYTES = 240;                   // 17 + 19 * 3 + 258 * 7 bits = 235 bytes at most
constexpr int TABLE_WORDS = 260;
constexpr long long MAX_SEG = 1LL << 30;         // bytes in one segment: frequencies and chunk lengths stay inside 31 bits

struct View {
  const void* data;
  int dtype;
  long long sn, sc, sh, sw;
};

struct Seg {                                     // what build leaves for scan and pack
  uint32_t hdr_bits, adler_a, adler_b, pad;
  long long data_bytes;                          // header + codes + empty stored block
  long long offset;                              // of the chunk (PNG) or of the segment's bytes (plain) inside the frame's slot
};

struct Job {
  const uint8_t* src;                            // filtered bytes (PNG) or the caller's buffer (plain)
  long long fstride, total, seg;                 // bytes between frames of src, bytes per frame, bytes per segment
  int S, png, h, w, c;
  Seg* segs;
  uint32_t* tables;                              // per segment: bit-reversed code | length << 16 for each of the 257 symbols
  uint8_t* hdrs;
  uint32_t* fadler;
  uint8_t* out;
  long long slot;
  long long* sizes;
};

__device__ __forceinline__ int quant(float v) { return (int)fminf(fmaxf(v * 255.0f, 0.f), 255.f); }   // dove_postprocess_u8's rule

template <int DT>
__device__ __forceinline__ int load_q(const void* p, long long o) {
  if (DT == DOVE_U8) return ((const uint8_t*)p)[o];
  if (DT == DOVE_BF16) return quant(bf2f(((const bf16_t*)p)[o]));
  return quant(((const float*)p)[o]);
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int filt_byte(int f, int x, int a, int b, int c) {
  switch (f) {
    case 0: return x;
    case 1: return (x - a) & 255;
    case 2: return (x - b) & 255;
    case 3: return (x - ((a + b) >> 1)) & 255;
    default: return (x - paeth(a, b, c)) & 255;
  }
}

template <int DT>
__global__ __launch_bounds__(NT) void filter_kernel(View v, int H, int W, int C, uint8_t* __restrict__ filt, long long fstride) {
  __shared__ long long part[NT / 64][5];
  __shared__ int best_s;
  const int y = (int)(blockIdx.x % (unsigned)H);
  const long long fr = blockIdx.x / (unsigned)H;
  const int rb = W * C, tid = threadIdx.x;
  const long long base = fr * v.sn + (long long)y * v.sh, up = base - v.sh;
  long long sum[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < rb; i += NT) {
    const int px = i / C, ch = i - px * C;
    const long long o = ch * v.sc + (long long)px * v.sw;
    const int x = load_q<DT>(v.data, base + o);
    const int a = px > 0 ? load_q<DT>(v.data, base + o - v.sw) : 0;
    const int b = y > 0 ? load_q<DT>(v.data, up + o) : 0;
    const int c = (y > 0 && px > 0) ? load_q<DT>(v.data, up + o - v.sw) : 0;
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const int t = filt_byte(f, x, a, b, c);
      sum[f] += t < 128 ? t : 256 - t;
    }
  }
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    const long long s = wave_sum_ll(sum[f]);
    if ((tid & 63) == 0) part[tid >> 6][f] = s;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    long long bs = 0;
    for (int f = 0; f < 5; ++f) {
      long long s = 0;
      for (int wv = 0; wv < NT / 64; ++wv) s += part[wv][f];
      if (f == 0 || s < bs) {
        bs = s;
        best = f;
      }
    }
    best_s = best;
  }
  __syncthreads();
  const int f = best_s;
  uint8_t* dst = filt + fr * fstride + (long long)y * (rb + 1);
  if (tid == 0) dst[0] = (uint8_t)f;
  for (int i = tid; i < rb; i += NT) {
    const int px = i / C, ch = i - px * C;
    const long long o = ch * v.sc + (long long)px * v.sw;
    const int x = load_q<DT>(v.data, base + o);
    const int a = px > 0 ? load_q<DT>(v.data, base + o - v.sw) : 0;
    const int b = y > 0 ? load_q<DT>(v.data, up + o) : 0;
    const int c = (y > 0 && px > 0) ? load_q<DT>(v.data, up + o - v.sw) : 0;
    dst[1 + i] = (uint8_t)filt_byte(f, x, a, b, c);
  }
}

// Code lengths of at most maxlen bits for n >= 2 symbols whose frequencies sf[] are sorted ascending; out[i] belongs to sf[i].  Huffman's
// algorithm with two queues, then the depth counts are folded to maxlen and the Kraft sum repaired one leaf at a time (the method miniz
// uses); the longest codes go to the rarest symbols.  One thread; every array lives in LDS.
__device__ void huff_lengths(const uint32_t* sf, int n, int maxlen, uint32_t* nf, uint16_t* par, uint16_t* dep, int* cnt, uint8_t* out) {
  for (int i = 0; i < n; ++i) nf[i] = sf[i];
  int li = 0, ii = n;
  for (int next = n; next < 2 * n - 1; ++next) {
    int pick[2];
    for (int k = 0; k < 2; ++k) {
      if (li < n && (ii >= next || nf[li] <= nf[ii])) pick[k] = li++;
      else pick[k] = ii++;
    }
    nf[next] = nf[pick[0]] + nf[pick[1]];
    par[pick[0]] = par[pick[1]] = (uint16_t)next;
  }
  dep[2 * n - 2] = 0;
  for (int k = 2 * n - 3; k >= 0; --k) dep[k] = dep[par[k]] + 1;
  for (int l = 0; l <= maxlen; ++l) cnt[l] = 0;
  for (int i = 0; i < n; ++i) cnt[min((int)dep[i], maxlen)]++;
  int total = 0;
  for (int l = maxlen; l > 0; --l) total += cnt[l] << (maxlen - l);
  while (total > (1 << maxlen)) {
    cnt[maxlen]--;
    for (int l = maxlen - 1; l > 0; --l)
      if (cnt[l]) {
        cnt[l]--;
        cnt[l + 1] += 2;
        break;
      }
    total--;
  }
  int j = 0;
  for (int l = maxlen; l > 0; --l)
    for (int k = 0; k < cnt[l]; ++k) out[j++] = (uint8_t)l;
}

struct BitWriter {                               // LSB-first bits into a byte array (one thread)
  uint8_t* p;
  unsigned long long acc;
  int fill, bits;
  __device__ void put(uint32_t v, int n) {
    acc |= (unsigned long long)v << fill;
    fill += n;
    bits += n;
    while (fill >= 8) {
      *p++ = (uint8_t)acc;
      acc >>= 8;
      fill -= 8;
    }
  }
  __device__ void flush() {
    if (fill > 0) *p++ = (uint8_t)acc;
  }
};

__device__ __forceinline__ void segment_of(const Job& j, int& s, long long& fr, long long& n, const uint8_t*& p) {
  s = (int)(blockIdx.x % (unsigned)j.S);
  fr = blockIdx.x / (unsigned)j.S;
  const long long beg = (long long)s * j.seg;
  n = min(j.seg, j.total - beg);
  p = j.src + fr * j.fstride + beg;
}

__global__ __launch_bounds__(NT) void build_kernel(Job j) {
  __shared__ uint32_t hist[NSYM], sfreq[NSYM], nf[2 * NSYM], next_code[MAXLEN + 1], clf[19], csf[19], clcode[19];
  __shared__ uint16_t ssym[NSYM], par[2 * NSYM], dep[2 * NSYM];
  __shared__ uint8_t lsorted[NSYM], lens[NSYM + 1], hdr[HDR_BYTES], css[19], cll[19], clsorted[19];
  __shared__ int cnt[MAXLEN + 1], nused, lcnt[MAXLEN + 1];
  __shared__ unsigned long long sa, sb, payload;
  int s;
  long long fr, n;
  const uint8_t* p;
  segment_of(j, s, fr, n, p);
  const int tid = threadIdx.x;
  for (int i = tid; i < NSYM; i += NT) hist[i] = 0;
  for (int i = tid; i < HDR_BYTES; i += NT) hdr[i] = 0;
  if (tid <= MAXLEN) lcnt[tid] = 0;
  if (tid == 0) {
    nused = 0;
    sa = sb = payload = 0;
  }
  __syncthreads();

  // histogram (a run of equal bytes costs one LDS atomic) and the Adler-32 partial sums: a = sum of bytes, b = sum of (n - i) byte[i]
  unsigned long long a = 0, b = 0;
  for (long long b0 = (long long)tid * SYM_PER_THREAD; b0 < n; b0 += CHUNK) {
    const int m = (int)min((long long)SYM_PER_THREAD, n - b0);
    int cur = p[b0], run = 0;
    for (int k = 0; k < m; ++k) {
      const int x = p[b0 + k];
      a += x;
      b += (unsigned long long)(n - b0 - k) * x;
      if (x == cur) ++run;
      else {
        atomicAdd(&hist[cur], (uint32_t)run);
        cur = x;
        run = 1;
      }
    }
    atomicAdd(&hist[cur], (uint32_t)run);
    b %= ADLER;
  }
  atomicAdd(&sa, a % ADLER);
  atomicAdd(&sb, b);
  if (tid == 0) hist[EOB] = 1;
  __syncthreads();

  // rank sort of the used symbols by (frequency, symbol)
  for (int x = tid; x < NSYM; x += NT) {
    const uint32_t f = hist[x];
    if (f) {
      int rank = 0;
      for (int k = 0; k < NSYM; ++k) {
        const uint32_t fk = hist[k];
        rank += (fk != 0 && (fk < f || (fk == f && k < x))) ? 1 : 0;
      }
      sfreq[rank] = f;
      ssym[rank] = (uint16_t)x;
      atomicAdd(&nused, 1);
    }
    lens[x] = 0;
  }
  if (tid == 0) lens[NSYM] = 0;                  // the single distance code, never used
  __syncthreads();
  if (tid == 0) huff_lengths(sfreq, nused, MAXLEN, nf, par, dep, cnt, lsorted);
  __syncthreads();
  for (int i = tid; i < nused; i += NT) {
    lens[ssym[i]] = lsorted[i];
    atomicAdd(&payload, (unsigned long long)sfreq[i] * lsorted[i]);
  }
  __syncthreads();
  const unsigned long long flat = 8ull * (unsigned long long)n + hist[255] + 9ull;
  const bool use_flat = payload > flat;          // uniform: read after the barrier
  __syncthreads();
  if (use_flat) {
    for (int x = tid; x < NSYM; x += NT) lens[x] = x < 255 ? 8 : 9;
    if (tid == 0) payload = flat;
  }
  __syncthreads();

  // canonical codes, stored bit-reversed (deflate packs Huffman codes most significant bit first)
  for (int x = tid; x < NSYM; x += NT)
    if (lens[x]) atomicAdd(&lcnt[lens[x]], 1);
  __syncthreads();
  if (tid == 0) {
    uint32_t code = 0;
    next_code[0] = 0;
    for (int l = 1; l <= MAXLEN; ++l) {
      code = (code + (l > 1 ? (uint32_t)lcnt[l - 1] : 0u)) << 1;
      next_code[l] = code;
    }
  }
  __syncthreads();
  uint32_t* table = j.tables + (long long)blockIdx.x * TABLE_WORDS;
  for (int x = tid; x < NSYM; x += NT) {
    const int l = lens[x];
    uint32_t e = 0;
    if (l) {
      uint32_t code = next_code[l];
      for (int k = 0; k < x; ++k) code += lens[k] == l ? 1u : 0u;
      e = (__brev(code) >> (32 - l)) | ((uint32_t)l << 16);
    }
    table[x] = e;
  }

  // the block header: the 258 code lengths, each sent with a code of the code-length alphabet (symbols 0..15 only)
  if (tid == 0) {
    for (int k = 0; k < 19; ++k) {
      clf[k] = 0;
      cll[k] = 0;
    }
    for (int x = 0; x <= NSYM; ++x) clf[lens[x]]++;
    int m = 0;
    for (int k = 0; k < 19; ++k) {
      if (!clf[k]) continue;
      int q = m++;
      while (q > 0 && csf[q - 1] > clf[k]) {
        csf[q] = csf[q - 1];
        css[q] = css[q - 1];
        --q;
      }
      csf[q] = clf[k];
      css[q] = (uint8_t)k;
    }
    huff_lengths(csf, m, CL_MAXLEN, nf, par, dep, cnt, clsorted);
    for (int i = 0; i < m; ++i) cll[css[i]] = clsorted[i];
    uint32_t code = 0;
    for (int l = 1; l <= CL_MAXLEN; ++l) {
      for (int k = 0; k < 19; ++k)
        if (cll[k] == l) clcode[k] = __brev(code++) >> (32 - l);
      code <<= 1;
    }
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = 19;
    while (hclen > 4 && cll[order[hclen - 1]] == 0) --hclen;
    BitWriter bw{hdr, 0ull, 0, 0};
    bw.put(0, 1);                                // BFINAL = 0
    bw.put(2, 2);                                // BTYPE = dynamic Huffman
    bw.put(0, 5);                                // HLIT = 257
    bw.put(0, 5);                                // HDIST = 1
    bw.put((uint32_t)(hclen - 4), 4);
    for (int k = 0; k < hclen; ++k) bw.put(cll[order[k]], 3);
    for (int x = 0; x <= NSYM; ++x) bw.put(clcode[lens[x]], cll[lens[x]]);
    bw.flush();
    Seg sg;
    sg.hdr_bits = (uint32_t)bw.bits;
    sg.adler_a = (uint32_t)(sa % ADLER);
    sg.adler_b = (uint32_t)(sb % ADLER);
    sg.pad = 0;
    sg.data_bytes = (long long)(((unsigned long long)bw.bits + payload + 3 + 7) >> 3) + 4;
    sg.offset = 0;
    j.segs[blockIdx.x] = sg;
  }
  __syncthreads();
  uint8_t* gh = j.hdrs + (long long)blockIdx.x * HDR_BYTES;
  for (int i = tid; i < HDR_BYTES; i += NT) gh[i] = hdr[i];
}

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

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

__device__ uint32_t crc_serial(const uint8_t* p, int n) {
  uint32_t c = 0xffffffffu;
  for (int i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
  }
  return ~c;
}

__device__ __forceinline__ long long chunk_bytes(const Job& j, int s, long long data_bytes) {
  return data_bytes + (s == 0 ? 2 : 0) + (s == j.S - 1 ? 6 : 0) + (j.png ? 12 : 0);
}

__global__ __launch_bounds__(NT) void scan_kernel(Job j) {
  __shared__ long long tmp[NT];
  __shared__ unsigned long long sa, sb;
  const int tid = threadIdx.x;
  const long long fr = blockIdx.x;
  Seg* segs = j.segs + fr * j.S;
  if (tid == 0) sa = sb = 0;
  long long carry = j.png ? 33 : 0;
  unsigned long long a = 0, b = 0;
  for (int c0 = 0; c0 < j.S; c0 += NT) {
    const int s = c0 + tid;
    long long v = 0;
    if (s < j.S) {
      const Seg sg = segs[s];
      v = chunk_bytes(j, s, sg.data_bytes);
      const long long after = j.total - min(j.total, (long long)(s + 1) * j.seg);
      a = (a + sg.adler_a) % ADLER;
      b = (b + sg.adler_b + (unsigned long long)sg.adler_a * (unsigned long long)(after % ADLER)) % ADLER;
    }
    long long total;
    const long long excl = block_scan(v, tmp, &total);
    if (s < j.S) segs[s].offset = carry + excl;
    carry += total;
  }
  atomicAdd(&sa, a);
  atomicAdd(&sb, b);
  __syncthreads();
  if (tid == 0) {
    const uint32_t fa = (uint32_t)((1 + sa) % ADLER), fb = (uint32_t)(((unsigned long long)(j.total % ADLER) + sb) % ADLER);
    j.fadler[fr] = (fb << 16) | fa;
    uint8_t* o = j.out + fr * j.slot;
    if (j.png) {
      const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
      for (int k = 0; k < 8; ++k) o[k] = sig[k];
      put_be32(o + 8, 13);
      o[12] = 'I'; o[13] = 'H'; o[14] = 'D'; o[15] = 'R';
      put_be32(o + 16, (uint32_t)j.w);
      put_be32(o + 20, (uint32_t)j.h);
      o[24] = 8;
      o[25] = j.c == 3 ? 2 : 0;
      o[26] = o[27] = o[28] = 0;
      put_be32(o + 29, crc_serial(o + 12, 17));
      uint8_t* e = o + carry;
      put_be32(e, 0);
      e[4] = 'I'; e[5] = 'E'; e[6] = 'N'; e[7] = 'D';
      put_be32(e + 8, 0xAE426082u);
      carry += 12;
    }
    j.sizes[fr] = carry;
  }
}

// a(x) b(x) mod the CRC polynomial, bit-reflected: bit 31 is x^0
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 0x80000000u; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}

__global__ __launch_bounds__(NT) void pack_kernel(Job j) {
  __shared__ uint32_t tab[TABLE_WORDS], buf[PACK_WORDS], crct[256], cc[NT];
  __shared__ long long tmp[NT];
  int s;
  long long fr, n;
  const uint8_t* p;
  segment_of(j, s, fr, n, p);
  const int tid = threadIdx.x;
  const Seg sg = j.segs[blockIdx.x];
  const bool first = s == 0, last = s == j.S - 1;
  const long long dlen = sg.data_bytes + (first ? 2 : 0) + (last ? 6 : 0);
  uint8_t* chunk = j.out + fr * j.slot + sg.offset;
  uint8_t* d = chunk + (j.png ? 8 : 0);
  if (tid == 0) {
    if (j.png) {
      put_be32(chunk, (uint32_t)dlen);
      chunk[4] = 'I'; chunk[5] = 'D'; chunk[6] = 'A'; chunk[7] = 'T';
    }
    if (first) {
      d[0] = 0x78;                               // deflate, 32 KiB window
      d[1] = 0x01;                               // no preset dictionary, fastest level; 0x7801 is a multiple of 31
    }
  }
  uint8_t* o = d + (first ? 2 : 0);
  const uint32_t* table = j.tables + (long long)blockIdx.x * TABLE_WORDS;
  for (int i = tid; i < NSYM; i += NT) tab[i] = table[i];
  {
    uint32_t c = (uint32_t)tid;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
    crct[tid] = c;
  }
  const uint8_t* gh = j.hdrs + (long long)blockIdx.x * HDR_BYTES;
  const int hb = (int)(sg.hdr_bits >> 3);
  for (int i = tid; i < hb; i += NT) o[i] = gh[i];
  int carry_bits = (int)(sg.hdr_bits & 7);
  uint32_t carry_val = carry_bits ? (uint32_t)gh[hb] & ((1u << carry_bits) - 1u) : 0u;
  long long opos = hb;
  __syncthreads();

  for (long long c0 = 0; c0 <= n; c0 += CHUNK) {           // symbols 0 .. n - 1 are the bytes, symbol n is the end-of-block
    for (int i = tid; i < PACK_WORDS; i += NT) buf[i] = 0;
    const long long b0 = c0 + (long long)tid * SYM_PER_THREAD;
    const int m = (int)max(0LL, min((long long)SYM_PER_THREAD, n + 1 - b0));
    uint32_t e[SYM_PER_THREAD];
    int bits = 0;
#pragma unroll
    for (int k = 0; k < SYM_PER_THREAD; ++k) {
      e[k] = 0;
      if (k < m) {
        const int sym = b0 + k < n ? (int)p[b0 + k] : EOB;
        e[k] = tab[sym];
        bits += (int)(e[k] >> 16);
      }
    }
    long long total;
    const long long excl = block_scan(bits, tmp, &total);   // its barriers also order the zeroing of buf before the ORs below
    if (tid == 0 && carry_bits) atomicOr(&buf[0], carry_val);
    const long long ob = carry_bits + excl;
    unsigned long long acc = 0;
    int fill = (int)(ob & 31), wi = (int)(ob >> 5);
#pragma unroll
    for (int k = 0; k < SYM_PER_THREAD; ++k) {
      if (k < m) {
        acc |= (unsigned long long)(e[k] & 0xffffu) << fill;
        fill += (int)(e[k] >> 16);
        if (fill >= 32) {
          atomicOr(&buf[wi++], (uint32_t)acc);
          acc >>= 32;
          fill -= 32;
        }
      }
    }
    if (fill > 0 && acc) atomicOr(&buf[wi], (uint32_t)acc);
    __syncthreads();
    const long long T = carry_bits + total;
    const int full = (int)(T >> 3);
    for (int i = tid; i < full; i += NT) o[opos + i] = (uint8_t)(buf[i >> 2] >> ((i & 3) * 8));
    carry_bits = (int)(T & 7);
    carry_val = carry_bits ? (buf[full >> 2] >> ((full & 3) * 8)) & ((1u << carry_bits) - 1u) : 0u;
    opos += full;
    __syncthreads();
  }

  if (tid == 0) {
    uint8_t* q = o + opos;                       // the empty stored block: 3 header bits, padding, LEN = 0, NLEN = 0xffff
    int k = 0;
    q[k++] = (uint8_t)carry_val;
    if (carry_bits + 3 > 8) q[k++] = 0;
    q[k++] = 0; q[k++] = 0; q[k++] = 0xff; q[k++] = 0xff;
    if (last) {                                  // a final, empty fixed-Huffman block, then the Adler-32
      q[k++] = 0x03;
      q[k++] = 0x00;
      put_be32(q + k, j.fadler[fr]);
    }
  }
  if (!j.png) return;
  __syncthreads();

  // CRC-32 over the chunk type and data.  Thread t takes slice t of 256 equal slices that END at the data's end (the first ones may be
  // empty or short); the register state after a slice, times x^(8 * bytes that follow), summed, is the state after all bytes.
  const long long len = dlen + 4, L = (len + NT - 1) / NT;
  const uint8_t* cp = chunk + 4;
  const long long end = len - (long long)(NT - 1 - tid) * L, beg = end - L;
  uint32_t st = (beg <= 0 && end > 0) ? 0xffffffffu : 0u;
  for (long long i = max(beg, 0LL); i < end; ++i) st = crct[(st ^ cp[i]) & 0xff] ^ (st >> 8);
  uint32_t pw = 0x80000000u, bs = 0x00800000u;   // x^0, x^8
  for (long long ex = L; ex; ex >>= 1) {
    if (ex & 1) pw = crc_mul(pw, bs);
    bs = crc_mul(bs, bs);
  }
  cc[tid] = st;
  __syncthreads();
  for (int cnt = NT / 2; cnt >= 1; cnt >>= 1) {
    uint32_t v = 0;
    if (tid < cnt) v = crc_mul(cc[2 * tid], pw) ^ cc[2 * tid + 1];
    __syncthreads();
    if (tid < cnt) cc[tid] = v;
    __syncthreads();
    pw = crc_mul(pw, pw);
  }
  if (tid == 0) put_be32(chunk + 8 + dlen, ~cc[0]);
}

struct Layout {
  size_t segs, tables, fadler, hdrs, filt, total;
  long long fstride;
};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ws: Seg records, code tables, per-frame Adler-32, header bytes, then (PNG) the filtered frames
Layout layout_of(long long n, long long S, long long filt_bytes_per_frame) {
  Layout l;
  const size_t nseg = (size_t)n * (size_t)S;
  l.segs = 0;
  l.tables = align_up(nseg * sizeof(Seg), 256);
  l.fadler = align_up(l.tables + nseg * TABLE_WORDS * 4, 256);
  l.hdrs = align_up(l.fadler + (size_t)n * 4, 256);
  l.filt = align_up(l.hdrs + nseg * HDR_BYTES, 256);
  l.fstride = (long long)align_up((size_t)filt_bytes_per_frame, 256);
  l.total = l.filt + (size_t)n * (size_t)l.fstride;
  return l;
}

bool good_png_shape(long long h, long long w, int c) { return h > 0 && w > 0 && (c == 1 || c == 3) && w * c + 1 <= MAX_SEG && h < (1LL << 31); }

long long seg_rows(long long w, int c) { return (SEGMENT_BYTES + w * c) / (w * c + 1); }

long long bound_of(long long bytes, long long S) { return (bytes * 9 + 7) / 8 + 256 * S + 64; }

bool plane_fits(const dove_image_view* v, int h, int w) {
  const long long lim = 1LL << 31, ah = v->sh < 0 ? -v->sh : v->sh, aw = v->sw < 0 ? -v->sw : v->sw;
  return ah < lim && aw < lim && (h - 1) * ah + (w - 1) * aw < lim;
}

void fill_job(Job& j, const Layout& l, void* ws) {
  uint8_t* b = (uint8_t*)ws;
  j.segs = (Seg*)(b + l.segs);
  j.tables = (uint32_t*)(b + l.tables);
  j.fadler = (uint32_t*)(b + l.fadler);
  j.hdrs = b + l.hdrs;
}

void launch_coder(const Job& j, long long n, hipStream_t st) {
  const unsigned blocks = (unsigned)(n * j.S);
  hipLaunchKernelGGL(build_kernel, dim3(blocks), dim3(NT), 0, st, j);
  hipLaunchKernelGGL(scan_kernel, dim3((unsigned)n), dim3(NT), 0, st, j);
  hipLaunchKernelGGL(pack_kernel, dim3(blocks), dim3(NT), 0, st, j);
}

}  // namespace

extern "C" int dove_png_segment_rows(int w, int channels) {
  if (!good_png_shape(1, w, channels)) return 0;
  return (int)seg_rows(w, channels);
}

extern "C" size_t dove_png_bound(int h, int w, int channels) {
  if (!good_png_shape(h, w, channels)) return 0;
  const long long R = seg_rows(w, channels), S = ((long long)h + R - 1) / R;
  return (size_t)bound_of((long long)h * ((long long)w * channels + 1), S);
}

extern "C" size_t dove_png_workspace_bytes(int n, int h, int w, int channels) {
  if (n <= 0 || !good_png_shape(h, w, channels)) return 0;
  const long long R = seg_rows(w, channels), S = ((long long)h + R - 1) / R;
  return layout_of(n, S, (long long)h * ((long long)w * channels + 1)).total;
}

extern "C" int dove_png_encode(const dove_image_view* img, int n, int h, int w, int channels, void* ws, size_t ws_bytes, unsigned char* out,
                               long long* sizes, void* stream) {
  DOVE_CHECK_ARG(img, "png_encode: null view");
  DOVE_CHECK_ARG(n > 0 && h > 0 && w > 0, "png_encode: bad shape n=%d h=%d w=%d", n, h, w);
  DOVE_CHECK_ARG(channels == 1 || channels == 3, "png_encode: channels must be 1 (grey) or 3 (RGB), got %d", channels);
  DOVE_CHECK_ARG(good_png_shape(h, w, channels), "png_encode: a row of %d x %d bytes is too long", w, channels);
  DOVE_CHECK_ARG(img->dtype == DOVE_F32 || img->dtype == DOVE_BF16 || img->dtype == DOVE_U8, "png_encode: bad dtype %d (0 f32, 1 bf16, 2 u8)",
                 img->dtype);
  DOVE_CHECK_ARG(plane_fits(img, h, w), "png_encode: one %d x %d plane of the view spans 2^31 elements or more", h, w);
  const long long rb = (long long)w * channels, R = seg_rows(w, channels), S = ((long long)h + R - 1) / R;
  DOVE_CHECK_ARG(R * (rb + 1) <= MAX_SEG, "png_encode: a segment of %lld rows is too long", R);
  DOVE_CHECK_ARG((long long)n * S < (1LL << 31) && (long long)n * h < (1LL << 31), "png_encode: n=%d frames of %d x %d exceed one launch", n, h, w);
  const Layout l = layout_of(n, S, (long long)h * (rb + 1));
  DOVE_CHECK_ARG(ws_bytes >= l.total, "png_encode: workspace of %zu bytes, need %zu (dove_png_workspace_bytes)", ws_bytes, l.total);
  DOVE_CHECK_ARG(img->data && ws && out && sizes, "png_encode: null pointer");
  DOVE_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)sizes & 7) == 0, "png_encode: ws and sizes must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const View v{img->data, img->dtype, img->sn, img->sc, img->sh, img->sw};
  uint8_t* filt = (uint8_t*)ws + l.filt;
  const unsigned rows = (unsigned)((long long)n * h);
  if (img->dtype == DOVE_U8) hipLaunchKernelGGL(filter_kernel<DOVE_U8>, dim3(rows), dim3(NT), 0, st, v, h, w, channels, filt, l.fstride);
  else if (img->dtype == DOVE_BF16) hipLaunchKernelGGL(filter_kernel<DOVE_BF16>, dim3(rows), dim3(NT), 0, st, v, h, w, channels, filt, l.fstride);
  else hipLaunchKernelGGL(filter_kernel<DOVE_F32>, dim3(rows), dim3(NT), 0, st, v, h, w, channels, filt, l.fstride);
  Job j{};
  j.src = filt;
  j.fstride = l.fstride;
  j.total = (long long)h * (rb + 1);
  j.seg = R * (rb + 1);
  j.S = (int)S;
  j.png = 1;
  j.h = h;
  j.w = w;
  j.c = channels;
  fill_job(j, l, ws);
  j.out = out;
  j.slot = (long long)dove_png_bound(h, w, channels);
  j.sizes = sizes;
  launch_coder(j, n, st);
  DOVE_CHECK_LAUNCH("dove_png_encode");
  return DOVE_OK;
}

extern "C" size_t dove_zlib_huffman_bound(long long nbytes, long long segment_bytes) {
  if (nbytes <= 0 || segment_bytes < 1024 || segment_bytes > (1 << 20)) return 0;
  return (size_t)bound_of(nbytes, (nbytes + segment_bytes - 1) / segment_bytes);
}

extern "C" size_t dove_zlib_huffman_workspace_bytes(long long nbytes, long long segment_bytes) {
  if (nbytes <= 0 || segment_bytes < 1024 || segment_bytes > (1 << 20)) return 0;
  return layout_of(1, (nbytes + segment_bytes - 1) / segment_bytes, 0).total;
}

extern "C" int dove_zlib_huffman(const unsigned char* in, long long nbytes, long long segment_bytes, void* ws, size_t ws_bytes,
                                 unsigned char* out, long long* size, void* stream) {
  DOVE_CHECK_ARG(nbytes > 0, "zlib_huffman: nbytes must be positive, got %lld", nbytes);
  DOVE_CHECK_ARG(segment_bytes >= 1024 && segment_bytes <= (1 << 20), "zlib_huffman: segment_bytes %lld outside 1 KiB .. 1 MiB", segment_bytes);
  const long long S = (nbytes + segment_bytes - 1) / segment_bytes;
  DOVE_CHECK_ARG(S < (1LL << 31), "zlib_huffman: %lld bytes in segments of %lld exceed one launch", nbytes, segment_bytes);
  const Layout l = layout_of(1, S, 0);
  DOVE_CHECK_ARG(ws_bytes >= l.total, "zlib_huffman: workspace of %zu bytes, need %zu (dove_zlib_huffman_workspace_bytes)", ws_bytes, l.total);
  DOVE_CHECK_ARG(in && ws && out && size, "zlib_huffman: null pointer");
  DOVE_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)size & 7) == 0, "zlib_huffman: ws and size must be 8-byte aligned");
  Job j{};
  j.src = in;
  j.fstride = 0;
  j.total = nbytes;
  j.seg = segment_bytes;
  j.S = (int)S;
  j.png = 0;
  fill_job(j, l, ws);
  j.out = out;
  j.slot = 0;
  j.sizes = size;
  launch_coder(j, 1, (hipStream_t)stream);
  DOVE_CHECK_LAUNCH("dove_zlib_huffman");
  return DOVE_OK;
}
