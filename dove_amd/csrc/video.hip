// Whole videos at the graph level (include/dove_hip.h "whole videos from C"): the script around process_video
// (/root/reference/inference_script.py:192-361 padding / chunks / tiles / valid regions, :670-731 the chunk x tile loop, stitch, coverage
// check and crop) as library code.
//   1. the host planner: dove_amd/tiling.py and dove_amd.stream.ChunkPlanner restated in C (integer logic, no GPU);
//   2. dove_randn: a counter-based normal generator (Philox4x32-10 + Box-Muller) a C host can reproduce;
//   3. dove_stitch: the valid box of a piece into the chunk buffer, one launch, no write counts;
//   4. dove_video_*: the streaming session that chains the operator entry points per chunk exactly as dove_amd.stream.sr_stream orders
//      them, so its bytes equal that composition's.
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "common.h"
#include "philox.h"
#include "../../include/dove_hip.h"
#include "ctx_access.h"

namespace {

#define VCHK(expr)              \
  do {                          \
    const int rc__ = (expr);    \
    if (rc__ != 0) return rc__; \
  } while (0)
#define VHIPCHK(expr)                                                 \
  do {                                                                \
    const hipError_t e__ = (expr);                                    \
    if (e__ != hipSuccess) {                                          \
      dove_set_error("%s failed: %s", #expr, hipGetErrorString(e__)); \
      return DOVE_ELAUNCH;                                            \
    }                                                                 \
  } while (0)

const char* const MSG_LACK = "Error: Lack of write in region !!!";
const char* const MSG_DOUBLE = "Error: Write count > 1 in region !!!";

// ================================================================ 1. host planner ================================================
// range(0, total - overlap, length - overlap) + the reference's border start (tiling._axis_starts)
void axis_starts(int total, int length, int overlap, bool allow_empty_fix, std::vector<int>* st) {
  st->clear();
  const int stride = length - overlap;
  for (long long s = 0; s < (long long)total - overlap; s += stride) st->push_back((int)s);
  if ((allow_empty_fix && st->empty()) || (!st->empty() && st->back() + length < total)) st->push_back(total - length);
}

int temporal_chunks(int F, int chunk_len, int overlap_t, std::vector<std::pair<int, int>>* out) {
  out->clear();
  if (chunk_len == 0) { out->push_back({0, F}); return 0; }
  DOVE_CHECK_ARG(chunk_len - overlap_t > 0, "chunk_len must be greater than overlap");
  std::vector<int> st;
  axis_starts(F, chunk_len, overlap_t, false, &st);
  for (int s : st) out->push_back({s, std::min(s + chunk_len, F)});
  if (out->size() >= 2 && out->back().second - out->back().first < chunk_len) {      // a short tail is merged (ref :274-277)
    const int end = out->back().second;
    out->pop_back();
    out->back().second = end;
  }
  return 0;
}

struct Tile { int h0, h1, w0, w1; };
int spatial_tiles(int H, int W, int th, int tw, int oh, int ow, std::vector<Tile>* out) {
  out->clear();
  if (th == 0 || tw == 0) { out->push_back({0, H, 0, W}); return 0; }
  const int sh = th - oh, sw = tw - ow;
  DOVE_CHECK_ARG(sh > 0 && sw > 0, "Tile size must be greater than overlap");
  auto starts = [](int total, int length, int overlap, std::vector<int>* st) {
    axis_starts(total, length, overlap, true, st);
    if (st->size() >= 2 && st->back() + length > total) st->pop_back();              // "merge last row/col" (ref :303-327)
  };
  std::vector<int> hs, ws;
  starts(H, th, oh, &hs);
  starts(W, tw, ow, &ws);
  for (int h0 : hs) {
    int h1 = std::min(h0 + th, H);
    if (h1 + sh > H) h1 = H;
    for (int w0 : ws) {
      int w1 = std::min(w0 + tw, W);
      if (w1 + sw > W) w1 = W;
      out->push_back({h0, h1, w0, w1});
    }
  }
  return 0;
}

// get_valid_tile_region: axis by axis, half of an interior overlap is dropped on each side
void valid_region(const int* piece, const int* full, const int* ov, int* valid, int* out) {
  for (int a = 0; a < 3; ++a) {
    const int lo = piece[2 * a], hi = piece[2 * a + 1], n = hi - lo;
    const int vs = lo == 0 ? 0 : ov[a] / 2;
    const int ve = hi == full[a] ? n : n - ov[a] / 2;
    valid[2 * a] = vs; valid[2 * a + 1] = ve;
    out[2 * a] = lo + vs; out[2 * a + 1] = lo + ve;
  }
}

// Exactly-once cover of [0,F) x [0,H) x [0,W) by integer boxes: count the boxes over every cell of the grid their faces cut the domain
// into (a 3-D difference array, prefix-summed) - the boxes of a plan share almost all their faces, so the grid is tiny.
int check_coverage(const int* boxes, int n, int F, int H, int W) {
  DOVE_CHECK_ARG(n >= 0 && (boxes || n == 0) && F >= 0 && H >= 0 && W >= 0, "dove_plan_check_coverage: bad arguments");
  if ((long long)F * H * W == 0) return DOVE_OK;                 // an empty region has nothing to miss (torch: any() of an empty tensor)
  const int full[3] = {F, H, W};
  std::vector<int> cut[3];
  for (int a = 0; a < 3; ++a) { cut[a].push_back(0); cut[a].push_back(full[a]); }
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const int lo = boxes[6 * i + 2 * a], hi = boxes[6 * i + 2 * a + 1];
      DOVE_CHECK_ARG(lo >= 0 && hi <= full[a], "dove_plan_check_coverage: box %d reaches outside the region", i);
      if (hi > lo) { cut[a].push_back(lo); cut[a].push_back(hi); }
    }
  size_t dim[3];
  for (int a = 0; a < 3; ++a) {
    std::sort(cut[a].begin(), cut[a].end());
    cut[a].erase(std::unique(cut[a].begin(), cut[a].end()), cut[a].end());
    dim[a] = cut[a].size();                                     // cells = dim - 1; the difference array needs the closing face too
  }
  DOVE_CHECK_ARG(dim[0] * dim[1] * dim[2] <= ((size_t)1 << 26), "dove_plan_check_coverage: %d boxes cut the region into too many cells", n);
  std::vector<int> d(dim[0] * dim[1] * dim[2], 0);
  auto at = [&](size_t t, size_t h, size_t w) -> int& { return d[(t * dim[1] + h) * dim[2] + w]; };
  auto idx = [&](int a, int v) { return (size_t)(std::lower_bound(cut[a].begin(), cut[a].end(), v) - cut[a].begin()); };
  for (int i = 0; i < n; ++i) {
    const int* b = boxes + 6 * i;
    if (b[1] <= b[0] || b[3] <= b[2] || b[5] <= b[4]) continue;
    const size_t t0 = idx(0, b[0]), t1 = idx(0, b[1]), h0 = idx(1, b[2]), h1 = idx(1, b[3]), w0 = idx(2, b[4]), w1 = idx(2, b[5]);
    at(t0, h0, w0) += 1; at(t1, h0, w0) -= 1; at(t0, h1, w0) -= 1; at(t0, h0, w1) -= 1;
    at(t1, h1, w0) += 1; at(t1, h0, w1) += 1; at(t0, h1, w1) += 1; at(t1, h1, w1) -= 1;
  }
  for (size_t t = 0; t < dim[0]; ++t) for (size_t h = 0; h < dim[1]; ++h) for (size_t w = 1; w < dim[2]; ++w) at(t, h, w) += at(t, h, w - 1);
  for (size_t t = 0; t < dim[0]; ++t) for (size_t h = 1; h < dim[1]; ++h) for (size_t w = 0; w < dim[2]; ++w) at(t, h, w) += at(t, h - 1, w);
  for (size_t t = 1; t < dim[0]; ++t) for (size_t h = 0; h < dim[1]; ++h) for (size_t w = 0; w < dim[2]; ++w) at(t, h, w) += at(t - 1, h, w);
  bool lack = false, twice = false;
  for (size_t t = 0; t + 1 < dim[0]; ++t) for (size_t h = 0; h + 1 < dim[1]; ++h) for (size_t w = 0; w + 1 < dim[2]; ++w) {
    const int cnt = at(t, h, w);
    lack |= cnt == 0;
    twice |= cnt > 1;
  }
  DOVE_CHECK_ARG(!lack, "%s", MSG_LACK);                        // the reference tests the hole first (ref :724-729)
  DOVE_CHECK_ARG(!twice, "%s", MSG_DOUBLE);
  return DOVE_OK;
}

}  // namespace

// stream.ChunkPlanner
struct dove_chunk_planner { int chunk_len = 0, overlap_t = 0; long long start = 0; bool done = false; };

namespace {
inline long long lookahead(const dove_chunk_planner& p) { return 2ll * p.chunk_len - p.overlap_t; }
// 1: a chunk, 0: none left, < 0: called too early
int planner_next(dove_chunk_planner* p, long long known, bool eof, long long* t0, long long* t1, int* last) {
  if (p->done) return 0;
  const long long s = p->start, n = p->chunk_len, ov = p->overlap_t;
  if (n == 0) {
    DOVE_CHECK_ARG(eof, "chunk_len == 0 is one piece of the whole clip: the planner needs the end of the stream");
    p->done = true;
    *t0 = 0; *t1 = known; *last = 1;
    return 1;
  }
  bool is_last;
  if (!eof) {
    DOVE_CHECK_ARG(known >= s + lookahead(*p), "the chunk at %lld needs %lld known frames or the end of the stream, got %lld", s,
                   s + lookahead(*p), known);
    is_last = false;
  } else if (s == 0 && known <= ov) {
    p->done = true;                                             // make_temporal_chunks returns no chunk at all
    return 0;
  } else {
    is_last = known <= s + n || known - (s + n - ov) < n;       // the clip ends inside it / the next chunk is short and merged
  }
  *t0 = s; *t1 = is_last ? known : s + n; *last = is_last ? 1 : 0;
  p->start = s + n - ov;
  p->done = is_last;
  return 1;
}
}  // namespace

extern "C" int dove_plan_padding(int F, int H, int W, int* pad_f, int* pad_h, int* pad_w) {
  DOVE_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "dove_plan_padding: bad shape %d x %d x %d", F, H, W);
  const int rem = (F - 1) % 8;
  if (pad_f) *pad_f = rem ? 8 - rem : 0;
  if (pad_h) *pad_h = (16 - H % 16) % 16;
  if (pad_w) *pad_w = (16 - W % 16) % 16;
  return DOVE_OK;
}
extern "C" int dove_plan_output_size(int H, int W, int upscale, int* out_h, int* out_w) {
  DOVE_CHECK_ARG(H >= 1 && W >= 1 && upscale >= 1, "dove_plan_output_size: bad arguments");
  int pad_h, pad_w;
  VCHK(dove_plan_padding(1, H, W, nullptr, &pad_h, &pad_w));
  if (out_h) *out_h = (H + pad_h) * upscale - pad_h * 4;       // the reference's hard-coded 4 (ref :731)
  if (out_w) *out_w = (W + pad_w) * upscale - pad_w * 4;
  return DOVE_OK;
}
extern "C" int dove_plan_temporal_chunks(int F, int chunk_len, int overlap_t, int* chunks, int cap) {
  DOVE_CHECK_ARG(F >= 0 && chunk_len >= 0 && overlap_t >= 0, "dove_plan_temporal_chunks: negative argument");
  std::vector<std::pair<int, int>> c;
  VCHK(temporal_chunks(F, chunk_len, overlap_t, &c));
  for (size_t i = 0; chunks && i < c.size() && (int)i < cap; ++i) { chunks[2 * i] = c[i].first; chunks[2 * i + 1] = c[i].second; }
  return (int)c.size();
}
extern "C" int dove_plan_spatial_tiles(int H, int W, int tile_h, int tile_w, int overlap_h, int overlap_w, int* tiles, int cap) {
  DOVE_CHECK_ARG(H >= 0 && W >= 0 && tile_h >= 0 && tile_w >= 0 && overlap_h >= 0 && overlap_w >= 0, "dove_plan_spatial_tiles: negative argument");
  std::vector<Tile> t;
  VCHK(spatial_tiles(H, W, tile_h, tile_w, overlap_h, overlap_w, &t));
  for (size_t i = 0; tiles && i < t.size() && (int)i < cap; ++i) {
    tiles[4 * i] = t[i].h0; tiles[4 * i + 1] = t[i].h1; tiles[4 * i + 2] = t[i].w0; tiles[4 * i + 3] = t[i].w1;
  }
  return (int)t.size();
}
extern "C" int dove_plan_valid_region(const int* piece, int F, int H, int W, int overlap_t, int overlap_h, int overlap_w, int* valid, int* out) {
  DOVE_CHECK_ARG(piece && valid && out, "dove_plan_valid_region: null pointer");
  const int full[3] = {F, H, W}, ov[3] = {overlap_t, overlap_h, overlap_w};
  valid_region(piece, full, ov, valid, out);
  return DOVE_OK;
}
extern "C" int dove_plan_pieces(int F, int H, int W, int chunk_len, int overlap_t, int tile_h, int tile_w, int overlap_h, int overlap_w,
                                int* pieces, int* valid, int* out, int cap) {
  DOVE_CHECK_ARG(F >= 0 && H >= 0 && W >= 0 && chunk_len >= 0 && overlap_t >= 0 && tile_h >= 0 && tile_w >= 0 && overlap_h >= 0 && overlap_w >= 0,
                 "dove_plan_pieces: negative argument");
  const int ov_t = chunk_len > 0 ? overlap_t : 0;
  const bool tiled = !(tile_h == 0 && tile_w == 0);
  const int ov[3] = {ov_t, tiled ? overlap_h : 0, tiled ? overlap_w : 0}, full[3] = {F, H, W};
  std::vector<std::pair<int, int>> chunks;
  std::vector<Tile> tiles;
  VCHK(temporal_chunks(F, chunk_len, ov_t, &chunks));
  if (chunks.empty()) return 0;                                  // the reference never reaches make_spatial_tiles
  VCHK(spatial_tiles(H, W, tile_h, tile_w, ov[1], ov[2], &tiles));
  int n = 0;
  for (const auto& c : chunks)
    for (const auto& t : tiles) {
      if (n < cap) {
        const int p[6] = {c.first, c.second, t.h0, t.h1, t.w0, t.w1};
        int v[6], o[6];
        valid_region(p, full, ov, v, o);
        if (pieces) memcpy(pieces + 6 * n, p, sizeof p);
        if (valid) memcpy(valid + 6 * n, v, sizeof v);
        if (out) memcpy(out + 6 * n, o, sizeof o);
      }
      ++n;
    }
  return n;
}
extern "C" int dove_plan_check_coverage(const int* boxes, int n, int F, int H, int W) { return check_coverage(boxes, n, F, H, W); }

extern "C" int dove_chunk_planner_create(int chunk_len, int overlap_t, dove_chunk_planner** out) {
  DOVE_CHECK_ARG(out, "dove_chunk_planner_create: null pointer");
  DOVE_CHECK_ARG(chunk_len >= 0 && overlap_t >= 0, "dove_chunk_planner_create: negative argument");
  DOVE_CHECK_ARG(chunk_len == 0 || chunk_len - overlap_t > 0, "chunk_len must be greater than overlap");
  dove_chunk_planner* p = new dove_chunk_planner();
  p->chunk_len = chunk_len;
  p->overlap_t = chunk_len ? overlap_t : 0;
  *out = p;
  return DOVE_OK;
}
extern "C" long long dove_chunk_planner_need(const dove_chunk_planner* p) {
  return !p || p->chunk_len == 0 ? -1 : p->start + lookahead(*p);
}
extern "C" int dove_chunk_planner_next(dove_chunk_planner* p, long long known, int eof, long long* t0, long long* t1, int* last) {
  DOVE_CHECK_ARG(p && t0 && t1 && last, "dove_chunk_planner_next: null pointer");
  return planner_next(p, known, eof != 0, t0, t1, last);
}
extern "C" void dove_chunk_planner_destroy(dove_chunk_planner* p) { delete p; }

// ================================================================ 2. dove_randn ==================================================
namespace {

// MODE 0: raw words (uint32), 1: normals fp32, 2: normals bf16.  One thread per Philox block; the blocks are walked grid-stride, so the
// values depend on (seed, stream, element index) alone.  A block whose four elements all lie inside [offset, offset + n) and land on a
// 16-byte (bf16: 8-byte) boundary of `out` leaves as one vector store.
template <int MODE>
__global__ void philox_kernel(void* __restrict__ out, long long n, uint64_t seed, uint64_t stream_id, uint64_t offset, long long nblocks,
                              int aligned) {
  const uint64_t first = offset >> 2;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nblocks; j += (long long)gridDim.x * blockDim.x) {
    const uint64_t b = first + (uint64_t)j;
    const Words wd = philox4x32_10(b, stream_id, seed);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE != 0) {
      box_muller(wd.x[0], wd.x[1], &z[0], &z[1]);
      box_muller(wd.x[2], wd.x[3], &z[2], &z[3]);
    }
    const long long e0 = (long long)(b * 4 - offset);           // index in `out` of the block's first element (may be negative: wraps are impossible, n < 2^62)
    if (aligned && e0 >= 0 && e0 + 4 <= n) {
      if (MODE == 0) *(uint4*)((uint32_t*)out + e0) = make_uint4(wd.x[0], wd.x[1], wd.x[2], wd.x[3]);
      else if (MODE == 1) *(float4*)((float*)out + e0) = make_float4(z[0], z[1], z[2], z[3]);
      else *(uint2*)((bf16_t*)out + e0) = make_uint2(pack_bf2(z[0], z[1]), pack_bf2(z[2], z[3]));
    } else {
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const long long e = e0 + l;
        if (e < 0 || e >= n) continue;
        if (MODE == 0) ((uint32_t*)out)[e] = wd.x[l];
        else if (MODE == 1) ((float*)out)[e] = z[l];
        else ((bf16_t*)out)[e] = (bf16_t)(pack_bf2(z[l], 0.f) & 0xffffu);
      }
    }
  }
}

int philox_launch(int mode, void* out, long long n, uint64_t seed, uint64_t stream_id, uint64_t offset, void* stream, const char* what) {
  DOVE_CHECK_ARG(n >= 0 && n < (1ll << 62) && offset < (1ull << 62), "%s: n / offset out of range", what);
  if (n == 0) return DOVE_OK;
  DOVE_CHECK_ARG(out, "%s: null pointer", what);
  const uint64_t first = offset >> 2, lastb = (offset + (uint64_t)n - 1) >> 2;
  const long long nblocks = (long long)(lastb - first + 1);
  const size_t vec = mode == 2 ? 8 : 16;
  const int aligned = (offset & 3) == 0 && ((uintptr_t)out % vec) == 0;
  const long long want = (nblocks + 255) / 256;
  const unsigned grid = (unsigned)(want < 2048 ? want : 2048);
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0) hipLaunchKernelGGL(philox_kernel<0>, dim3(grid), dim3(256), 0, s, out, n, seed, stream_id, offset, nblocks, aligned);
  else if (mode == 1) hipLaunchKernelGGL(philox_kernel<1>, dim3(grid), dim3(256), 0, s, out, n, seed, stream_id, offset, nblocks, aligned);
  else hipLaunchKernelGGL(philox_kernel<2>, dim3(grid), dim3(256), 0, s, out, n, seed, stream_id, offset, nblocks, aligned);
  DOVE_CHECK_LAUNCH(what);
  return DOVE_OK;
}

}  // namespace

extern "C" int dove_philox_u32(void* out, long long n, unsigned long long seed, unsigned long long stream_id, unsigned long long offset,
                               void* stream) {
  return philox_launch(0, out, n, seed, stream_id, offset, stream, "dove_philox_u32");
}
extern "C" int dove_randn(void* out, int dtype, long long n, unsigned long long seed, unsigned long long stream_id, unsigned long long offset,
                          void* stream) {
  DOVE_CHECK_ARG(dtype == DOVE_F32 || dtype == DOVE_BF16, "dove_randn: bad dtype %d", dtype);
  return philox_launch(dtype == DOVE_F32 ? 1 : 2, out, n, seed, stream_id, offset, stream, "dove_randn");
}

// ================================================================ 3. dove_stitch =================================================
namespace {

// box [3][nt][nh][nw] between two [3][.][.][.] bf16 arrays: element (c, t, y, x) at base + c*sc + t*st + y*sh + x.  VEC = 8: 16-byte units.
struct BoxSide { long long sc, st, sh; };
template <int VEC>
__global__ void box_copy_kernel(const bf16_t* __restrict__ src, BoxSide ss, bf16_t* __restrict__ dst, BoxSide ds, int nt, int nh, int nwv) {
  const long long total = 3ll * nt * nh * nwv;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int xv = (int)(i % nwv);
    long long r = i / nwv;
    const int y = (int)(r % nh);
    r /= nh;
    const int t = (int)(r % nt), c = (int)(r / nt);
    const long long so = c * ss.sc + t * ss.st + y * ss.sh + (long long)xv * VEC, dof = c * ds.sc + t * ds.st + y * ds.sh + (long long)xv * VEC;
    if (VEC == 8) *(uint4*)(dst + dof) = *(const uint4*)(src + so);
    else dst[dof] = src[so];
  }
}

// src / dst already point at the first element of their boxes
int box_copy(const bf16_t* src, BoxSide ss, bf16_t* dst, BoxSide ds, int nt, int nh, int nw, hipStream_t s, const char* what) {
  if (nt <= 0 || nh <= 0 || nw <= 0) return DOVE_OK;
  auto m8 = [](long long v) { return v % 8 == 0; };
  const bool vec = nw % 8 == 0 && m8(ss.sc) && m8(ss.st) && m8(ss.sh) && m8(ds.sc) && m8(ds.st) && m8(ds.sh) && (uintptr_t)src % 16 == 0 &&
                   (uintptr_t)dst % 16 == 0;
  const int nwv = vec ? nw / 8 : nw;
  const long long total = 3ll * nt * nh * nwv, want = (total + 255) / 256;
  const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
  if (vec) hipLaunchKernelGGL(box_copy_kernel<8>, dim3(grid), dim3(256), 0, s, src, ss, dst, ds, nt, nh, nwv);
  else hipLaunchKernelGGL(box_copy_kernel<1>, dim3(grid), dim3(256), 0, s, src, ss, dst, ds, nt, nh, nwv);
  DOVE_CHECK_LAUNCH(what);
  return DOVE_OK;
}

}  // namespace

extern "C" int dove_stitch(const void* piece, int f, int h, int w, const int* valid, void* chunk, int f_chunk, int Hs, int Ws, int out_t0,
                           int out_h0, int out_w0, void* stream) {
  DOVE_CHECK_ARG(piece && chunk && valid, "dove_stitch: null pointer");
  DOVE_CHECK_ARG(f > 0 && h > 0 && w > 0 && f_chunk > 0 && Hs > 0 && Ws > 0, "dove_stitch: bad shape");
  const int nt = valid[1] - valid[0], nh = valid[3] - valid[2], nw = valid[5] - valid[4];
  DOVE_CHECK_ARG(valid[0] >= 0 && valid[1] <= f && valid[2] >= 0 && valid[3] <= h && valid[4] >= 0 && valid[5] <= w && nt >= 0 && nh >= 0 && nw >= 0,
                 "dove_stitch: the valid box (%d:%d, %d:%d, %d:%d) does not fit inside the %d x %d x %d piece", valid[0], valid[1], valid[2],
                 valid[3], valid[4], valid[5], f, h, w);
  DOVE_CHECK_ARG(out_t0 >= 0 && out_h0 >= 0 && out_w0 >= 0 && out_t0 + nt <= f_chunk && out_h0 + nh <= Hs && out_w0 + nw <= Ws,
                 "dove_stitch: a %d x %d x %d box at (%d, %d, %d) does not fit inside the %d x %d x %d chunk", nt, nh, nw, out_t0, out_h0, out_w0,
                 f_chunk, Hs, Ws);
  const BoxSide ss{(long long)f * h * w, (long long)h * w, w}, ds{(long long)f_chunk * Hs * Ws, (long long)Hs * Ws, Ws};
  const bf16_t* src = (const bf16_t*)piece + valid[0] * ss.st + valid[2] * ss.sh + valid[4];
  bf16_t* dst = (bf16_t*)chunk + out_t0 * ds.st + out_h0 * ds.sh + out_w0;
  return box_copy(src, ss, dst, ds, nt, nh, nw, (hipStream_t)stream, "dove_stitch");
}

// ================================================================ 4. the session =================================================
namespace {

inline size_t al(size_t v) { return (v + 255) / 256 * 256; }

struct Layout {                       // the session's one allocation, sized from the parameters alone
  int pad_h = 0, pad_w = 0, Hs = 0, Ws = 0, Ho = 0, Wo = 0;
  int fmax = 0, ring_frames = 0, th_max = 0, tw_max = 0, ntiles = 0;
  bool whole = false;                 // one tile that is the whole frame: pieces read the chunk's video in place
  size_t in_fb = 0, out_fb = 0;
  size_t ring = 0, stage = 0, rgb = 0, video = 0, out = 0, tile_in = 0, piece = 0, noise = 0, eps = 0, fixed = 0, cf_ws = 0, total = 0;
  size_t cf_ws_bytes = 0;
  std::vector<Tile> tiles;
};

int valid_yuv(const dove_yuv_format& f) { return f.chroma >= DOVE_YUV_444 && f.chroma <= DOVE_YUV_MONO; }

int make_layout(const dove_model_config* cf, const dove_video_params* p, Layout* L) {
  DOVE_CHECK_ARG(p, "dove_video: null parameters");
  DOVE_CHECK_ARG(p->struct_size == sizeof(dove_video_params), "dove_video_params.struct_size is %u, this library's is %zu", p->struct_size,
                 sizeof(dove_video_params));
  DOVE_CHECK_ARG(p->width >= 1 && p->height >= 1 && p->upscale >= 1 && p->upscale <= 16, "dove_video: bad frame size / upscale");
  DOVE_CHECK_ARG(p->chunk_len >= 0 && p->overlap_t >= 0 && p->tile_h >= 0 && p->tile_w >= 0 && p->overlap_h >= 0 && p->overlap_w >= 0,
                 "dove_video: negative chunk / tile setting");
  DOVE_CHECK_ARG(p->chunk_len == 0 || p->chunk_len - p->overlap_t > 0, "chunk_len must be greater than overlap");
  DOVE_CHECK_ARG(p->color_fix == 0 || p->color_fix == DOVE_COLORFIX_WAVELET || p->color_fix == DOVE_COLORFIX_ADAIN, "dove_video: bad color_fix %d", p->color_fix);
  DOVE_CHECK_ARG((p->in_format == DOVE_VIDEO_RGB_U8 || (p->in_format == DOVE_VIDEO_YUV && valid_yuv(p->in_yuv))) &&
                 (p->out_format == DOVE_VIDEO_RGB_U8 || (p->out_format == DOVE_VIDEO_YUV && valid_yuv(p->out_yuv))), "dove_video: bad input / output format");
  DOVE_CHECK_ARG(p->text && p->text_len >= 1, "dove_video: no text embedding");
  DOVE_CHECK_ARG(p->max_push >= 0 && p->max_frames >= 0, "dove_video: negative max_push / max_frames");
  DOVE_CHECK_ARG(p->chunk_len > 0 || p->max_frames >= 1, "dove_video: chunk_len 0 is one piece of the whole clip: max_frames must say how long it can be");
  VCHK(dove_plan_padding(1, p->height, p->width, nullptr, &L->pad_h, &L->pad_w));
  const long long Hs = (long long)(p->height + L->pad_h) * p->upscale, Ws = (long long)(p->width + L->pad_w) * p->upscale;
  DOVE_CHECK_ARG(Hs <= 16384 && Ws <= 16384, "dove_video: upscaled frames of %lld x %lld are too large", Ws, Hs);
  L->Hs = (int)Hs; L->Ws = (int)Ws;
  VCHK(dove_plan_output_size(p->height, p->width, p->upscale, &L->Ho, &L->Wo));
  DOVE_CHECK_ARG(L->Ho >= 1 && L->Wo >= 1, "dove_video: x%d leaves nothing after the reference's pad * 4 crop", p->upscale);
  const bool tiled = !(p->tile_h == 0 && p->tile_w == 0);
  VCHK(spatial_tiles(L->Hs, L->Ws, p->tile_h, p->tile_w, tiled ? p->overlap_h : 0, tiled ? p->overlap_w : 0, &L->tiles));
  L->ntiles = (int)L->tiles.size();
  for (const auto& t : L->tiles) {
    DOVE_CHECK_ARG(t.h0 >= 0 && t.w0 >= 0 && t.h1 > t.h0 && t.w1 > t.w0, "dove_video: tile size %d x %d is larger than the %d x %d frames", p->tile_h, p->tile_w, L->Hs, L->Ws);
    DOVE_CHECK_ARG((t.h1 - t.h0) % 16 == 0 && (t.w1 - t.w0) % 16 == 0, "dove_video: a %d x %d tile is not a multiple of 16 (tile size and overlap must be)", t.h1 - t.h0, t.w1 - t.w0);
    L->th_max = std::max(L->th_max, t.h1 - t.h0);
    L->tw_max = std::max(L->tw_max, t.w1 - t.w0);
  }
  L->whole = L->ntiles == 1 && L->tiles[0].h0 == 0 && L->tiles[0].w0 == 0 && L->tiles[0].h1 == L->Hs && L->tiles[0].w1 == L->Ws;
  if (p->chunk_len > 0) {
    L->fmax = 2 * p->chunk_len - p->overlap_t - 1;               // a merged tail is shorter than chunk_len + stride
    L->ring_frames = 2 * p->chunk_len - p->overlap_t + (p->max_push ? p->max_push : 64);
  } else {
    int pad_f;
    VCHK(dove_plan_padding(p->max_frames, 1, 1, &pad_f, nullptr, nullptr));
    L->fmax = p->max_frames + pad_f;
    L->ring_frames = p->max_frames;
  }
  L->in_fb = p->in_format == DOVE_VIDEO_YUV ? dove_yuv_frame_bytes(p->height, p->width, p->in_yuv.chroma) : (size_t)p->height * p->width * 3;
  L->out_fb = p->out_format == DOVE_VIDEO_YUV ? dove_yuv_frame_bytes(L->Ho, L->Wo, p->out_yuv.chroma) : (size_t)L->Ho * L->Wo * 3;
  DOVE_CHECK_ARG(L->in_fb && L->out_fb, "dove_video: bad YUV layout");
  const size_t fm = (size_t)L->fmax;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += al(bytes); return o; };
  L->ring = take((size_t)L->ring_frames * L->in_fb);
  L->stage = take(fm * L->in_fb);
  L->rgb = p->in_format == DOVE_VIDEO_YUV ? take(fm * p->height * p->width * 3) : L->stage;
  L->video = take(3 * fm * L->Hs * L->Ws * 2);
  L->out = take(3 * fm * L->Hs * L->Ws * 2);
  L->tile_in = L->whole ? L->video : take(3 * fm * L->th_max * L->tw_max * 2);
  L->piece = take(3 * fm * L->th_max * L->tw_max * 2);
  const int tc = cf->vae_temporal_compression, Tmax = 1 + (L->fmax - 1) / tc, Tdmax = Tmax + cf->dit_patch_t;
  const size_t lat = (size_t)cf->vae_latent_channels * (L->th_max / 8) * (L->tw_max / 8);
  L->noise = take(lat * Tmax * 4);
  L->eps = p->noise_step ? take(lat * Tdmax * 4) : 0;
  L->cf_ws_bytes = p->color_fix ? dove_color_fix_workspace_bytes(p->color_fix, L->fmax, L->Ho, L->Wo) : 0;
  L->cf_ws = p->color_fix ? take(L->cf_ws_bytes) : 0;
  L->fixed = p->color_fix && p->out_format == DOVE_VIDEO_YUV ? take(fm * L->Ho * L->Wo * 3) : 0;
  L->total = off;
  return DOVE_OK;
}

}  // namespace

struct dove_video {
  dove_ctx* ctx = nullptr;
  dove_video_params p;
  Layout L;
  char* mem = nullptr;
  dove_chunk_planner planner;
  long long base = 0, total = 0;      // input frames [base, total) are in the ring, frame t in slot t % ring_frames
  bool eof = false, done = false;
  long long pieces = 0, chunks = 0;   // piece ordinal over the whole video (noise streams 2p, 2p + 1)
  long long written_end = 0;          // frames [0, written_end) of the padded clip have been written by the chunks so far
};

extern "C" size_t dove_video_workspace_bytes(dove_ctx* ctx, const dove_video_params* params) {
  const dove_model_config* cf = dove_ctx_config(ctx);
  if (!cf) { dove_set_error("dove_video_workspace_bytes: the context is not finalized (dove_finalize_weights)"); return 0; }
  Layout L;
  return make_layout(cf, params, &L) == DOVE_OK ? L.total : 0;
}

extern "C" int dove_video_open(dove_ctx* ctx, const dove_video_params* params, dove_video** out) {
  DOVE_CHECK_ARG(ctx && out, "dove_video_open: null pointer");
  const dove_model_config* cf = dove_ctx_config(ctx);
  DOVE_CHECK_ARG(cf, "dove_video_open: the context is not finalized (dove_finalize_weights)");
  DOVE_CHECK_ARG(dove_ctx_nranks(ctx) == 1, "dove_video_open: the context has a communicator (%d ranks); the whole-video session runs on a single-rank "
                 "context (the sharded single-clip mode is dove_sr_clip's)", dove_ctx_nranks(ctx));
  dove_video* v = new dove_video();
  const int rc = make_layout(cf, params, &v->L);
  if (rc != DOVE_OK) { delete v; return rc; }
  v->ctx = ctx;
  v->p = *params;
  v->planner.chunk_len = params->chunk_len;
  v->planner.overlap_t = params->chunk_len ? params->overlap_t : 0;
  // the arena is sized for the largest piece now, not when that piece turns up: what a piece keeps in flight depends on the room it finds, so
  // the memory a clip needs would otherwise depend on where its longest chunk falls
  const int rs = dove_ctx_reserve(ctx, v->L.fmax, v->L.th_max, v->L.tw_max);
  if (rs != DOVE_OK) { delete v; return rs; }
  hipError_t e = hipSetDevice(dove_ctx_device(ctx));
  void* mem = nullptr;
  if (e == hipSuccess) e = hipMalloc(&mem, v->L.total);
  if (e != hipSuccess) {
    dove_set_error("dove_video_open: allocating the session's %zu bytes failed: %s", v->L.total, hipGetErrorString(e));
    delete v;
    return DOVE_ELAUNCH;
  }
  v->mem = (char*)mem;
  *out = v;
  return DOVE_OK;
}

extern "C" void dove_video_close(dove_video* v) {
  if (!v) return;
  if (v->mem) { (void)hipSetDevice(dove_ctx_device(v->ctx)); (void)hipDeviceSynchronize(); (void)hipFree(v->mem); }   // work of the last step may still run
  delete v;
}

extern "C" int dove_video_info(const dove_video* v, size_t* in_frame_bytes, size_t* out_frame_bytes, int* out_h, int* out_w, int* max_step_frames) {
  DOVE_CHECK_ARG(v, "dove_video_info: null session");
  if (in_frame_bytes) *in_frame_bytes = v->L.in_fb;
  if (out_frame_bytes) *out_frame_bytes = v->L.out_fb;
  if (out_h) *out_h = v->L.Ho;
  if (out_w) *out_w = v->L.Wo;
  if (max_step_frames) *max_step_frames = v->L.fmax;
  return DOVE_OK;
}

extern "C" int dove_video_push(dove_video* v, const void* frames, int n, void* stream) {
  DOVE_CHECK_ARG(v && (frames || n == 0) && n >= 0, "dove_video_push: bad arguments");
  DOVE_CHECK_ARG(!v->eof, "dove_video_push: after dove_video_end_of_input");
  const int cap = v->L.ring_frames;
  DOVE_CHECK_ARG(v->total + n - v->base <= cap, "dove_video_push: %d more frames do not fit (%lld held, room for %d): push what dove_video_need "
                 "asks for plus at most max_push%s", n, v->total - v->base, cap, v->p.chunk_len ? "" : "; chunk_len 0 holds the whole clip, max_frames");
  const size_t fb = v->L.in_fb;
  for (int i = 0; i < n;) {                                     // at most two runs: the ring wraps once
    const int slot = (int)((v->total + i) % cap), run = std::min(n - i, cap - slot);
    VHIPCHK(hipMemcpyAsync(v->mem + v->L.ring + (size_t)slot * fb, (const char*)frames + (size_t)i * fb, (size_t)run * fb, hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    i += run;
  }
  v->total += n;
  return DOVE_OK;
}

extern "C" int dove_video_end_of_input(dove_video* v) {
  DOVE_CHECK_ARG(v, "dove_video_end_of_input: null session");
  v->eof = true;
  return DOVE_OK;
}

extern "C" int dove_video_need(const dove_video* v, long long* frames, int* end_of_input) {
  DOVE_CHECK_ARG(v, "dove_video_need: null session");
  long long f = 0;
  int e = 0;
  if (!v->eof && !v->done) {
    const long long need = dove_chunk_planner_need(&v->planner);
    if (need < 0) e = 1;
    else f = std::max(0ll, need - v->total);
  }
  if (frames) *frames = f;
  if (end_of_input) *end_of_input = e;
  return DOVE_OK;
}

extern "C" int dove_video_step(dove_video* v, void* out, size_t out_bytes, int* frames_written, int* done, void* stream) {
  DOVE_CHECK_ARG(v && frames_written, "dove_video_step: null pointer");
  *frames_written = 0;
  if (done) *done = v->done ? 1 : 0;
  if (v->done) return DOVE_OK;
  const Layout& L = v->L;
  const dove_video_params& p = v->p;
  const dove_model_config* cf = dove_ctx_config(v->ctx);
  DOVE_CHECK_ARG(cf && dove_ctx_nranks(v->ctx) == 1, "dove_video_step: the context got a communicator after the session was opened");
  DOVE_CHECK_ARG(!(v->eof && v->total == 0), "the input stream holds no frame");
  // ---- the plan of this step, on a copy of the planner: a refused step changes nothing ----
  const int rem = (int)((v->total - 1) % 8), pad_f = v->eof && rem ? 8 - rem : 0;     // dove_plan_padding, once the end is known
  const long long known = v->total + pad_f;                     // the padded length once the end is known (the tail repeats the last frame)
  dove_chunk_planner pl = v->planner;
  long long t0 = 0, t1 = 0;
  int last = 0;
  const int got = planner_next(&pl, known, v->eof, &t0, &t1, &last);
  if (got < 0) return got;
  if (got == 0) {
    DOVE_CHECK_ARG(v->chunks > 0, "%s", MSG_LACK);              // no chunk at all: the in-memory coverage check's text
    v->planner = pl; v->done = true;
    if (done) *done = 1;
    return DOVE_OK;
  }
  const int f = (int)(t1 - t0);
  DOVE_CHECK_ARG(f >= 1 && f <= L.fmax, "dove_video_step: a chunk of %d frames (the session was opened for at most %d)", f, L.fmax);
  DOVE_CHECK_ARG(t0 >= v->base, "dove_video_step: internal: frame %lld was dropped", t0);
  const bool tiled = !(p.tile_h == 0 && p.tile_w == 0);
  const int ov[3] = {p.chunk_len > 0 ? p.overlap_t : 0, tiled ? p.overlap_h : 0, tiled ? p.overlap_w : 0};
  // "is the first / the last chunk" is all the valid region asks of the clip (get_valid_tile_region tests t0 == 0 and t1 == F only): in
  // chunk-local frames the chunk is [lo, lo + f) of a clip that ends with it or later
  const int lo = t0 == 0 ? 0 : 1, full[3] = {lo + f + (last ? 0 : 1), L.Hs, L.Ws};
  std::vector<int> valid(6 * L.ntiles), outb(6 * L.ntiles);
  for (int i = 0; i < L.ntiles; ++i) {
    const Tile& t = L.tiles[i];
    const int piece[6] = {lo, lo + f, t.h0, t.h1, t.w0, t.w1};
    valid_region(piece, full, ov, &valid[6 * i], &outb[6 * i]);
    outb[6 * i] -= lo; outb[6 * i + 1] -= lo;                    // frames of this chunk
  }
  const int a = valid[0], b_all = valid[1];                      // the same for every tile of the chunk
  {
    std::vector<int> boxes(outb);
    for (int i = 0; i < L.ntiles; ++i) { boxes[6 * i] -= a; boxes[6 * i + 1] -= a; }
    VCHK(check_coverage(boxes.data(), L.ntiles, b_all - a, L.Hs, L.Ws));
  }
  // the seam between chunks: this chunk's kept frames must begin where the previous chunk's ended (an odd overlap_t floors ov / 2 on both
  // sides, so two chunks keep the same frame: the whole-clip count of the reference then reads 2)
  DOVE_CHECK_ARG(t0 + a <= v->written_end, "%s", MSG_LACK);
  DOVE_CHECK_ARG(t0 + a >= v->written_end, "%s", MSG_DOUBLE);
  int b = b_all;
  if (v->eof) b = (int)std::min<long long>(b, v->total - t0);   // minus the padded tail
  const int k = std::max(0, b - a);
  DOVE_CHECK_ARG(k == 0 || (out && out_bytes >= (size_t)k * L.out_fb), "dove_video_step: this step writes %d frames of %zu bytes, the output buffer holds "
                 "%zu bytes", k, L.out_fb, out_bytes);
  const int tc = cf->vae_temporal_compression, T = 1 + (f - 1) / tc;
  const int Td = T + T % cf->dit_patch_t;                       // the first-frame pad of dove_sr_clip (csrc/graph.hip: ncopy = T % patch_t, ref :418-421)
  std::vector<dove_dit_aux> auxes(L.ntiles, dove_dit_aux{nullptr, nullptr, nullptr});
  for (int i = 0; p.aux_fn && i < L.ntiles; ++i) {
    const int h8 = (L.tiles[i].h1 - L.tiles[i].h0) / 8, w8 = (L.tiles[i].w1 - L.tiles[i].w0) / 8;
    DOVE_CHECK_ARG(p.aux_fn(p.aux_user, Td, h8, w8, &auxes[i]) == 0, "dove_video_step: aux_fn failed for a %d x %d x %d latent grid", Td, h8, w8);
  }
  v->planner = pl;                                              // nothing above changed the session; from here on a failure (a launch) ends it
  v->written_end = t0 + b_all;
  // ---- the chunk ----
  hipStream_t s = (hipStream_t)stream;
  VHIPCHK(hipSetDevice(dove_ctx_device(v->ctx)));
  char* m = v->mem;
  for (int i = 0; i < f;) {                                     // the chunk's input frames, the padding repeats the last frame
    const long long t = std::min(t0 + i, v->total - 1);
    const int slot = (int)(t % L.ring_frames);
    int run = 1;
    while (i + run < f && t0 + i + run < v->total && slot + run < L.ring_frames) ++run;
    VHIPCHK(hipMemcpyAsync(m + L.stage + (size_t)i * L.in_fb, m + L.ring + (size_t)slot * L.in_fb, (size_t)run * L.in_fb, hipMemcpyDeviceToDevice, s));
    i += run;
  }
  if (p.in_format == DOVE_VIDEO_YUV) VCHK(dove_yuv_to_rgb_u8(m + L.stage, f, p.height, p.width, &p.in_yuv, m + L.rgb, stream));
  bf16_t* video = (bf16_t*)(m + L.video);
  bf16_t* outc = (bf16_t*)(m + L.out);
  VCHK(dove_preprocess_u8(m + L.rgb, f, p.height, p.width, 0, L.pad_h, L.pad_w, p.upscale, video, DOVE_BF16, stream));
  const BoxSide vs{(long long)f * L.Hs * L.Ws, (long long)L.Hs * L.Ws, L.Ws};
  for (int i = 0; i < L.ntiles; ++i) {
    const Tile& t = L.tiles[i];
    const int th = t.h1 - t.h0, tw = t.w1 - t.w0;
    const bf16_t* tin = video;
    if (!L.whole) {
      const BoxSide ts{(long long)f * th * tw, (long long)th * tw, tw};
      VCHK(box_copy(video + (long long)t.h0 * L.Ws + t.w0, vs, (bf16_t*)(m + L.tile_in), ts, f, th, tw, s, "dove_video_step (tile)"));
      tin = (const bf16_t*)(m + L.tile_in);
    }
    const long long lat = (long long)cf->vae_latent_channels * (th / 8) * (tw / 8);
    const unsigned long long ord = (unsigned long long)v->pieces;
    VCHK(dove_randn(m + L.noise, DOVE_F32, lat * T, p.seed, 2 * ord, 0, stream));
    dove_pre_noise pre{nullptr, DOVE_F32, 0.f, 0.f};
    if (p.noise_step) {
      VCHK(dove_randn(m + L.eps, DOVE_F32, lat * Td, p.seed, 2 * ord + 1, 0, stream));
      pre.eps = m + L.eps; pre.eps_dtype = DOVE_F32; pre.sqrt_alpha = p.noise_sqrt_alpha; pre.sqrt_one_minus_alpha = p.noise_sqrt_one_minus_alpha;
    }
    VCHK(dove_sr_clip(v->ctx, tin, DOVE_BF16, f, th, tw, m + L.noise, DOVE_F32, p.text, p.text_len, p.timestep, p.sqrt_alpha, p.sqrt_one_minus_alpha,
                      p.aux_fn ? &auxes[i] : nullptr, p.noise_step ? &pre : nullptr, m + L.piece, DOVE_BF16, stream));
    VCHK(dove_stitch(m + L.piece, f, th, tw, &valid[6 * i], outc, f, L.Hs, L.Ws, outb[6 * i], outb[6 * i + 2], outb[6 * i + 4], stream));
    ++v->pieces;
  }
  if (k > 0) {
    const long long plane = (long long)L.Hs * L.Ws;
    dove_image_view content{outc + a * plane, DOVE_BF16, 0, plane, (long long)f * plane, L.Ws, 1};
    if (p.color_fix) {
      const dove_image_view style{video + a * plane, DOVE_BF16, 0, plane, (long long)f * plane, L.Ws, 1};
      void* fixed = p.out_format == DOVE_VIDEO_YUV ? (void*)(m + L.fixed) : out;
      const dove_image_view fv{fixed, DOVE_U8, 0, (long long)L.Ho * L.Wo * 3, 1, (long long)L.Wo * 3, 3};
      VCHK(dove_color_fix(&content, 1.f, 0.f, &style, 0.5f, 0.5f, k, L.Ho, L.Wo, p.color_fix, DOVE_COLORFIX_CLAMP, &fv, m + L.cf_ws, L.cf_ws_bytes, stream));
      if (p.out_format == DOVE_VIDEO_YUV) VCHK(dove_rgb_to_yuv_u8(&fv, k, L.Ho, L.Wo, &p.out_yuv, out, stream));
    } else if (p.out_format == DOVE_VIDEO_YUV) {
      VCHK(dove_rgb_to_yuv_u8(&content, k, L.Ho, L.Wo, &p.out_yuv, out, stream));
    } else {
      VCHK(dove_postprocess_u8(outc + a * plane, DOVE_BF16, f, L.Hs, L.Ws, k, L.Ho, L.Wo, out, stream));
    }
  }
  ++v->chunks;
  v->done = last != 0;
  v->base = std::max(v->base, std::min(v->planner.start, v->total));   // frames before the next chunk's start are done with
  *frames_written = k;
  if (done) *done = v->done ? 1 : 0;
  return DOVE_OK;
}
