// Flash-attention forward for the CogVideoX DiT joint [text ; video] self-attention (gfx950): the entry point dove_attention_fwd_bf16 and the
// RUNNING-MAXIMUM kernel.  Heads the caller hands a finite score bound for (norm2) run on the software-pipelined no-shift kernel of
// attention_pipe.hip first (round 5: bound <= 40; round 6: every finite bound, the row sums checked in that kernel's epilogue); this kernel
// keeps the heads that one marked NaN, the heads whose bound was not finite - and every head when no bound is given - and exits at once for a
// head the other kernel finished.  Its own constant-shift loop (below) runs only for a caller that gives a bound and skip_bounded == 0,
// which this library's entry point never does (rounds 3-4 ran the bounded heads on it).
//   head_dim 64, bf16 MFMA 32x32x16, fp32 online softmax, non-causal, no mask, N not a tile multiple.
// Replaces F.scaled_dot_product_attention inside diffusers' CogVideoXAttnProcessor2_0, reached from
// /root/reference/inference_script.py:483-489.
//
// Operands come head-major from dove_qkv_post_bf16: Q' [H][Npad][64] (already multiplied by
// scale*log2e), K' [H][Npad][64], V^T [H][64][Npad]; pad rows/columns are zero.
// Workgroup = 4 waves = 128 query rows (32 per wave); KV tiles of 64 keys are staged K and V^T alike with
// 16-byte buffer_load ... lds into XOR-swizzled LDS (per-thread constant offsets, the tile index rides in
// soffset).  Four 16 KB stages = two PAIRS of tiles: ONE workgroup barrier per two tiles (128 keys), the next pair in
// flight while the current one is multiplied; every ds_read address is a per-lane constant + immediate.
// Swapped products keep the softmax lane-local (guide T12): S^T = K Q^T puts one query column in each
// lane (row max/sum = in-lane + one half exchange by v_permlane32_swap), P^T is packed with v_cvt_pk_bf16_f32 and
// re-laid to the MFMA B layout with v_permlane32_swap, and O^T = V^T P^T accumulates with the same query-per-lane
// ownership.
// Softmax shift without VALU work: the running max m enters the S accumulator through the MFMA's C operand (16 registers
// holding -m; the first MFMA of each S chain is issued with C != D, which the builtin cannot express), so the MFMA
// result is already S - m.  m is updated lazily (guide T13): only on a query block's first tile and when some score
// exceeds it by THR = 2^6; then O, l, the current tile's S and the -m registers are rescaled once, BEFORE the tile's
// P is exponentiated (the safe order of T13).  P <= 64 in bf16 keeps its 8-bit relative precision and O / l accumulate
// in fp32, so the result matches the exact-max formulation to rounding (tests: spiked keys early / late, full tensor).
// Measured on MI355X at N = 18226, 48 heads (tools/archive/attn_ab.py, within-run A/B; profiles/r02_attn_ab.log, r03_*): 0.93-0.99 PF by box
// (round 1: 0.88-0.91).  What did NOT pay (same harness): row sum on the matrix pipe (ones x P^T, -2 %), four partial sums / v_pk_add
// (0 %), the shift as a fifth K slice (+1 % but 2x the rounding error), two query blocks per wave, in-wave software pipelining (+3 %),
// 6 / 8 waves per workgroup, and - round 3 - two wave groups one barrier phase apart (tools/exp/attn2g_exp.hip: 0.94-0.98x).
// tools/archive/coissue.py shows what bounds all of them: on gfx950 the MFMAs of one wave and the VALU of ANOTHER wave on the same SIMD
// serialize completely (t = t_mfma + t_valu at any priority); only VALU instructions that follow an MFMA in the same wave's own
// stream hide under it (about half of the softmax mix).  Per 32 x 64 wave-tile: 16 MFMAs = 290 ns on N(0,1)-like operands
// (the pipes throttle with operand toggling: 1.9 PF sustained, tools/archive/mfma_storm.py), softmax VALU = 311-353 ns, measured 540 ns.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "../../include/dove_hip.h"

typedef __attribute__((address_space(3))) void* lds_ptr_t;

__attribute__((visibility("hidden"))) int dove_attention_pipe_launch(const void* Qh, const void* Kh, const void* Vt, void* O, long long N, long long Npad,
                                                                    int heads, long long ldo, float* norm2, void* stream);   // attention_pipe.hip

__device__ __forceinline__ bf16x8 make_frag(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  u32x4 v = {a, b, c, d};
  return __builtin_bit_cast(bf16x8, v);
}

// D = A B + C with the accumulator INPUT in other registers than the output (C = -m broadcast, D = S - m).  The builtin
// ties C to D and the compiler would copy the 16 registers first.  `s_nop 1`: a VALU write of C (rare rescale path) needs
// two wait states before an MFMA reads it and hipcc pads nothing inside an asm statement (guide 5.7 item 2).
__device__ __forceinline__ f32x16 mfma_c_in(bf16x8 a, bf16x8 b, const f32x16& c) {
  f32x16 d;
  asm("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// NW = waves per workgroup: NW x 32 queries share every K / V^T tile (waves 0-3 stage them).  The library instantiates <4, true, false> only:
// 8 waves sharing a tile measured within noise of 4 (0 / +1.7 % on two boxes), 6 waves -13 %; the 2-D grid (XCD = false) and FIXED (a
// compile-time constant shift) were experiments.  The entry point that launched those variants left with the timing library (git history).
// XCD: 1-D grid of heads x query-blocks, remapped so that each XCD (= blockIdx % 8, its own L2) walks a CONTIGUOUS range of the
// head-major tile list: the ~64 workgroups an XCD runs at a time then belong to one or two heads and stream the same K / V^T tiles
// through one L2, instead of every XCD streaming every head (the 2-D grid puts consecutive query blocks of a head on 8 XCDs).
// The eight K / V^T LDS-DMA loads of a tile pair are issued as one burst behind the barrier.  Spreading them two at a time between the four
// MFMA groups of the pair's first tile (fenced like gemm4x's groups, where that is worth +5-8 %) changes nothing here: 4.263 / 4.267 / 4.260 ms
// (profiles/r03_attn_dma.log) - the second workgroup of the CU computes through the first one's burst.
template <int NW, bool XCD = true, bool FIXED = false>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_kernel(const bf16_t* __restrict__ Qh, const bf16_t* __restrict__ Kh,
                                                          const bf16_t* __restrict__ Vt, bf16_t* __restrict__ O,
                                                          long long N, long long Npad, long long ldo, int qblocks,
                                                          const float* __restrict__ bound = nullptr, int skip_bounded = 0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int STAGE = 16384, VOFF = 8192;
  constexpr float THR = 6.0f;                    // rescale when a score exceeds the running max by 2^6
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  int h, qb;
  if (XCD) {
    const unsigned t = xcd_remap(blockIdx.x, gridDim.x);
    h = (int)(t / (unsigned)qblocks);
    qb = (int)(t - (unsigned)h * (unsigned)qblocks);
  } else {
    h = blockIdx.y;
    qb = blockIdx.x;
  }
  const long long q0 = (long long)qb * (NW * 32) + wave * 32;
  const bool live = q0 + l31 < N;                // rows of the padded tail are never stored - and never vote for a rescale (compute)
  // skip_bounded: attn_pipe_kernel (attention_pipe.hip) ran first on every head with a finite bound and marked the ones it could not finish
  // NaN; this kernel keeps the marked ones and those whose bound was NaN / infinite to begin with.  (Before any load: ~6.9 k workgroups of a
  // DiT attention call leave here.)
  if (bound && skip_bounded && bound[2 * h] * bound[2 * h + 1] < __builtin_inff()) return;

  bf16x8 qf[4];
  {
    long long qrow = q0 + l31;
    if (qrow >= Npad) qrow = Npad - 1;           // rows past the padded end are never stored; keep the load in range
    const bf16_t* qp = Qh + ((long long)h * Npad + qrow) * 64 + hi * 8;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const bf16x8*)(qp + kk * 16);
  }

  f32x16 o[2], negm;
  float m = 0.f, lsum = 0.f;                     // m becomes a real maximum on the first tile
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; negm[r] = 0.f; }
  // FIXED (compile time, experiment) / fixed (run time): the caller bounds every score of this head (|q . k| <= max |q| max |k|, squared
  // norms from dove_qkv_post_bf16): a constant shift rides in the C operand and the loop needs no running maximum at all - the constant
  // cancels in O / l.  Bounds above 40 fall back to the running maximum: a row whose every key is anti-aligned has all its probabilities near
  // 2^-2b, and 2^-80 keeps P, l and the P V products far inside the NORMAL fp32 / bf16 range (60, the first cutoff, left 2^-120 - six binades
  // above the denormals, less than |v| can take away; LayerNorm'd q / k give b ~ 12).
  bool fixed = FIXED;
  if (bound && !skip_bounded) {       // (never taken from dove_attention_fwd_bf16: the constant-shift loop of rounds 3-4)
    const float b = FIXED ? bound[h] : 1.01f * sqrtf(bound[2 * h] * bound[2 * h + 1]);   // [head][q, k]: max squared row norms
    fixed = FIXED || b <= 40.0f;      // NaN compares false: the running maximum
    if (fixed) {
#pragma unroll
      for (int r = 0; r < 16; ++r) negm[r] = -b;
    }
  }
  fixed = __builtin_amdgcn_readfirstlane(fixed);

  const int ntiles = (int)((N + 63) / 64);
  const int srow = tid >> 3;
  const int sc_ld = (tid & 7) ^ ((srow >> 1) & 7);
  const auto srd_k = __builtin_amdgcn_make_buffer_rsrc((void*)(Kh + (long long)h * Npad * 64), (short)0, (int)(Npad * 128), 0x00020000);
  const auto srd_v = __builtin_amdgcn_make_buffer_rsrc((void*)(Vt + (long long)h * 64 * Npad), (short)0, (int)(Npad * 128), 0x00020000);
  unsigned vk[2], vv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    vk[j] = (unsigned)(((j * 32 + srow) * 64 + sc_ld * 8) * 2);
    vv[j] = (unsigned)((((long long)(j * 32 + srow)) * Npad + sc_ld * 8) * 2);
  }
  auto stage = [&](auto bufc, int tile) {
    constexpr int BUF = decltype(bufc)::value;
    if (NW > 4 && wave >= 4) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_k, (lds_ptr_t)(smem + BUF * STAGE + (j * 256 + wave * 64) * 16), 16, vk[j],
                                               tile * (64 * 128), 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_v, (lds_ptr_t)(smem + BUF * STAGE + VOFF + (j * 256 + wave * 64) * 16), 16, vv[j],
                                               tile * (64 * 2), 0, 0);
    }
  };

  // per-lane constant fragment offsets; the V^T tile uses the same (row, chunk) pattern, so its reads are koff + VOFF (immediate)
  int koff[2][4];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int row = b * 32 + l31;
    const int sw = (row >> 1) & 7;
#pragma unroll
    for (int c = 0; c < 4; ++c) koff[b][c] = row * 128 + (((c * 2 + hi) ^ sw) << 4);
  }

  auto compute = [&](auto bufc, int tile, auto fixc) {
    constexpr int BUF = decltype(bufc)::value;
    constexpr bool kFixed = decltype(fixc)::value;   // no running maximum: the constant shift is already in negm
    // ---- (S - m)^T[kv][q] = K Q^T - m : the shift rides in the C operand of the first MFMA of each chain ----
    f32x16 st[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const bf16x8 kf = *(const bf16x8*)(smem + BUF * STAGE + koff[kb][kk]);
        if (kk == 0) st[kb] = mfma_c_in(kf, qf[kk], negm);
        else st[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], st[kb], 0, 0, 0);
      }
    const long long kv0 = (long long)tile * 64;
    if (kv0 + 64 > N) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const long long kv = kv0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (kv >= N) st[kb][r] = -1e30f;
        }
    }
    // ---- lazy online softmax (base 2; Q carries scale*log2e) ----
    if (!kFixed) {
    float mt = st[0][0];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mt = fmaxf(mt, st[kb][r]);
    {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mt), __float_as_uint(mt), false, false);
      mt = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));        // the other half of the same query column
    }
    const bool first = tile == 0;
    // (only rows that exist vote: the vote moves m, and with it the rounding, of every row of the wave whose tile maximum is positive - the
    // contents of the Q rows [N, Npad) must not reach the stored rows that way.  A pad row's own m may then lag: its lane may overflow, alone.)
    if (first || __any(live && mt > THR)) {      // wave-uniform and rare after the first tiles
      // everything still expressed against the old max is rescaled exactly once, before this tile's P exists
      const float delta = first ? mt : fmaxf(mt, 0.f);
      const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-delta);   // first tile: O = l = 0, and 2^(-mt) may overflow
      m += delta;
      lsum *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o[0][r] *= alpha; o[1][r] *= alpha; st[0][r] -= delta; st[1][r] -= delta; negm[r] = -m;
      }
    }
    }
    float ps = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(st[kb][r]);
        st[kb][r] = p;
        ps += p;
      }
    lsum += ps;
    bf16x8 pf[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        const int b = 8 * k2;
        const uint32_t a0 = pack_bf2(st[kb][b + 0], st[kb][b + 1]);
        const uint32_t a1 = pack_bf2(st[kb][b + 2], st[kb][b + 3]);
        const uint32_t b0 = pack_bf2(st[kb][b + 4], st[kb][b + 5]);
        const uint32_t b1 = pack_bf2(st[kb][b + 6], st[kb][b + 7]);
        // The QK^T MFMA leaves lane half hi with keys {0-3, 8-11} + 4 hi of these 16; the PV contraction runs over the keys, so
        // their order is free as long as V^T uses the same one: dove_qkv_post_bf16 (v_order 1) stores every 16 keys as
        // [0-3, 8-11, 4-7, 12-15] and the lane's own eight probabilities ARE its half of the B operand - no exchange between the
        // lane halves (was: 2 v_permlane32_swap per fragment, 72 issue cycles per tile).
        pf[kb][k2] = make_frag(a0, a1, b0, b1);
      }
    // ---- O^T[d][q] += V^T P^T ----
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const bf16x8 vf = *(const bf16x8*)(smem + BUF * STAGE + VOFF + koff[db][kb * 2 + k2]);
          o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[kb][k2], o[db], 0, 0, 0);
        }
  };

  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;
  using B2 = std::integral_constant<int, 2>;
  using B3 = std::integral_constant<int, 3>;
  stage(B0{}, 0);
  if (1 < ntiles) stage(B1{}, 1);
  // the tile loop exists twice - with and without the running maximum - so that neither copy carries the other's branch
#define DOVE_ATTN_LOOP(FX)                                                  \
  for (int it = 0; it < ntiles; it += 4) {                                  \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                        \
    __syncthreads();                                                        \
    if (it + 2 < ntiles) stage(B2{}, it + 2);                               \
    if (it + 3 < ntiles) stage(B3{}, it + 3);                               \
    compute(B0{}, it, FX{});                                                \
    if (it + 1 < ntiles) compute(B1{}, it + 1, FX{});                       \
    if (it + 2 >= ntiles) break;                                            \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                        \
    __syncthreads();                                                        \
    if (it + 4 < ntiles) stage(B0{}, it + 4);                               \
    if (it + 5 < ntiles) stage(B1{}, it + 5);                               \
    compute(B2{}, it + 2, FX{});                                            \
    if (it + 3 < ntiles) compute(B3{}, it + 3, FX{});                       \
  }
  if (fixed) { DOVE_ATTN_LOOP(std::true_type) } else { DOVE_ATTN_LOOP(std::false_type) }
#undef DOVE_ATTN_LOOP

  const float l = lsum + __shfl_xor(lsum, 32);
  const float inv = 1.0f / l;
  const long long q = q0 + l31;
  if (q < N) {
    bf16_t* op = O + q * ldo + h * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * hi;
        uint2 w;
        w.x = pack_bf2(o[db][g * 4 + 0] * inv, o[db][g * 4 + 1] * inv);
        w.y = pack_bf2(o[db][g * 4 + 2] * inv, o[db][g * 4 + 3] * inv);
        *(uint2*)(op + d) = w;
      }
  }
}

extern "C" int dove_attention_fwd_bf16(const void* Qh, const void* Kh, const void* Vt, void* O, long long N,
                                        long long Npad, int heads, int head_dim, long long ldo, float* norm2, void* stream) {
  DOVE_CHECK_ARG(Qh && Kh && Vt && O, "attention_fwd: null pointer");
  DOVE_CHECK_ARG(head_dim == 64, "attention_fwd: head_dim must be 64 (got %d)", head_dim);
  DOVE_CHECK_ARG(N > 0 && Npad % 128 == 0 && Npad >= N && Npad - N < 128, "attention_fwd: Npad must be N rounded up to 128");
  DOVE_CHECK_ARG(Npad * 128 < (1ll << 31), "attention_fwd: sequence too long for 31-bit buffer offsets");
  DOVE_CHECK_ARG(ldo >= (long long)heads * 64 && ldo % 4 == 0, "attention_fwd: bad ldo");
  constexpr int LDS = 4 * 16384;
  constexpr int NW = 4;
  static PerDeviceOnce attr_set;
  if (auto once_ = attr_set.guard()) {
    (void)hipFuncSetAttribute((const void*)(attn_fwd_kernel<NW, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  }
  const int qblocks = (int)((Npad + NW * 32 - 1) / (NW * 32));
  DOVE_CHECK_ARG((long long)qblocks * heads < (1ll << 31), "attention_fwd: grid too large");
  // With a score bound per head (norm2) every head whose bound is finite runs on the software-pipelined kernel (attention_pipe.hip: one wave
  // per SIMD, no shift), which marks norm2[2 h] NaN for a head whose row sums left its safe window; those, the heads with a non-finite bound -
  // and every head when no bound is given - run here on the running maximum, AFTER the other kernel on the same stream: the final contents of
  // every output row come from exactly one of them, and norm2 says which (dove_attention_head_paths).
  const int skip_bounded = norm2 ? 1 : 0;
  if (norm2) {
    const int rc = dove_attention_pipe_launch(Qh, Kh, Vt, O, N, Npad, heads, ldo, norm2, stream);
    if (rc) return rc;
  }
  hipLaunchKernelGGL((attn_fwd_kernel<NW, true>), dim3((unsigned)(qblocks * heads)), dim3(NW * 64), LDS, (hipStream_t)stream, (const bf16_t*)Qh,
                     (const bf16_t*)Kh, (const bf16_t*)Vt, (bf16_t*)O, N, Npad, ldo, qblocks, norm2, skip_bounded);
  DOVE_CHECK_LAUNCH("dove_attention_fwd_bf16");
  return DOVE_OK;
}

extern "C" int dove_attention_head_paths(const float* norm2_host, int heads, int* path) {
  DOVE_CHECK_ARG(path && heads >= 0, "attention_head_paths: bad arguments");
  for (int h = 0; h < heads; ++h) path[h] = norm2_host && norm2_host[2 * h] * norm2_host[2 * h + 1] < __builtin_inff() ? 1 : 0;   // the kernels' own test
  return DOVE_OK;
}
extern "C" const char* dove_attention_path_name(int path) { return path == 1 ? "attn_pipe_kernel" : path == 0 ? "attn_fwd_kernel" : ""; }
