// The library's counter-based generator, shared by dove_randn (video.hip) and the noise operators (degrade.hip): Philox4x32-10 and the
// Box-Muller pair.  tests/randn_ref.py is the definition; include/dove_hip.h has it in words.
#pragma once
#include "common.h"

struct Words { uint32_t x[4]; };
__host__ __device__ inline Words philox4x32_10(uint64_t block, uint64_t stream_id, uint64_t seed) {
  uint32_t c0 = (uint32_t)block, c1 = (uint32_t)(block >> 32), c2 = (uint32_t)stream_id, c3 = (uint32_t)(stream_id >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Words{{c0, c1, c2, c3}};
}

// one Box-Muller pair.  -ln u1 for u1 = (x + 1) 2^-32: above 1/2 the complement 1 - u1 = (2^32 - 1 - x) 2^-32 is formed exactly from the
// integer and goes through log1p, so the radius near zero does not lose its leading bits to the rounding of u1 towards 1.
__device__ inline void box_muller(uint32_t xa, uint32_t xb, float* z0, float* z1) {
  const float two_m32 = 2.3283064365386963e-10f;
  float neg_ln;
  if (xa >= 0x80000000u) neg_ln = -log1pf(-((float)(~xa) * two_m32));
  else neg_ln = -logf(((float)xa + 1.0f) * two_m32);
  const float r = sqrtf(2.0f * neg_ln);
  float s, c;
  sincospif(2.0f * ((float)xb * two_m32), &s, &c);
  *z0 = r * c;
  *z1 = r * s;
}
