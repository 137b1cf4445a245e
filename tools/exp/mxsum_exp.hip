// EXPERIMENT: how v_mfma_scale_f32_32x32x64_f8f6f4 sums its 64 scaled products (one wave, one instruction, C input); operand layout as
// csrc/mxfp8.hip uses it (layout 1 of mxprobe_exp.hip).  Driver: tools/archive/mxsum.py; findings: docs/kernels.md section 4.2.
#include <hip/hip_runtime.h>
#include <stdint.h>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
__global__ void probe(const unsigned char* A, const unsigned char* B, const unsigned* sa, const unsigned* sb, const float* Cin, float* C) {
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
  v8i a, b;
  for (int j = 0; j < 8; ++j) {
    const int k = (j >> 2) * 32 + hi * 16 + (j & 3) * 4;
    a[j] = *(const int*)(A + l31 * 64 + k);
    b[j] = *(const int*)(B + l31 * 64 + k);
  }
  f32x16 c;
  for (int r = 0; r < 16; ++r) c[r] = Cin[((r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + l31];
  c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, sa[l31 * 2 + hi], 0, sb[l31 * 2 + hi]);
  for (int r = 0; r < 16; ++r) C[((r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + l31] = c[r];
}
extern "C" int mxsum(const void* A, const void* B, const void* sa, const void* sb, const void* Cin, void* C, void* stream) {
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, (hipStream_t)stream, (const unsigned char*)A, (const unsigned char*)B, (const unsigned*)sa,
                     (const unsigned*)sb, (const float*)Cin, (float*)C);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
