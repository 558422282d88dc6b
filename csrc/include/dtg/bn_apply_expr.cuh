// The elementwise expressions of the forward BN apply passes, 8 channels at a time, and their packed relu mask.
// batchnorm.hip's streaming kernels and the apply pass that also feeds the next block's conv1 (bn_dx_wgrad.hip:
// bn_apply_gemm_kernel) evaluate these very functions, so their outputs and mask bits agree bit for bit.
#pragma once
#include "dtg/common.h"

namespace dtg {

// a = [relu]( a * sc + sf [+ r] )
template <bool RES, bool RELU>
__device__ __forceinline__ void bn_apply8(float (&a)[8], const float (&r)[8], const float (&sc)[8],
                                          const float (&sf)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float v = a[k] * sc[k] + sf[k];
    if constexpr (RES) v += r[k];
    if constexpr (RELU) v = fmaxf(v, 0.f);
    a[k] = v;
  }
}

// a = relu( a * sc + b * sc2 + sf ), sf the sum of both BNs' shifts (projection blocks)
__device__ __forceinline__ void bn_apply2_8(float (&a)[8], const float (&b)[8], const float (&sc)[8],
                                            const float (&sc2)[8], const float (&sf)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = fmaxf(fmaf(a[k], sc[k], fmaf(b[k], sc2[k], sf[k])), 0.f);
}

__device__ __forceinline__ uint8_t pos_bits8(const float (&v)[8]) {
  uint32_t b = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) b |= (v[k] > 0.f ? 1u : 0u) << k;
  return (uint8_t)b;
}

// packed relu-mask byte of this lane's 8 channels -> bits[off >> 3].  The 4 lanes tx = 4i .. 4i+3 of a row
// hold 4 consecutive bytes: with C % 32 == 0 they are gathered by two lane shuffles into one 4-byte store by
// the first of them (a byte store per lane measured ~1/5 of the apply pass's bandwidth lost)
__device__ __forceinline__ void store_bits(uint8_t* bits, long long off, const float (&v)[8], int tx, int C) {
  const uint32_t b = pos_bits8(v);
  if ((C & 31) == 0) {
    uint32_t w = b << (8 * (tx & 3));
    w |= __shfl_xor(w, 1, 64);
    w |= __shfl_xor(w, 2, 64);
    if ((tx & 3) == 0) *reinterpret_cast<uint32_t*>(bits + (off >> 3)) = w;
  } else {
    bits[off >> 3] = (uint8_t)b;
  }
}

}  // namespace dtg
