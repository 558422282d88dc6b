// Online (max, sum) logsumexp pieces shared by softmax_xent.hip and eval_metrics.hip: the per-value updates, the
// wave butterfly and the 4-wave block combine.  Everything in fp32 with the fast exp / log.
#pragma once
#include "dtg/common.h"

namespace dtg {

template <typename T>
__device__ __forceinline__ float ld(const T* p, long long i);
template <>
__device__ __forceinline__ float ld<float>(const float* p, long long i) { return p[i]; }
template <>
__device__ __forceinline__ float ld<bf16_t>(const bf16_t* p, long long i) { return bf2f(p[i]); }

// online (max, sum) update with one value / with 8 values
__device__ __forceinline__ void ms_add(float& m, float& s, float v) {
  if (v == -INFINITY) return;  // masked out (with m still -inf, exp(v - m) would be NaN)
  if (v > m) {
    s = s * __expf(m - v) + 1.f;
    m = v;
  } else {
    s += __expf(v - m);
  }
}
__device__ __forceinline__ void ms_add8(float& m, float& s, const float (&v)[8]) {
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) mx = fmaxf(mx, v[k]);
  if (mx == -INFINITY) return;  // all eight masked out
  if (mx > m) {
    s = (m == -INFINITY ? 0.f : s * __expf(m - mx));
    m = mx;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) s += __expf(v[k] - m);
}

// combine the (m, s) pairs of a wave's 64 lanes; every lane ends with the wave's pair
__device__ __forceinline__ void wave_ms(float& m, float& s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float mo = __shfl_xor(m, o, 64), so = __shfl_xor(s, o, 64);
    const float mn = fmaxf(m, mo);
    s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (mo == -INFINITY ? 0.f : so * __expf(mo - mn));
    m = mn;
  }
}

// block-wide logsumexp of the per-thread (m, s) pairs (256 threads = 4 waves)
__device__ __forceinline__ float block_lse(float m, float s, float (*red)[4]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  wave_ms(m, s);
  if (lane == 0) {
    red[0][wid] = m;
    red[1][wid] = s;
  }
  __syncthreads();
  float M = red[0][0];
#pragma unroll
  for (int w = 1; w < 4; ++w) M = fmaxf(M, red[0][w]);
  float S = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) S += red[1][w] * __expf(red[0][w] - M);
  return M + __logf(S);
}

}  // namespace dtg
