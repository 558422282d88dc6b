// Gradient accumulation over micro-batches (parallel/accum.py): the fp32 accumulator's two streaming kernels.
//   grad_fold    acc[i] = (first ? 0 : acc[i]) + float(g[i]);  g[i] = 0       one pass, one launch per flat group
//   grad_unfold  g[i]   = cast(acc[i] + float(g[i]))                            over a range (a bucket); acc is kept
// Same form as axpby_kernel / f32_to_bf16_kernel (optim.hip): 8 elements per lane with 16-byte accesses, a grid
// capped at 2048 workgroups with a grid stride, the tail on block 0.  Operands that are not 16-byte aligned (a view
// or a range cut at an odd offset) take the scalar kernels.  With `first` the old accumulator is never read.
// NT: the accumulator is stored with a non-temporal hint.  optim.hip builds the plain-store form; the other one is
// built by the lab extension for tools/bench_accum.py (profiles/grad_accum).
#pragma once
#include "dtg/common.h"

namespace dtg {

constexpr int kFoldBlock = 256;
constexpr int kFoldGridCap = 2048;

template <bool NT>
__device__ __forceinline__ void fold_store8(float* p, const float (&o)[8]) {
  if constexpr (NT) {
    __builtin_nontemporal_store((f32x4){o[0], o[1], o[2], o[3]}, reinterpret_cast<f32x4*>(p));
    __builtin_nontemporal_store((f32x4){o[4], o[5], o[6], o[7]}, reinterpret_cast<f32x4*>(p + 4));
  } else {
    store8_f32(p, o);
  }
}

template <bool GBF16>
__device__ __forceinline__ float fold_load1(const void* g, long long i) {
  if constexpr (GBF16) return bf2f(reinterpret_cast<const bf16_t*>(g)[i]);
  else return reinterpret_cast<const float*>(g)[i];
}

template <bool GBF16>
__device__ __forceinline__ void fold_store1(void* g, long long i, float v) {
  if constexpr (GBF16) reinterpret_cast<bf16_t*>(g)[i] = f2bf(v);
  else reinterpret_cast<float*>(g)[i] = v;
}

template <bool GBF16, bool NT>
__global__ void __launch_bounds__(kFoldBlock) grad_fold_kernel(float* __restrict__ acc, void* __restrict__ g,
                                                               long long n, int first) {
  const long long nvec = n >> 3;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    const long long i = v << 3;
    float a[8], gv[8];
    if constexpr (GBF16) load8_bf16(reinterpret_cast<const bf16_t*>(g) + i, gv);
    else load8_f32(reinterpret_cast<const float*>(g) + i, gv);
    if (!first) {
      load8_f32(acc + i, a);
#pragma unroll
      for (int k = 0; k < 8; ++k) gv[k] = a[k] + gv[k];
    }
    fold_store8<NT>(acc + i, gv);
    if constexpr (GBF16) {
      *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(g) + i) = make_uint4(0u, 0u, 0u, 0u);
    } else {
      float* p = reinterpret_cast<float*>(g) + i;
      *reinterpret_cast<float4*>(p) = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(p + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  if (blockIdx.x == 0)
    for (long long i = (nvec << 3) + threadIdx.x; i < n; i += blockDim.x) {
      const float s = fold_load1<GBF16>(g, i);
      acc[i] = first ? s : acc[i] + s;
      fold_store1<GBF16>(g, i, 0.f);
    }
}

template <bool GBF16>
__global__ void __launch_bounds__(kFoldBlock) grad_fold_scalar_kernel(float* __restrict__ acc, void* __restrict__ g,
                                                                      long long n, int first) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float s = fold_load1<GBF16>(g, i);
    acc[i] = first ? s : acc[i] + s;
    fold_store1<GBF16>(g, i, 0.f);
  }
}

template <bool GBF16>
__global__ void __launch_bounds__(kFoldBlock) grad_unfold_kernel(void* __restrict__ g, const float* __restrict__ acc,
                                                                 long long n) {
  const long long nvec = n >> 3;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    const long long i = v << 3;
    float a[8], gv[8];
    load8_f32(acc + i, a);
    if constexpr (GBF16) load8_bf16(reinterpret_cast<const bf16_t*>(g) + i, gv);
    else load8_f32(reinterpret_cast<const float*>(g) + i, gv);
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = a[k] + gv[k];
    if constexpr (GBF16) store8_bf16(reinterpret_cast<bf16_t*>(g) + i, a);
    else store8_f32(reinterpret_cast<float*>(g) + i, a);
  }
  if (blockIdx.x == 0)
    for (long long i = (nvec << 3) + threadIdx.x; i < n; i += blockDim.x)
      fold_store1<GBF16>(g, i, acc[i] + fold_load1<GBF16>(g, i));
}

template <bool GBF16>
__global__ void __launch_bounds__(kFoldBlock) grad_unfold_scalar_kernel(void* __restrict__ g,
                                                                        const float* __restrict__ acc, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    fold_store1<GBF16>(g, i, acc[i] + fold_load1<GBF16>(g, i));
}

inline bool fold_aligned16(const void* a, const void* b) {
  return (((uintptr_t)a | (uintptr_t)b) & 15u) == 0;
}

// acc, g: n elements each (the caller has checked the sizes); n <= 0 launches nothing
template <bool NT>
inline void launch_grad_fold(float* acc, void* g, int g_bf16, long long n, int first, hipStream_t st) {
  if (n <= 0) return;
  if (fold_aligned16(acc, g)) {
    const int grid = grid_for((n >> 3) + 1, kFoldBlock, kFoldGridCap);
    if (g_bf16) grad_fold_kernel<true, NT><<<grid, kFoldBlock, 0, st>>>(acc, g, n, first);
    else grad_fold_kernel<false, NT><<<grid, kFoldBlock, 0, st>>>(acc, g, n, first);
  } else {
    const int grid = grid_for(n, kFoldBlock, kFoldGridCap);
    if (g_bf16) grad_fold_scalar_kernel<true><<<grid, kFoldBlock, 0, st>>>(acc, g, n, first);
    else grad_fold_scalar_kernel<false><<<grid, kFoldBlock, 0, st>>>(acc, g, n, first);
  }
  DTG_LAUNCH_CHECK();
}

}  // namespace dtg
