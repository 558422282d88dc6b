// What the decode kernels of attention_decode.hip (bf16 cache) and attention_decode_fp8.hip (e4m3 cache) share: the
// split geometry, the partial layout and the merge of a workgroup's 4 waves.  The split choice itself
// (attn_decode_splits / attn_decode_force_splits) and the combine launch (attn_decode_combine) are host functions of
// attention_decode.hip, declared in kernels.h.
#pragma once
#include "dtg/common.h"

namespace dtg {
namespace adec {

constexpr int kNW = 4;           // waves per workgroup
constexpr int kPart = 66;        // floats of a partial: m, l, acc[64]
constexpr int kMaxSplits = 1024;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// chunks a record can span: the window's positions len + 1 - window .. len start anywhere in a chunk
inline int max_chunks(int max_len, int window) {
  const int all = max_len / 64 + 1;
  if (window <= 0) return all;
  const long long w = ((long long)window + 62) / 64 + 1;
  return w < all ? (int)w : all;
}

// After the 4 waves left their (m, l, acc[64]) in red and the workgroup met at a barrier: thread tid < 64 merges dim
// tid.  nsplit = 1: ctx (bf16) and lse; nsplit > 1: the fp32 partial of split sp.
__device__ __forceinline__ void merge_waves(const float (&red)[kNW][kPart + 2], int tid, int b, int h, int bh, int H,
                                            int sp, int nsplit, float* __restrict__ ws, bf16_t* __restrict__ ctx,
                                            float* __restrict__ lse) {
  float M = red[0][0];
#pragma unroll
  for (int w = 1; w < kNW; ++w) M = fmaxf(M, red[w][0]);
  float L = 0.f, a = 0.f;
  if (M != -INFINITY) {
#pragma unroll
    for (int w = 0; w < kNW; ++w) {
      const float f = __builtin_amdgcn_exp2f(red[w][0] - M);  // an idle wave: exp2(-inf) = 0
      L = fmaf(f, red[w][1], L);
      a = fmaf(f, red[w][2 + tid], a);
    }
  }
  if (nsplit == 1) {
    // L = 0 only for a refused record: zeros
    ctx[(long long)b * H + h * 64 + tid] = f2bf(L > 0.f ? a / L : 0.f);
    if (tid == 0) lse[bh] = L > 0.f ? fmaf(M, kLn2, __logf(L)) : 0.f;
  } else {
    float* part = ws + ((long long)bh * nsplit + sp) * kPart;
    if (tid == 0) {
      part[0] = M;
      part[1] = L;
    }
    part[2 + tid] = a;
  }
}

}  // namespace adec
}  // namespace dtg
