// Evaluation metrics over the rows of a [B, V] logit matrix (bf16 or fp32), labels int64 [B].
//
//   xent_rank          one pass per row:
//                        loss[r] = logsumexp(x[r,:]) - x[r, label]                                (fp32)
//                        rank[r] = #{j : x[r,j] > x[r,label]} + #{j < label : x[r,j] == x[r,label]}   (int32)
//                      the label's 0-based place in a descending sort, ties toward the lower column; top-k correct
//                      is rank < k.  The label's logit is read once, before the row loop; the counts ride in the
//                      same pass as the online max / sum of softmax_xent.hip (dtg/xent_online.cuh).
//                        label < 0    ignored row (the MLM convention):  loss 0, rank -1
//                        label >= V   out of range, the row is never indexed with it:  loss 0, rank -2
//                        the label's logit or the row's logsumexp is NaN:  rank V, a miss at every k
//   metric_accumulate  adds one batch of (loss, rank) into a device-resident fp64 acc[8]; one workgroup and a fixed
//                      summation order, so two runs give the same bits.  Slots: 0 rows with rank >= 0, 1 the sum of
//                      their loss, 2 rows with rank == -2, 3 rows with rank == V, 4 + i rows with 0 <= rank < ks[i].
//
// Row forms.  bf16 rows with V % 8 == 0 and 16-byte aligned rows move as 16-byte vectors, 8 logits per lane-access;
// every other row goes element-wise.  The row-to-workgroup mapping depends on V alone: up to kWaveRowMaxV columns a
// wave takes a row and a 256-thread workgroup four rows (the 1000-way ResNet head is 125 chunks: a whole workgroup
// per row would idle half its lanes), longer rows (BERT's 30528-wide decoder) take a workgroup each.  No atomics; the
// only LDS is the block form's reduction scratch.
#include "dtg/common.h"
#include "dtg/kernels.h"
#include "dtg/xent_online.cuh"

namespace dtg {

constexpr int kWaveRowMaxV = 2048;  // V <= this: one wave per row

// what a lane carries through its part of the row
struct RowAcc {
  float m = -INFINITY, s = 0.f;
  int above = 0;  // columns that sort before the label's
  int flags = 0;  // bit 0: a NaN was seen, bit 1: a +inf was seen
};

__device__ __forceinline__ void acc_one(RowAcc& a, float v, int col, float xl, int lab) {
  ms_add(a.m, a.s, v);
  a.above += (v > xl || (v == xl && col < lab)) ? 1 : 0;
  a.flags |= (v != v ? 1 : 0) | (v == INFINITY ? 2 : 0);
}

__device__ __forceinline__ void acc_eight(RowAcc& a, const float (&v)[8], int col0, float xl, int lab) {
  ms_add8(a.m, a.s, v);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a.above += (v[k] > xl || (v[k] == xl && col0 + k < lab)) ? 1 : 0;
    a.flags |= (v[k] != v[k] ? 1 : 0) | (v[k] == INFINITY ? 2 : 0);
  }
}

// a lane's share of one row: lanes `tid` of `nthr`
template <typename T, bool VEC>
__device__ __forceinline__ void scan_row(RowAcc& a, const T* xr, int V, int tid, int nthr, float xl, int lab) {
  if constexpr (VEC) {
    const bf16_t* xb = reinterpret_cast<const bf16_t*>(xr);
    for (int c = tid; c < (V >> 3); c += nthr) {
      float v[8];
      load8_bf16(xb + c * 8, v);
      acc_eight(a, v, c * 8, xl, lab);
    }
  } else {
    for (int j = tid; j < V; j += nthr) acc_one(a, ld<T>(xr, j), j, xl, lab);
  }
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_or_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}

// The online sum turns a +inf into NaN as soon as a second value follows it; a row's logsumexp is NaN only if the row
// holds a NaN, and +inf if it holds a +inf.
__device__ __forceinline__ float fix_lse(float lse, int flags) {
  return (flags & 1) ? __builtin_nanf("") : (flags & 2) ? INFINITY : lse;
}

__device__ __forceinline__ void write_row(float* loss, int* rank, long long row, float lse, float xl, int above, int V) {
  loss[row] = lse - xl;
  rank[row] = (xl != xl || lse != lse) ? V : above;
}

// rows whose label selects no column: true if the row is done
__device__ __forceinline__ bool special_row(long long lab, int V, float* loss, int* rank, long long row, bool writer) {
  if (lab >= 0 && lab < V) return false;
  if (writer) {
    loss[row] = 0.f;
    rank[row] = lab < 0 ? -1 : -2;
  }
  return true;
}

// one wave per row, 4 rows per 256-thread workgroup; nothing is shared between the waves, so the waves of a partly
// filled last workgroup simply leave
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) xent_rank_wave_kernel(const T* __restrict__ x, const long long* __restrict__ label,
                                                             long long B, int V, float* __restrict__ loss,
                                                             int* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const long long lab = label[row];
  if (special_row(lab, V, loss, rank, row, lane == 0)) return;
  const T* xr = x + row * V;
  const float xl = ld<T>(xr, lab);
  RowAcc a;
  scan_row<T, VEC>(a, xr, V, lane, 64, xl, (int)lab);
  wave_ms(a.m, a.s);
  const int above = wave_sum_i(a.above), flags = wave_or_i(a.flags);
  if (lane == 0) write_row(loss, rank, row, fix_lse(a.m + __logf(a.s), flags), xl, above, V);
}

// one 256-thread workgroup per row
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) xent_rank_block_kernel(const T* __restrict__ x,
                                                              const long long* __restrict__ label, int V,
                                                              float* __restrict__ loss, int* __restrict__ rank) {
  __shared__ float red[2][4];
  __shared__ int redi[2][4];
  const long long row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long long lab = label[row];
  if (special_row(lab, V, loss, rank, row, tid == 0)) return;  // the whole workgroup leaves: no barrier is skipped
  const T* xr = x + row * V;
  const float xl = ld<T>(xr, lab);
  RowAcc a;
  scan_row<T, VEC>(a, xr, V, tid, 256, xl, (int)lab);
  const int wabove = wave_sum_i(a.above), wflags = wave_or_i(a.flags);
  if (lane == 0) {
    redi[0][wid] = wabove;
    redi[1][wid] = wflags;
  }
  const float lse = block_lse(a.m, a.s, red);  // its barrier also publishes redi
  if (tid == 0) {
    const int above = redi[0][0] + redi[0][1] + redi[0][2] + redi[0][3];
    const int flags = redi[1][0] | redi[1][1] | redi[1][2] | redi[1][3];
    write_row(loss, rank, row, fix_lse(lse, flags), xl, above, V);
  }
}

void xent_rank(const void* x, int x_bf16, const long long* label, long long B, int V, float* loss, int* rank,
               hipStream_t st) {
  if (B <= 0) return;
  const bool vec = x_bf16 && (V % 8) == 0 && ((uintptr_t)x % 16) == 0;
  if (V <= kWaveRowMaxV) {
    const unsigned grid = (unsigned)((B + 3) / 4);
    if (vec)
      xent_rank_wave_kernel<bf16_t, true><<<grid, 256, 0, st>>>((const bf16_t*)x, label, B, V, loss, rank);
    else if (x_bf16)
      xent_rank_wave_kernel<bf16_t, false><<<grid, 256, 0, st>>>((const bf16_t*)x, label, B, V, loss, rank);
    else
      xent_rank_wave_kernel<float, false><<<grid, 256, 0, st>>>((const float*)x, label, B, V, loss, rank);
  } else {
    if (vec)
      xent_rank_block_kernel<bf16_t, true><<<(unsigned)B, 256, 0, st>>>((const bf16_t*)x, label, V, loss, rank);
    else if (x_bf16)
      xent_rank_block_kernel<bf16_t, false><<<(unsigned)B, 256, 0, st>>>((const bf16_t*)x, label, V, loss, rank);
    else
      xent_rank_block_kernel<float, false><<<(unsigned)B, 256, 0, st>>>((const float*)x, label, V, loss, rank);
  }
  DTG_LAUNCH_CHECK();
}

// ---- metric_accumulate ---------------------------------------------------------------------------------------------
struct MetricKs {
  int k[4];
  int n;
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// thread t takes rows t, t + 256, ...; counts are int32 (B < 2^31), the loss sum is fp64 from the first addition on.
// Then the wave butterfly, then wave 0..3 in that order: the order of every addition is a function of B alone.
__global__ void __launch_bounds__(256) metric_accumulate_kernel(const float* __restrict__ loss,
                                                                const int* __restrict__ rank, long long B, int V,
                                                                MetricKs ks, double* __restrict__ acc) {
  __shared__ double red[4][8];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int cnt[7] = {0, 0, 0, 0, 0, 0, 0};  // n, bad labels, non-finite, k0..k3
  double lsum = 0.0;
  for (long long r = tid; r < B; r += 256) {
    const int rk = rank[r];
    if (rk >= 0) {
      cnt[0] += 1;
      lsum += (double)loss[r];
    }
    cnt[1] += rk == -2;
    cnt[2] += rk == V;
#pragma unroll
    for (int i = 0; i < 4; ++i) cnt[3 + i] += (i < ks.n && rk >= 0 && rk < ks.k[i]) ? 1 : 0;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) cnt[i] = wave_sum_i(cnt[i]);
  lsum = wave_sum_d(lsum);
  if (lane == 0) {
    red[wid][0] = (double)cnt[0];
    red[wid][1] = lsum;
#pragma unroll
    for (int i = 1; i < 7; ++i) red[wid][1 + i] = (double)cnt[i];
  }
  __syncthreads();
  if (tid < 8) acc[tid] += ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

void metric_accumulate(const float* loss, const int* rank, long long B, int V, const int* ks, int nk, double* acc,
                       hipStream_t st) {
  if (B <= 0) return;
  MetricKs k{{0, 0, 0, 0}, nk};
  for (int i = 0; i < nk && i < 4; ++i) k.k[i] = ks[i];
  metric_accumulate_kernel<<<1, 256, 0, st>>>(loss, rank, B, V, k, acc);
  DTG_LAUNCH_CHECK();
}

}  // namespace dtg
