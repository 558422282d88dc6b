// Packed token rows for BERT without padding: the row plumbing between the padded layout [B * S, W] (what the
// attention kernels and the heads take) and the packed layout [T_alloc, W] (what every token-wise GEMM, LayerNorm,
// dropout and GELU of the encoder runs on), T = sum(len), T_alloc = T rounded up to 64 rows.
//
//   seq_offsets        cu[0] = 0, cu[b + 1] = cu[b] + clamp(length[b], 0, S)      (one workgroup, looping scan)
//   seq_pad            dst[b * S + s] = src[cu[b] + s] for s < len[b]; every other row of dst = 0
//   seq_unpad          dst[cu[b] + s] = src[b * S + s] for s < len[b]; rows T .. T_alloc - 1 of dst = 0
//   emb_fwd_packed     seq_unpad(emb_fwd(ids)) without the padded intermediate: the same sum in the same order
//   seq_gather_ids     seq_unpad for the int64 ids and token types (tail rows take id 0)
//   emb_pos_bwd_packed gP[p] += sum over b with len[b] > p of ds[cu[b] + p], fp32, a fixed order over b
//
// Addressing is by the padded coordinate (b, s) and cu[b] in both directions: a wave owns one padded row and either
// copies it or knows that it is padding, so no direction needs a search or a per-token table, every packed row has
// exactly one writer, and every store is a plain 16-byte vector store (no atomics).  Rows are bf16 of width W with
// W % 8 == 0 and 16-byte aligned bases; the bindings refuse anything else (seqpack_ops.cc).
//
// The tail-row invariant.  Rows T .. T_alloc - 1 of a packed tensor belong to no token.  Forward they hold zeros
// after the embedding sum and finite values after every later kernel (LayerNorm of a zero row is beta; a GEMM row
// depends on its own input row only).  Backward their upstream gradient is EXACTLY zero, because seq_unpad -- the
// backward of seq_pad, through which every gradient enters the packed encoder -- writes zeros there.  LayerNorm
// backward maps a zero row to a zero row and adds zero to dgamma / dbeta / dbias, the GELU' epilogue multiplies by
// zero, a dgrad GEMM row of a zero row is zero, and the column sums and weight gradients add x^T * 0: the tail
// contributes exactly zero to every parameter gradient.  The same holds for the padded rows of dQKV (see the
// argument next to the attention backward call in models/bert_fused.py).
//
// The overrun guard.  T_alloc comes from the host's copy of the lengths, cu from the device's.  Should the two ever
// disagree, a row whose packed index is negative or >= T_alloc is treated as padding: it is never read and never
// written.  Lengths are clamped to [0, S] where cu is built, and cu[b + 1] - cu[b] is clamped again where it is used.
#include "dtg/common.h"
#include "dtg/kernels.h"

namespace dtg {

namespace {

constexpr int kRows = 4;        // waves (rows) per workgroup
constexpr int kTailWaves = 64;  // waves that zero the tail rows, striding: any tail length is covered

// padded row r = b * S + s -> its packed row, or -1 when (b, s) is padding or the packed row lies outside
// [0, T_alloc)
__device__ __forceinline__ long long packed_row(const int* __restrict__ cu, int b, int s, int S, long long T_alloc) {
  const int base = cu[b];
  int len = cu[b + 1] - base;
  len = len < 0 ? 0 : (len > S ? S : len);
  const long long t = (long long)base + s;
  return (s < len && t >= 0 && t < T_alloc) ? t : -1;
}

__device__ __forceinline__ void zero_row(bf16_t* __restrict__ row, int nvec, int lane) {
  uint4* d = reinterpret_cast<uint4*>(row);
  for (int c = lane; c < nvec; c += 64) d[c] = make_uint4(0u, 0u, 0u, 0u);
}

// waves BS .. BS + kTailWaves - 1: wave j zeroes the rows cu[B] + j, cu[B] + j + kTailWaves, ... below T_alloc
__device__ __forceinline__ void zero_tail(bf16_t* __restrict__ dst, const int* __restrict__ cu, int B, int j,
                                          long long T_alloc, int W, int lane) {
  long long t = (long long)cu[B] + j;
  if (t < 0) t += ((-t + kTailWaves - 1) / kTailWaves) * kTailWaves;
  for (; t < T_alloc; t += kTailWaves) zero_row(dst + t * W, W >> 3, lane);
}

__global__ void __launch_bounds__(256) seq_offsets_kernel(const int* __restrict__ length, int* __restrict__ cu, int B,
                                                          int S) {
  __shared__ int wsum[4];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) {
    carry = 0;
    cu[0] = 0;
  }
  __syncthreads();
  for (int i0 = 0; i0 < B; i0 += 256) {
    const int i = i0 + tid;
    int v = 0;
    if (i < B) {
      v = length[i];
      v = v < 0 ? 0 : (v > S ? S : v);
    }
    int x = v;  // inclusive scan within the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wv; ++w) before += wsum[w];
    if (i < B) cu[i + 1] = before + x;
    __syncthreads();
    if (tid == 255) carry = before + x;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) seq_pad_kernel(const bf16_t* __restrict__ src, const int* __restrict__ cu,
                                                      bf16_t* __restrict__ dst, int B, int S, long long T_alloc,
                                                      int W) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (r >= (long long)B * S) return;
  const int b = (int)(r / S), s = (int)(r % S);
  const long long t = packed_row(cu, b, s, S, T_alloc);
  const int nvec = W >> 3;
  if (t < 0) {
    zero_row(dst + r * W, nvec, lane);
    return;
  }
  const uint4* a = reinterpret_cast<const uint4*>(src + t * W);
  uint4* d = reinterpret_cast<uint4*>(dst + r * W);
  for (int c = lane; c < nvec; c += 64) d[c] = a[c];
}

__global__ void __launch_bounds__(256) seq_unpad_kernel(const bf16_t* __restrict__ src, const int* __restrict__ cu,
                                                        bf16_t* __restrict__ dst, int B, int S, long long T_alloc,
                                                        int W) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  const long long BS = (long long)B * S;
  if (r >= BS) {
    if (r < BS + kTailWaves) zero_tail(dst, cu, B, (int)(r - BS), T_alloc, W, lane);
    return;
  }
  const int b = (int)(r / S), s = (int)(r % S);
  const long long t = packed_row(cu, b, s, S, T_alloc);
  if (t < 0) return;
  const uint4* a = reinterpret_cast<const uint4*>(src + r * W);
  uint4* d = reinterpret_cast<uint4*>(dst + t * W);
  for (int c = lane; c < (W >> 3); c += 64) d[c] = a[c];
}

// out[cu[b] + s] = word[ids[b, s]] + (pos[s] + type[tt[b, s]]): emb_fwd_kernel's sum, term for term
__global__ void __launch_bounds__(256) emb_fwd_packed_kernel(const long long* __restrict__ ids,
                                                             const long long* __restrict__ tt,
                                                             const bf16_t* __restrict__ word,
                                                             const bf16_t* __restrict__ pos,
                                                             const bf16_t* __restrict__ type,
                                                             const int* __restrict__ cu, bf16_t* __restrict__ out,
                                                             int B, int S, long long T_alloc, int H) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * kRows + (threadIdx.x >> 6);
  const long long BS = (long long)B * S;
  if (r >= BS) {
    if (r < BS + kTailWaves) zero_tail(out, cu, B, (int)(r - BS), T_alloc, H, lane);
    return;
  }
  const int b = (int)(r / S), s = (int)(r % S);
  const long long t = packed_row(cu, b, s, S, T_alloc);
  if (t < 0) return;
  const bf16_t* w = word + ids[r] * (long long)H;
  const bf16_t* p = pos + (long long)s * H;
  const bf16_t* ty = tt ? type + tt[r] * (long long)H : nullptr;
  for (int c = lane; c < (H >> 3); c += 64) {
    float a[8], q[8], d[8];
    load8_bf16(w + c * 8, a);
    load8_bf16(p + c * 8, q);
    if (ty) load8_bf16(ty + c * 8, d);
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] += q[k] + (ty ? d[k] : 0.f);
    store8_bf16(out + t * H + c * 8, a);
  }
}

// one thread per padded position; threads BS .. : the tail ids (0)
__global__ void __launch_bounds__(256) seq_gather_ids_kernel(const long long* __restrict__ ids,
                                                             const long long* __restrict__ tt,
                                                             const int* __restrict__ cu, long long* __restrict__ ids_out,
                                                             long long* __restrict__ tt_out, int B, int S,
                                                             long long T_alloc) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long BS = (long long)B * S;
  if (r >= BS) {
    if (r >= BS + 256) return;
    long long t = (long long)cu[B] + (r - BS);
    if (t < 0) t += ((-t + 255) / 256) * 256;
    for (; t < T_alloc; t += 256) {
      ids_out[t] = 0;
      if (tt_out) tt_out[t] = 0;
    }
    return;
  }
  const long long t = packed_row(cu, (int)(r / S), (int)(r % S), S, T_alloc);
  if (t < 0) return;
  ids_out[t] = ids[r];
  if (tt_out) tt_out[t] = tt[r];
}

// One workgroup per (position p, block of 64 column chunks): wave g sums the sequences g, g + 4, ... that reach p
// (two independent loads in flight), lane = chunk; the four partial sums are added in wave order through LDS.  The
// order over b is fixed by (B, the lengths) alone: the result does not depend on scheduling.
__global__ void __launch_bounds__(256) emb_pos_bwd_packed_kernel(const bf16_t* __restrict__ ds,
                                                                 const int* __restrict__ cu, bf16_t* __restrict__ gP,
                                                                 int B, int S, long long T_alloc, int H) {
  __shared__ float red[kRows][64 * 8];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int p = blockIdx.x, c = blockIdx.y * 64 + lane;
  const bool on = c < (H >> 3);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (on) {
    int b = g;
    for (; b + kRows < B; b += 2 * kRows) {
      const long long t0 = packed_row(cu, b, p, S, T_alloc), t1 = packed_row(cu, b + kRows, p, S, T_alloc);
      float v0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, v1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (t0 >= 0) load8_bf16(ds + t0 * H + c * 8, v0);
      if (t1 >= 0) load8_bf16(ds + t1 * H + c * 8, v1);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += v0[k] + v1[k];
    }
    for (; b < B; b += kRows) {
      const long long t0 = packed_row(cu, b, p, S, T_alloc);
      if (t0 < 0) continue;
      float v0[8];
      load8_bf16(ds + t0 * H + c * 8, v0);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += v0[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) red[g][lane * 8 + k] = acc[k];
  __syncthreads();
  if (g == 0 && on) {
    float o[8];
    bf16_t* dst = gP + (long long)p * H + c * 8;
    load8_bf16(dst, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = lane * 8 + k;
      o[k] += (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
    store8_bf16(dst, o);
  }
}

inline unsigned rows_grid(long long rows) { return (unsigned)((rows + kRows - 1) / kRows); }

}  // namespace

void seq_offsets(const int* length, int* cu, int B, int S, hipStream_t st) {
  hipLaunchKernelGGL(seq_offsets_kernel, dim3(1), dim3(256), 0, st, length, cu, B, S); DTG_LAUNCH_CHECK();
}

void seq_pad(const bf16_t* src, const int* cu, bf16_t* dst, int B, int S, long long T_alloc, int W, hipStream_t st) {
  if ((long long)B * S <= 0) return;
  hipLaunchKernelGGL(seq_pad_kernel, dim3(rows_grid((long long)B * S)), dim3(256), 0, st, src, cu, dst, B, S, T_alloc,
                     W); DTG_LAUNCH_CHECK();
}

void seq_unpad(const bf16_t* src, const int* cu, bf16_t* dst, int B, int S, long long T_alloc, int W, hipStream_t st) {
  if (T_alloc <= 0) return;
  hipLaunchKernelGGL(seq_unpad_kernel, dim3(rows_grid((long long)B * S + kTailWaves)), dim3(256), 0, st, src, cu, dst,
                     B, S, T_alloc, W); DTG_LAUNCH_CHECK();
}

void emb_fwd_packed(const long long* ids, const long long* tt, const bf16_t* word, const bf16_t* pos,
                    const bf16_t* type, const int* cu, bf16_t* out, int B, int S, long long T_alloc, int H,
                    hipStream_t st) {
  if (T_alloc <= 0) return;
  hipLaunchKernelGGL(emb_fwd_packed_kernel, dim3(rows_grid((long long)B * S + kTailWaves)), dim3(256), 0, st, ids, tt,
                     word, pos, type, cu, out, B, S, T_alloc, H); DTG_LAUNCH_CHECK();
}

void seq_gather_ids(const long long* ids, const long long* tt, const int* cu, long long* ids_out, long long* tt_out,
                    int B, int S, long long T_alloc, hipStream_t st) {
  if (T_alloc <= 0) return;
  const long long n = (long long)B * S + 256;
  hipLaunchKernelGGL(seq_gather_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ids, tt, cu, ids_out,
                     tt_out, B, S, T_alloc); DTG_LAUNCH_CHECK();
}

void emb_pos_bwd_packed(const bf16_t* ds, const int* cu, bf16_t* gP, int B, int S, long long T_alloc, int H,
                        hipStream_t st) {
  if (B <= 0 || S <= 0 || T_alloc <= 0) return;
  hipLaunchKernelGGL(emb_pos_bwd_packed_kernel, dim3(S, (H / 8 + 63) / 64), dim3(256), 0, st, ds, cu, gP, B, S,
                     T_alloc, H); DTG_LAUNCH_CHECK();
}

}  // namespace dtg
