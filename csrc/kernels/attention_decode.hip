// Incremental decoding: one query row per (record, head) against a KV cache.  Head dim 64, bf16, no dropout, no
// additive mask.  kcache / vcache are bf16 [B, nh, S_max, 64]: one head's keys are one contiguous stream of 128-byte
// rows, S_max any positive int.  Record b holds len_b = lens0[b] + t cached keys before the call (lens0 int32 on the
// device, t a host int: nothing is read back).  The new token's q, k, v come in qkv1 [B, 3H] (row layout
// [3][nh][64]); its position is len_b and it sees cached keys max(0, len_b + 1 - window) .. len_b - 1 plus its own key
// (window = 0: every key).  A record with len_b < 0 or len_b >= S_max writes nothing to the cache and gets zeros.
//
// The shape is bandwidth-bound on the K/V bytes and B * nh is far below what fills the device, so the keys of one
// (record, head) are split over blockIdx.y:
//
//   grid [B * nh, nsplit], 4 waves per workgroup.  With lo = max(0, len + 1 - window), the record's chunks (64 keys
//   each) are c_lo = lo / 64 .. c_hi = len / 64; split s owns chunks c_lo + s * cps .. c_lo + (s + 1) * cps - 1, cut at
//   c_hi (the last split runs up to c_hi whatever cps is, so a host that underestimated max_len loses speed, not
//   keys).  The window bounds the chunks at both ends; a split wholly outside c_lo .. c_hi writes the empty partial
//   (m = -inf, l = 0, acc = 0) and leaves.  Wave w of the workgroup takes chunks cb + w, cb + w + 4, ...
//
//   Keys across lanes, dims across 8 lanes.  A 16-byte load of lane (r = lane / 8, sub = lane % 8) takes dims
//   8 sub .. 8 sub + 7 of key 8 i + r of the chunk (i = 0 .. 7): one load instruction of a wave reads 8 whole rows,
//   1 KiB contiguous, and a chunk is 8 such loads of K and 8 of V, all issued before the arithmetic.  q (scaled by
//   log2(e) / 8, fp32) lives in the same layout, so a score is 8 lane-private FMAs and a 3-step butterfly over the 8
//   lanes of a row (xor 1, 2, 4); the chunk maximum is a butterfly over the 8 row groups (xor 8, 16, 32).  P V needs no
//   cross-lane step at all until the end: lane (r, sub) accumulates p[key] * V[key][8 sub + j] over its own keys, and
//   the 8 row groups are summed once per wave after the loop.  No LDS in the loop, no transpose, no MFMA: an MFMA form
//   would spend 15/16 of the pipe on padding rows and still has to put K through LDS or a fragment shuffle, while
//   this form runs ~350 VALU instructions per 16 KiB chunk, two orders of magnitude below the HBM time of the chunk.
//
//   Every visible K and V byte is read exactly once; an invisible row (below lo, or at and above len -- row len
//   itself included, which this launch writes) is NOT loaded: its registers are zeros and its score is -inf, so the
//   key is out of the maximum and the sum (P = 0 exactly) whatever the cache holds there, and rows at and beyond S_max
//   are never addressed.  Interior chunks take an unpredicated body.  A chunk can hold no visible key (c_hi when
//   len % 64 == 0): its maximum is -inf and the running maximum may still be; the body then subtracts 0 instead
//   (alpha = exp2(-inf) = 0 on l = acc = 0), attention_window.hip's rule.
//
//   The new token.  The workgroup whose split holds chunk c_hi owns position len: its wave 0 folds the token's own
//   key and value in from qkv1 (never from the cache) and writes them to cache row len with 16-byte stores.  No other
//   workgroup touches that row in this launch, so the append needs no ordering.
//
//   The 4 waves' (m, l, acc[64]) meet in LDS; 64 threads merge them (attn_decode_common.cuh).  nsplit = 1: they write ctx (bf16) and lse.
//   nsplit > 1: they write the fp32 partial to ws[(bh * nsplit + s) * 66 + {0: m (log2 units), 1: l, 2..65: acc}] and
//   attn_decode_combine_kernel (grid B * nh, 64 threads) merges the splits: no atomics, no "last workgroup" scheme.
//
// kv_cache_fill_kernel is the prefill's copy of the K and V thirds of a padded qkv [B * S0, 3H] into the cache (rows
// below min(lens0[b], S0, S_max) only, 16 bytes per thread); emb_fwd_at_kernel sums the embeddings of one token per
// record at position lens0[b] + t (token type 0), in emb_fwd_kernel's order: word + (pos + type), one rounding.
#include "dtg/attn_decode_common.cuh"
#include "dtg/kernels.h"

namespace dtg {

namespace {
using namespace adec;  // kNW, kPart, kMaxSplits, kLog2e, kLn2, max_chunks, merge_waves
constexpr int kTargetWgs = 1024;  // workgroups the split choice aims at: 4 per CU

int g_force_splits = 0;  // attn_decode_force_splits: 0 = choose from max_len

__device__ __forceinline__ void unpack8(const u32x4v v, float (&o)[8]) {
  o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
  o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  o[4] = __uint_as_float(v.z << 16); o[5] = __uint_as_float(v.z & 0xffff0000u);
  o[6] = __uint_as_float(v.w << 16); o[7] = __uint_as_float(v.w & 0xffff0000u);
}
// over the 8 lanes that hold one key row (lane % 8)
__device__ __forceinline__ float dim_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v + __shfl_xor(v, 4, 64);
}
// over the 8 row groups (lane / 8)
__device__ __forceinline__ float rows_sum(float v) {
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float rows_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 8, 64));
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float dot8(const float (&a)[8], const float (&b)[8]) {
  float s = a[0] * b[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) s = fmaf(a[j], b[j], s);
  return s;
}

// One 64-key chunk for a wave.  kFull: every key of the chunk is visible; otherwise key x of it is visible iff
// lo <= k0 + x < len, and an invisible row is not loaded.
template <bool kFull>
__device__ __forceinline__ void decode_chunk(const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc, int k0,
                                             int lo, int len, int r, int sub, const float (&q)[8], float& m, float& l,
                                             float (&acc)[8]) {
  const u32x4v zero = {0u, 0u, 0u, 0u};
  u32x4v kk[8], vv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int key = k0 + i * 8 + r;
    const long long off = (long long)key * 64 + sub * 8;
    const bool vis = kFull || (key >= lo && key < len);
    kk[i] = vis ? *reinterpret_cast<const u32x4v*>(kc + off) : zero;
    vv[i] = vis ? *reinterpret_cast<const u32x4v*>(vc + off) : zero;
  }
  float s[8], mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int key = k0 + i * 8 + r;
    float kf[8];
    unpack8(kk[i], kf);
    const float d = dim_sum(dot8(kf, q));
    s[i] = (kFull || (key >= lo && key < len)) ? d : -INFINITY;  // excluded: out of the max, P = 0 below
    mx = fmaxf(mx, s[i]);
  }
  mx = rows_max(mx);
  const float mn = fmaxf(m, mx);
  const float mref = (!kFull && mn == -INFINITY) ? 0.f : mn;  // no visible key so far: alpha = 0 on l = acc = 0
  const float alpha = __builtin_amdgcn_exp2f(m - mref);
  m = mn;
  l *= alpha;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] *= alpha;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float p = __builtin_amdgcn_exp2f(s[i] - mref);
    float vf[8];
    unpack8(vv[i], vf);
    l += p;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaf(p, vf[j], acc[j]);
  }
}

__global__ void __launch_bounds__(64 * kNW) attn_decode_kernel(
    const bf16_t* __restrict__ qkv1, const int* __restrict__ lens0, int t, bf16_t* __restrict__ kcache,
    bf16_t* __restrict__ vcache, float* __restrict__ ws, bf16_t* __restrict__ ctx, float* __restrict__ lse, int nh,
    int S_max, int window, int cps, float scale_l2) {
  __shared__ float red[kNW][kPart + 2];
  const int bh = blockIdx.x, b = bh / nh, h = bh - b * nh, sp = blockIdx.y, nsplit = gridDim.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, sub = lane & 7, r = lane >> 3;
  const int H = nh * 64;
  const int len = lens0[b] + t;
  float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (len >= 0 && len < S_max) {  // (uniform over the workgroup)
    const int lo = window > 0 ? (len + 1 - window > 0 ? len + 1 - window : 0) : 0;
    const int c_lo = lo >> 6, c_hi = len >> 6;
    const int cb = c_lo + sp * cps;
    const int ce = (sp == nsplit - 1 || cb + cps > c_hi) ? c_hi + 1 : cb + cps;
    const bf16_t* qrow = qkv1 + (long long)b * 3 * H + h * 64 + sub * 8;
    float q[8];
    load8_bf16(qrow, q);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] *= scale_l2;
    const long long hb = (long long)bh * S_max * 64;
    for (int c = cb + wave; c < ce; c += kNW) {
      const int k0 = c * 64;
      if (k0 >= lo && k0 + 64 <= len)
        decode_chunk<true>(kcache + hb, vcache + hb, k0, lo, len, r, sub, q, m, l, acc);
      else
        decode_chunk<false>(kcache + hb, vcache + hb, k0, lo, len, r, sub, q, m, l, acc);
    }
    if (wave == 0 && cb <= c_hi && c_hi < ce) {
      // the new token: its key is always visible and comes from qkv1; row group 0 carries it into l and acc, and
      // appends the k / v rows to the cache at position len
      const u32x4v kn = *reinterpret_cast<const u32x4v*>(qrow + H), vn = *reinterpret_cast<const u32x4v*>(qrow + 2 * H);
      float kf[8], vf[8];
      unpack8(kn, kf);
      unpack8(vn, vf);
      const float sn = dim_sum(dot8(kf, q));
      const float mn = fmaxf(m, sn);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      const float p = r == 0 ? __builtin_amdgcn_exp2f(sn - mn) : 0.f;
      m = mn;
      l = l * alpha + p;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(p, vf[j], acc[j] * alpha);
      if (r == 0) {
        const long long off = hb + (long long)len * 64 + sub * 8;
        *reinterpret_cast<u32x4v*>(kcache + off) = kn;
        *reinterpret_cast<u32x4v*>(vcache + off) = vn;
      }
    }
  }
  // the wave's 8 row groups -> one (m, l, acc[64]); m is already uniform over the wave
  l = rows_sum(l);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = rows_sum(acc[j]);
  if (r == 0) {
    if (sub == 0) {
      red[wave][0] = m;
      red[wave][1] = l;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wave][2 + sub * 8 + j] = acc[j];
  }
  __syncthreads();
  if (tid >= 64) return;
  merge_waves(red, tid, b, h, bh, H, sp, nsplit, ws, ctx, lse);
}

// merges the nsplit partials of a (record, head): thread d owns dim d
__global__ void __launch_bounds__(64) attn_decode_combine_kernel(const float* __restrict__ ws, bf16_t* __restrict__ ctx,
                                                                 float* __restrict__ lse, int nh, int nsplit) {
  const int bh = blockIdx.x, b = bh / nh, h = bh - b * nh, d = threadIdx.x;
  const float* part = ws + (long long)bh * nsplit * kPart;
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, part[s * kPart]);
  float L = 0.f, a = 0.f;
  if (M != -INFINITY) {
    for (int s = 0; s < nsplit; ++s) {
      const float f = __builtin_amdgcn_exp2f(part[s * kPart] - M);  // an empty partial: exp2(-inf) = 0
      L = fmaf(f, part[s * kPart + 1], L);
      a = fmaf(f, part[s * kPart + 2 + d], a);
    }
  }
  ctx[(long long)b * nh * 64 + h * 64 + d] = f2bf(L > 0.f ? a / L : 0.f);
  if (d == 0) lse[bh] = L > 0.f ? fmaf(M, kLn2, __logf(L)) : 0.f;
}

// thread -> 16 bytes of K and of V: index ((s * nh + h) * 8 + sub) of record blockIdx.y
__global__ void __launch_bounds__(256) kv_cache_fill_kernel(const bf16_t* __restrict__ qkv,
                                                            const int* __restrict__ lens0, bf16_t* __restrict__ kcache,
                                                            bf16_t* __restrict__ vcache, int S0, int nh, int S_max) {
  const int b = blockIdx.y, H = nh * 64;
  int n = lens0[b];
  n = n < S0 ? n : S0;
  n = n < S_max ? n : S_max;
  const long long total = (long long)n * nh * 8;  // (n <= 0: nothing)
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int sub = (int)(i & 7), h = (int)((i >> 3) % nh), s = (int)((i >> 3) / nh);
    const bf16_t* src = qkv + ((long long)b * S0 + s) * 3 * H + H + h * 64 + sub * 8;
    const long long dst = (((long long)b * nh + h) * S_max + s) * 64 + sub * 8;
    *reinterpret_cast<u32x4v*>(kcache + dst) = *reinterpret_cast<const u32x4v*>(src);
    *reinterpret_cast<u32x4v*>(vcache + dst) = *reinterpret_cast<const u32x4v*>(src + H);
  }
}

// a wave per record; ids and positions are clamped into their tables
__global__ void __launch_bounds__(256) emb_fwd_at_kernel(const long long* __restrict__ ids,
                                                         const int* __restrict__ lens0, int t,
                                                         const bf16_t* __restrict__ word, const bf16_t* __restrict__ pos,
                                                         const bf16_t* __restrict__ type, bf16_t* __restrict__ out,
                                                         int B, int H, int V, int P) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  long long id = ids[b];
  id = id < 0 ? 0 : (id < V ? id : V - 1);
  int p = lens0[b] + t;
  p = p < 0 ? 0 : (p < P ? p : P - 1);
  const bf16_t* w = word + id * H;
  const bf16_t* pp = pos + (long long)p * H;
  for (int c = lane; c < (H >> 3); c += 64) {
    float x[8], y[8], z[8];
    load8_bf16(w + c * 8, x);
    load8_bf16(pp + c * 8, y);
    load8_bf16(type + c * 8, z);
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] += y[k] + z[k];
    store8_bf16(out + (long long)b * H + c * 8, x);
  }
}

}  // namespace

int attn_decode_supported(int dh, int S_max) { return dh == 64 && S_max >= 1 && S_max <= (1 << 30); }

void attn_decode_force_splits(int nsplit) { g_force_splits = nsplit < 0 ? 0 : (nsplit < kMaxSplits ? nsplit : kMaxSplits); }
int attn_decode_force_splits_get() { return g_force_splits; }

int attn_decode_splits(int bh, int max_len, int window) {
  if (g_force_splits > 0) return g_force_splits;
  const int chunks = max_chunks(max_len < 0 ? 0 : max_len, window);
  int n = (kTargetWgs + bh - 1) / (bh > 0 ? bh : 1);
  const int cap = (chunks + kNW - 1) / kNW;  // at least a chunk per wave: nsplit = 1 below 256 keys
  n = n < cap ? n : cap;
  n = n < kMaxSplits ? n : kMaxSplits;
  return n < 1 ? 1 : n;
}

void attn_decode(const bf16_t* qkv1, const int* lens0, int t, int max_len, bf16_t* kcache, bf16_t* vcache, float* ws,
                 int nsplit, bf16_t* ctx, float* lse, int B, int nh, int S_max, int window, hipStream_t st) {
  if (B <= 0 || nh <= 0) return;
  if (!attn_decode_supported(64, S_max) || nsplit < 1 || nsplit > kMaxSplits || (nsplit > 1 && !ws))
    throw std::runtime_error("dtg: attn_decode: 1 <= S_max <= 2^30, 1 <= nsplit <= 1024 and a workspace for nsplit > 1");
  const int chunks = max_chunks(max_len < 0 ? 0 : max_len, window);
  const int cps = (chunks + nsplit - 1) / nsplit;
  hipLaunchKernelGGL(attn_decode_kernel, dim3(B * nh, nsplit), dim3(64 * kNW), 0, st, qkv1, lens0, t, kcache, vcache,
                     ws, ctx, lse, nh, S_max, window, cps, kLog2e * 0.125f);
  DTG_LAUNCH_CHECK();
  if (nsplit > 1) attn_decode_combine(ws, ctx, lse, B, nh, nsplit, st);
}

void attn_decode_combine(const float* ws, bf16_t* ctx, float* lse, int B, int nh, int nsplit, hipStream_t st) {
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(B * nh), dim3(64), 0, st, ws, ctx, lse, nh, nsplit);
  DTG_LAUNCH_CHECK();
}

void kv_cache_fill(const bf16_t* qkv, const int* lens0, bf16_t* kcache, bf16_t* vcache, int B, int S0, int nh,
                   int S_max, hipStream_t st) {
  if (B <= 0 || S0 <= 0 || nh <= 0) return;
  const int rows = S0 < S_max ? S0 : S_max;
  hipLaunchKernelGGL(kv_cache_fill_kernel, dim3(grid_for((long long)rows * nh * 8, 256, 1024), B), dim3(256), 0, st,
                     qkv, lens0, kcache, vcache, S0, nh, S_max);
  DTG_LAUNCH_CHECK();
}

void emb_fwd_at(const long long* ids, const int* lens0, int t, const bf16_t* word, const bf16_t* pos,
                const bf16_t* type, bf16_t* out, int B, int H, int V, int P, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(emb_fwd_at_kernel, dim3((B + 3) / 4), dim3(256), 0, st, ids, lens0, t, word, pos, type, out, B, H,
                     V, P);
  DTG_LAUNCH_CHECK();
}

}  // namespace dtg
