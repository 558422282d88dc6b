// Incremental decoding against an FP8 KV cache: attention_decode.hip's kernels for a cache of half the width.
// kcache / vcache are OCP e4m3 [B, nh, S_max, 64], one byte per value: one head's keys are one contiguous stream of
// 64-byte rows.  Beside each sits kscale / vscale fp32 [B, nh, S_max], one scale per row.  A row x of 64 bf16 values is
// held as scale = amax|x| / 448 (1 when amax = 0) and code = e4m3_rne(x / scale), both in fp32 with a true division:
// the row's largest element lands on +-448, no quotient leaves the finite range, and torch's
// (x.float() / scale).to(float8_e4m3fn) gives the same bits.  The kernel reads 68 bytes per row where the bf16 kernel
// reads 128.  lens0, t, window, the refused lengths (len < 0 or len >= S_max: nothing written, zeros out), the grid
// [B * nh, nsplit] of 4 waves, the chunk split and the partials are attention_decode.hip's; what changes is the layout:
//
//   Keys across lanes, dims across 4 lanes.  A 16-byte load of lane (r = lane / 4, sub = lane % 4) takes dims
//   16 sub .. 16 sub + 15 of key 16 i + r of the chunk (i = 0 .. 3): one load instruction of a wave reads 16 whole rows,
//   1 KiB contiguous, and a chunk is 4 such loads of K and 4 of V plus, per i, the fp32 K and V scale of the lane's own
//   key (the 4 lanes of a row read the same address), all issued before the arithmetic.  q (scaled by log2(e) / 8,
//   fp32, 16 values per lane) lives in the same layout, so a score is 16 lane-private FMAs on converted codes
//   (v_cvt_pk_f32_fp8, two values per instruction), a 2-step butterfly over the 4 lanes of a row (xor 1, 2) and ONE
//   multiply by the key's K scale; the chunk maximum is a butterfly over the 16 row groups (xor 4, 8, 16, 32).  The V
//   scale goes into the probability, not into the 16 values: acc[j] += (p * vscale[key]) * V[key][16 sub + j], and
//   l += p.  The 16 row groups are summed once per wave after the loop.  Per lane and 64-key chunk that is 64
//   conversions, 128 FMAs and some 70 other VALU operations on 8.5 KiB of codes and scales: about twice the bf16
//   kernel's VALU work per byte, still far below the chunk's HBM time.
//
//   Exclusion is the bf16 kernel's, and it covers the scales: an invisible row (below lo, at and above len, so never
//   at or beyond S_max) has neither its codes nor its scales loaded; its registers are zeros and its score is -inf, so
//   a NaN code (0x7f) or a NaN / inf scale there never reaches the result.  Interior chunks take the unpredicated body;
//   while the running maximum is still -inf the body subtracts 0.
//
//   The new token.  Wave 0 of the workgroup whose split holds chunk c_hi takes the token's k and v from qkv1 in the
//   same layout and folds them into this step's softmax UNQUANTISED, as the bf16 kernel does.  The same 4 lanes of a
//   row then quantise them: amax over the lane's 16 values and a 2-step butterfly, 16 divisions, v_cvt_pk_fp8_f32, and
//   row group 0 writes row len (a 16-byte vector store per lane) and lane 0 the two scales.  No other workgroup touches
//   that row or those scales in this launch.
//
// kv_cache_fill_fp8_kernel is the prefill's copy with the same quantiser: 4 lanes per row, 32 bytes of bf16 in and 16
// bytes of codes out per lane for K and for V, one lane of the four stores the scales.
#include "dtg/attn_decode_common.cuh"
#include "dtg/kernels.h"

namespace dtg {

namespace {
using namespace adec;  // kNW, kPart, kMaxSplits, kLog2e, max_chunks, merge_waves

typedef __attribute__((ext_vector_type(2))) float f32x2;

// 16 e4m3 codes (a 16-byte load) -> 16 floats, in memory order
__device__ __forceinline__ void unpack16(const u32x4v v, float (&o)[16]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[d], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[d], true);
    o[4 * d] = a.x; o[4 * d + 1] = a.y; o[4 * d + 2] = b.x; o[4 * d + 3] = b.y;
  }
}
// 16 bf16 (32 bytes) -> 16 floats
__device__ __forceinline__ void load16_bf16(const bf16_t* p, float (&o)[16]) {
  float a[8], b[8];
  load8_bf16(p, a);
  load8_bf16(p + 8, b);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = a[j], o[8 + j] = b[j];
}
// over the 4 lanes that hold one key row (lane % 4)
__device__ __forceinline__ float dim_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  return v + __shfl_xor(v, 2, 64);
}
__device__ __forceinline__ float dim_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1, 64));
  return fmaxf(v, __shfl_xor(v, 2, 64));
}
// over the 16 row groups (lane / 4)
__device__ __forceinline__ float rows_sum(float v) {
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float rows_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 4, 64));
  v = fmaxf(v, __shfl_xor(v, 8, 64));
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float dot16(const float (&a)[16], const float (&b)[16]) {
  float s = a[0] * b[0];
#pragma unroll
  for (int j = 1; j < 16; ++j) s = fmaf(a[j], b[j], s);
  return s;
}

// A lane's 16 values of a row -> its 16 codes and the row's scale (the same in the row's 4 lanes).  The quotient of
// the largest element is 448 or an ulp beside it, which rounds to the code of 448: nothing saturates.
__device__ __forceinline__ u32x4v quantize16(const float (&x)[16], float& scale) {
  float amax = fabsf(x[0]);
#pragma unroll
  for (int j = 1; j < 16; ++j) amax = fmaxf(amax, fabsf(x[j]));
  amax = dim_max(amax);
  scale = amax == 0.f ? 1.f : amax / 448.f;
  u32x4v c;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * d] / scale, x[4 * d + 1] / scale, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * d + 2] / scale, x[4 * d + 3] / scale, w, true);
    c[d] = (unsigned)w;
  }
  return c;
}

// One 64-key chunk for a wave.  kFull: every key of the chunk is visible; otherwise key x of it is visible iff
// lo <= k0 + x < len, and an invisible row has neither its codes nor its scales loaded.
template <bool kFull>
__device__ __forceinline__ void decode_chunk(const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
                                             const float* __restrict__ ksc, const float* __restrict__ vsc, int k0,
                                             int lo, int len, int r, int sub, const float (&q)[16], float& m, float& l,
                                             float (&acc)[16]) {
  const u32x4v zero = {0u, 0u, 0u, 0u};
  u32x4v kk[4], vv[4];
  float ks[4], vs[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int key = k0 + i * 16 + r;
    const long long off = (long long)key * 64 + sub * 16;
    const bool vis = kFull || (key >= lo && key < len);
    kk[i] = vis ? *reinterpret_cast<const u32x4v*>(kc + off) : zero;
    vv[i] = vis ? *reinterpret_cast<const u32x4v*>(vc + off) : zero;
    ks[i] = vis ? ksc[key] : 0.f;
    vs[i] = vis ? vsc[key] : 0.f;
  }
  float s[4], mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int key = k0 + i * 16 + r;
    float kf[16];
    unpack16(kk[i], kf);
    const float d = dim_sum(dot16(kf, q)) * ks[i];
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
  for (int j = 0; j < 16; ++j) acc[j] *= alpha;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float p = __builtin_amdgcn_exp2f(s[i] - mref);
    const float pv = p * vs[i];
    float vf[16];
    unpack16(vv[i], vf);
    l += p;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = fmaf(pv, vf[j], acc[j]);
  }
}

__global__ void __launch_bounds__(64 * kNW) attn_decode_fp8_kernel(
    const bf16_t* __restrict__ qkv1, const int* __restrict__ lens0, int t, uint8_t* __restrict__ kcache,
    uint8_t* __restrict__ vcache, float* __restrict__ kscale, float* __restrict__ vscale, float* __restrict__ ws,
    bf16_t* __restrict__ ctx, float* __restrict__ lse, int nh, int S_max, int window, int cps, float scale_l2) {
  __shared__ float red[kNW][kPart + 2];
  const int bh = blockIdx.x, b = bh / nh, h = bh - b * nh, sp = blockIdx.y, nsplit = gridDim.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, sub = lane & 3, r = lane >> 2;
  const int H = nh * 64;
  const int len = lens0[b] + t;
  float m = -INFINITY, l = 0.f, acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  if (len >= 0 && len < S_max) {  // (uniform over the workgroup)
    const int lo = window > 0 ? (len + 1 - window > 0 ? len + 1 - window : 0) : 0;
    const int c_lo = lo >> 6, c_hi = len >> 6;
    const int cb = c_lo + sp * cps;
    const int ce = (sp == nsplit - 1 || cb + cps > c_hi) ? c_hi + 1 : cb + cps;
    const bf16_t* qrow = qkv1 + (long long)b * 3 * H + h * 64 + sub * 16;
    float q[16];
    load16_bf16(qrow, q);
#pragma unroll
    for (int j = 0; j < 16; ++j) q[j] *= scale_l2;
    const long long hs = (long long)bh * S_max, hb = hs * 64;
    for (int c = cb + wave; c < ce; c += kNW) {
      const int k0 = c * 64;
      if (k0 >= lo && k0 + 64 <= len)
        decode_chunk<true>(kcache + hb, vcache + hb, kscale + hs, vscale + hs, k0, lo, len, r, sub, q, m, l, acc);
      else
        decode_chunk<false>(kcache + hb, vcache + hb, kscale + hs, vscale + hs, k0, lo, len, r, sub, q, m, l, acc);
    }
    if (wave == 0 && cb <= c_hi && c_hi < ce) {
      // the new token: its key is always visible and enters unquantised from qkv1; row group 0 carries it into l and
      // acc, and appends the quantised k / v rows and their scales to the cache at position len
      float kf[16], vf[16];
      load16_bf16(qrow + H, kf);
      load16_bf16(qrow + 2 * H, vf);
      const float sn = dim_sum(dot16(kf, q));
      const float mn = fmaxf(m, sn);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      const float p = r == 0 ? __builtin_amdgcn_exp2f(sn - mn) : 0.f;
      m = mn;
      l = l * alpha + p;
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] = fmaf(p, vf[j], acc[j] * alpha);
      float sk, sv;
      const u32x4v kq = quantize16(kf, sk), vq = quantize16(vf, sv);
      if (r == 0) {
        const long long off = hb + (long long)len * 64 + sub * 16;
        *reinterpret_cast<u32x4v*>(kcache + off) = kq;
        *reinterpret_cast<u32x4v*>(vcache + off) = vq;
        if (sub == 0) {
          kscale[hs + len] = sk;
          vscale[hs + len] = sv;
        }
      }
    }
  }
  // the wave's 16 row groups -> one (m, l, acc[64]); m is already uniform over the wave
  l = rows_sum(l);
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = rows_sum(acc[j]);
  if (r == 0) {
    if (sub == 0) {
      red[wave][0] = m;
      red[wave][1] = l;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) red[wave][2 + sub * 16 + j] = acc[j];
  }
  __syncthreads();
  if (tid >= 64) return;
  merge_waves(red, tid, b, h, bh, H, sp, nsplit, ws, ctx, lse);
}

// thread -> 16 dims of a K row and of a V row: index ((s * nh + h) * 4 + sub) of record blockIdx.y.  The 4 lanes of a
// row are neighbours in one wave and run the same trips (the total and the stride are multiples of 4).
__global__ void __launch_bounds__(256) kv_cache_fill_fp8_kernel(const bf16_t* __restrict__ qkv,
                                                                const int* __restrict__ lens0,
                                                                uint8_t* __restrict__ kcache,
                                                                uint8_t* __restrict__ vcache,
                                                                float* __restrict__ kscale, float* __restrict__ vscale,
                                                                int S0, int nh, int S_max) {
  const int b = blockIdx.y, H = nh * 64;
  int n = lens0[b];
  n = n < S0 ? n : S0;
  n = n < S_max ? n : S_max;
  const long long total = (long long)n * nh * 4;  // (n <= 0: nothing)
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int sub = (int)(i & 3), h = (int)((i >> 2) % nh), s = (int)((i >> 2) / nh);
    const bf16_t* src = qkv + ((long long)b * S0 + s) * 3 * H + H + h * 64 + sub * 16;
    float kf[16], vf[16], sk, sv;
    load16_bf16(src, kf);
    load16_bf16(src + H, vf);
    const u32x4v kq = quantize16(kf, sk), vq = quantize16(vf, sv);
    const long long row = ((long long)b * nh + h) * S_max + s;
    *reinterpret_cast<u32x4v*>(kcache + row * 64 + sub * 16) = kq;
    *reinterpret_cast<u32x4v*>(vcache + row * 64 + sub * 16) = vq;
    if (sub == 0) {
      kscale[row] = sk;
      vscale[row] = sv;
    }
  }
}
}  // namespace

void attn_decode_fp8(const bf16_t* qkv1, const int* lens0, int t, int max_len, uint8_t* kcache, uint8_t* vcache,
                     float* kscale, float* vscale, float* ws, int nsplit, bf16_t* ctx, float* lse, int B, int nh,
                     int S_max, int window, hipStream_t st) {
  if (B <= 0 || nh <= 0) return;
  if (!attn_decode_supported(64, S_max) || nsplit < 1 || nsplit > kMaxSplits || (nsplit > 1 && !ws))
    throw std::runtime_error("dtg: attn_decode: 1 <= S_max <= 2^30, 1 <= nsplit <= 1024 and a workspace for nsplit > 1");
  const int chunks = max_chunks(max_len < 0 ? 0 : max_len, window);
  const int cps = (chunks + nsplit - 1) / nsplit;
  hipLaunchKernelGGL(attn_decode_fp8_kernel, dim3(B * nh, nsplit), dim3(64 * kNW), 0, st, qkv1, lens0, t, kcache,
                     vcache, kscale, vscale, ws, ctx, lse, nh, S_max, window, cps, kLog2e * 0.125f);
  DTG_LAUNCH_CHECK();
  if (nsplit > 1) attn_decode_combine(ws, ctx, lse, B, nh, nsplit, st);
}

void kv_cache_fill_fp8(const bf16_t* qkv, const int* lens0, uint8_t* kcache, uint8_t* vcache, float* kscale,
                       float* vscale, int B, int S0, int nh, int S_max, hipStream_t st) {
  if (B <= 0 || S0 <= 0 || nh <= 0) return;
  const int rows = S0 < S_max ? S0 : S_max;
  hipLaunchKernelGGL(kv_cache_fill_fp8_kernel, dim3(grid_for((long long)rows * nh * 4, 256, 1024), B), dim3(256), 0, st,
                     qkv, lens0, kcache, vcache, kscale, vscale, S0, nh, S_max);
  DTG_LAUNCH_CHECK();
}

}  // namespace dtg
