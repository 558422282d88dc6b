// Device helpers shared by the fused attention kernels: attention.hip (padded rows) and attention_packed.hip
// (packed rows addressed through cu).  Fragment conventions as in dtg/mfma_gemm.cuh.
#pragma once
#include "dtg/common.h"
#include "dtg/mfma_gemm.cuh"

namespace dtg {
namespace attn {
using namespace gemm;

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
// Attention-probability dropout: ONE hash per pair of adjacent keys.  Element idx (= ((b*nh + h)*S + q)*S + key)
// is kept iff the low (even idx) / high (odd idx) 16 bits of fmix32((idx >> 1) * golden + seed) are >= th16 =
// floor(p * 2^16): half the hashes of a per-element draw, and the kernels hold 4 consecutive keys per lane.
__device__ __forceinline__ uint32_t pair_hash(uint32_t seed, uint32_t pidx) { return fmix32(pidx * 0x9E3779B1u + seed); }
__device__ __forceinline__ bool keep_attn(uint32_t seed, uint32_t idx, uint32_t th16) {
  const uint32_t h = pair_hash(seed, idx >> 1);
  return ((idx & 1u) ? (h >> 16) : (h & 0xffffu)) >= th16;
}
// keep flags of 4 consecutive keys starting at an even idx
__device__ __forceinline__ void keep4_attn(uint32_t seed, uint32_t idx0, uint32_t th16, bool (&k)[4]) {
  const uint32_t h0 = pair_hash(seed, idx0 >> 1), h1 = pair_hash(seed, (idx0 >> 1) + 1u);
  k[0] = (h0 & 0xffffu) >= th16;
  k[1] = (h0 >> 16) >= th16;
  k[2] = (h1 & 0xffffu) >= th16;
  k[3] = (h1 >> 16) >= th16;
}

// 16 B of a KC row straight from global memory (A/B fragment of a [rows][64] operand)
__device__ __forceinline__ v8bf gfrag(const bf16_t* base, long long ld, int row0, int ks, int lane) {
  const bf16_t* p = base + (long long)(row0 + (lane & 15)) * ld + ks * 32 + 8 * (lane >> 4);
  return *reinterpret_cast<const v8bf*>(p);
}
// the same of an operand that has only `rows` rows (rows >= 1): a row at or beyond them reads the last one
__device__ __forceinline__ v8bf gfrag_clamp(const bf16_t* base, long long ld, int row0, int rows, int ks, int lane) {
  const int r = row0 + (lane & 15);
  const bf16_t* p = base + (long long)(r < rows ? r : rows - 1) * ld + ks * 32 + 8 * (lane >> 4);
  return *reinterpret_cast<const v8bf*>(p);
}

// byte offset of element (row, k) in a [rows][64] bf16 KC tile with the frag_kc swizzle
__device__ __forceinline__ int kc_off(int row, int k) { return row * 128 + ((((k >> 3) ^ (row & 7))) << 4) + (k & 7) * 2; }

// B fragment X_B[n][k] = T[k][n] of a KC image T [rows = k][64 cols = n] (frag_kc's swizzle): the
// MC-orientation read of a tile that was staged row-wise (ds_read_b64_tr_b16, 4 rows x 4 cols per lane
// address; the chunk XOR moves whole 16-B chunks, so each 8-byte half stays contiguous)
__device__ __forceinline__ v8bf frag_tr_kc(const lds_char* t, int n0, int ks, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int kA = ks * 32 + 8 * g + q, kB = kA + 4;
  const int ch = (n0 + 4 * p) >> 3, sub = (p & 1) * 8;
  const lds_char* a = t + kA * 128 + ((ch ^ (kA & 7)) << 4) + sub;
  const lds_char* b = t + kB * 128 + ((ch ^ (kB & 7)) << 4) + sub;
  const v4bf lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4bf*)(a));
  const v4bf hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4bf*)(b));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2v;
// 4 bf16 (8 bytes) into LDS
__device__ __forceinline__ void st4_bf16(lds_char* p, const float (&v)[4]) {
  u32x2v w;
  w.x = pack_bf2(v[0], v[1]);
  w.y = pack_bf2(v[2], v[3]);
  *reinterpret_cast<__attribute__((address_space(3))) u32x2v*>(p) = w;
}

__device__ __forceinline__ void st_bf16(lds_char* base, int off, float v) {
  *reinterpret_cast<__attribute__((address_space(3))) bf16_t*>(base + off) = f2bf(v);
}

__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Column sums of a wave's 16 C-layout rows x 64 columns (v * scale): the lane's 4 rows, then the 4 lane groups
// that share a column (xor 16, 32).  Lanes 0-15 hold columns j * 16 + lane.
__device__ __forceinline__ void colsum16(const f32x4 (&v)[4], float scale, float (&s)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float t = (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    s[j] = t * scale;
  }
}

// rows [row0, row0+16) x 64 bf16 of a wave's C-layout accumulators -> global (16-B stores) via a
// 2 KB per-wave LDS staging area
__device__ __forceinline__ void store_rows16(lds_char* stg, const f32x4 (&v)[4], float scale, bf16_t* g, long long ldg,
                                             int lane) {
  const int rbase = (lane >> 4) * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) st_bf16(stg, (rbase + r) * 128 + (j * 16 + (lane & 15)) * 2, v[j][r] * scale);
  lds_fence();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + 64 * i, row = c >> 3, ch = c & 7;
    const v8bf x = *reinterpret_cast<const lds_v8bf*>(stg + row * 128 + ch * 16);
    *reinterpret_cast<v8bf*>(g + row * ldg + ch * 8) = x;
  }
  lds_fence();
}
// the same, storing only the first `rows` of the 16 (rows <= 0: none); a form of its own, so that the padded
// kernels' stores stay unpredicated
__device__ __forceinline__ void store_rows16_n(lds_char* stg, const f32x4 (&v)[4], float scale, bf16_t* g,
                                               long long ldg, int lane, int rows) {
  const int rbase = (lane >> 4) * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) st_bf16(stg, (rbase + r) * 128 + (j * 16 + (lane & 15)) * 2, v[j][r] * scale);
  lds_fence();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + 64 * i, row = c >> 3, ch = c & 7;
    const v8bf x = *reinterpret_cast<const lds_v8bf*>(stg + row * 128 + ch * 16);
    if (row < rows) *reinterpret_cast<v8bf*>(g + row * ldg + ch * 8) = x;
  }
  lds_fence();
}

// 16-bit threshold of the pair-hash dropout (keep_attn); 0 = no dropout
inline uint32_t drop_th(float p) {
  if (p <= 0.f) return 0u;
  const double t = (double)p * 65536.0;
  return t >= 65535.0 ? 0xffffu : (t < 1.0 ? 1u : (uint32_t)t);
}

}  // namespace attn
}  // namespace dtg
