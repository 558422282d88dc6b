// The pieces the causal fused attention kernels are built from: attention_causal.hip (padded rows),
// attention_causal_packed.hip (packed rows, no mask operand) and attention_window.hip (sliding window).  Each of the
// nine kernels keeps its own frame (chunk-loop bounds, ring staging, record geometry, block mapping); the chunk bodies
// and the epilogues that do not depend on the frame are here, once.  The template parameters say what a kernel does:
//
//   kEdges    0: every key of the chunk is visible to every query of the wave (the unmasked body);
//             1: the chunk holds the wave's diagonal, key <= query decides (causal, packed);
//             2: the chunk is the diagonal one or the window's far edge, W rows away, where the complement of the
//                diagonal predicate decides; which of the two is a wave-uniform argument (window);
//   kKeyMask  an additive key-mask operand exists (causal, window); without one the term is the constant the padded
//             kernels would have read for a real key, so the packed results carry the padded bits;
//   kRows     only the first `rows` of a wave's 16 rows exist (packed): the others are clamped copies, never stored.
//
// Registers.  All nine kernels are built for 4 waves per SIMD (amdgpu_waves_per_eu(4, 4)): 128 VGPRs, and they sit
// at 124 .. 128 without scratch.  A forward or dQ kernel holds two instances of its body (kEdges = 0 and one other)
// behind a wave-uniform branch; a third does not fit, which is why the window's two edges share one instance.  dKV
// holds one instance with the compares in a wave-uniform branch of their own.
#pragma once
#include "dtg/attn_common.cuh"

namespace dtg {
namespace attn {

constexpr int kNW = 8;                 // waves per workgroup
constexpr int kBlk = 16 * kNW;         // queries (forward, dQ) / keys (dKV) per workgroup
constexpr int kTile = 8192;            // one [64][64] bf16 tile
constexpr int kSlot = 2 * kTile;       // a ring slot: two tiles
constexpr int kRing = 2;
constexpr int kVec = 512;              // per-slot fp32 values travelling with a chunk (mask, or LSE | D)
constexpr int kScr = 2048;             // per-wave scratch
constexpr size_t kLds = (size_t)kRing * (kSlot + kVec) + kNW * kScr;  // 49.0 KiB: three workgroups per CU
constexpr float kLog2e = 1.4426950408889634f;

typedef const __attribute__((address_space(3))) f32x4 lds_f32x4;
typedef const __attribute__((address_space(3))) bf16_t lds_bf16;
typedef const __attribute__((address_space(3))) u32x2v lds_u32x2;

// Is position x + xl visible from position t of the same chunk (x: what varies in the caller's loops, xl: the lane's
// part)?  One edge: x + xl <= t.  Two edges: that is (x + xl - t - 1) < 0, and the far edge's x + xl > t is the
// complement, so the inversion is an xor with a wave-uniform word (inv = 0 / -1) in the VALU; a compare inverted in
// the lane masks keeps 16 loop-invariant masks alive in SGPRs, which then spill.  The loop-invariant xl - t - 1 is
// kept together: associated as (x + xl) - t - 1 the window's forward spills two VGPRs.
template <int kEdges>
__device__ __forceinline__ bool edge_visible(int x, int xl, int t, int inv) {
  if constexpr (kEdges == 2) return ((x + (xl - t - 1)) ^ inv) < 0;
  return x + xl <= t;
}

// One key chunk of the forward for a wave's 16 queries; lane (qi, g) holds query q0 + qi against keys j * 16 + 4g +
// [0, 4) of each 16-key block j.  far (kEdges = 2, wave-uniform): the chunk is the window's lower edge.
//   An invisible key is EXCLUDED by a select, whatever K held: out of the running max, P = exp(-inf - finite) = 0.
// With one edge every chunk a wave computes holds a visible key of each of its rows (its first key is <= q0), so the
// chunk maximum is finite.  On the window's lower edge row 15 of jd = 3 sees no key, and with m still -inf the
// subtrahend is 0 instead: alpha = exp(-inf) = 0 on l = o = 0, P = 0, and m stays -inf for the next chunk.
//   The second product (O^T += V^T P^T) would still multiply an excluded element (0 * V) inside an MFMA, which is
// exact only while V is finite.  So on a masked chunk the V^T fragments of the 16-key blocks that are not wholly
// visible are replaced by zeros, and the partial block jd is accumulated on the VALU under the predicate: an excluded
// key's K and V never reach a visible query's out or LSE, whatever their bits.
template <int kEdges, bool kKeyMask>
__device__ __forceinline__ void fwd_chunk(const lds_char* Kt, const lds_char* Vt, const lds_float* Mc, lds_char* scr,
                                          const v8bf (&qa)[2], float& m, float& l, f32x4 (&o)[4], int kc, int q0,
                                          int lane, float scale, uint32_t th, float dscale, uint32_t seed,
                                          uint32_t prow, bool far) {
  const int qi = lane & 15, g = lane >> 4;
  // (masked) the partial 16-key block: W % 64 == 0 puts it at the same in-chunk index on both edges
  const int jd = kEdges == 2 ? (q0 & 63) >> 4 : (q0 - kc * 64) >> 4;
  const int inv = far ? -1 : 0;
  f32x4 s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_kc(Kt, j * 16, ks, lane), qa[ks], s[j], 0, 0, 0);
  }
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 madd = {0.f, 0.f, 0.f, 0.f};  // (no operand) a real key's term: the rounding stays the padded kernels'
    if constexpr (kKeyMask) madd = *reinterpret_cast<lds_f32x4*>(Mc + j * 16 + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = fmaf(s[j][r], scale, madd[r]);
      s[j][r] = (!kEdges || edge_visible<kEdges>(j * 16 + r, 4 * g, jd * 16 + qi, inv)) ? v : -INFINITY;
      mx = fmaxf(mx, s[j][r]);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float mn = fmaxf(m, mx);
  const float mref = (kEdges == 2 && mn == -INFINITY) ? 0.f : mn;  // the row that sees no key yet
  const float alpha = __expf(m - mref);
  m = mn;
  float rs = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key0 = kc * 64 + j * 16 + 4 * g;
    float pd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pd[r] = __expf(s[j][r] - mref);
      rs += pd[r];
    }
    if (th) {
      bool kp[4];
      keep4_pair(seed, prow + (uint32_t)(key0 >> 1), th, kp);
#pragma unroll
      for (int r = 0; r < 4; ++r) pd[r] = kp[r] ? pd[r] * dscale : 0.f;
    }
    st4_bf16(scr + kc_off(qi, j * 16 + 4 * g), pd);  // P [16 q][64 keys] KC
  }
  l = l * alpha + rs;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[j][r] *= alpha;
  lds_fence();
  const v8bf pb0 = frag_kc(scr, 0, 0, lane), pb1 = frag_kc(scr, 0, 1, lane);  // X_B[q][key]
  // the lane's 8 keys of a V^T fragment lie in 16-key block 2 ks + (g >> 1): on a masked chunk only the blocks wholly
  // visible go through the MFMA (diagonal: below jd; far edge: above jd)
  const v8bf zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const int b0 = g >> 1, b1 = 2 + (g >> 1);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v8bf v0 = frag_mc<64>(Vt, j * 16, 0, lane), v1 = frag_mc<64>(Vt, j * 16, 1, lane);
    if constexpr (kEdges == 1) {
      if (b0 >= jd) v0 = zero;
      if (b1 >= jd) v1 = zero;
    } else if constexpr (kEdges == 2) {
      if (b0 == jd || (b0 > jd) != far) v0 = zero;
      if (b1 == jd || (b1 > jd) != far) v1 = zero;
    }
    o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, pb0, o[j], 0, 0, 0);
    o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v1, pb1, o[j], 0, 0, 0);
  }
  if constexpr (kEdges != 0) {
    // the partial 16 x 16 block: O^T[d][q] += V[key][d] * P[q][key] for the visible keys only, P as the MFMA would
    // read it (bf16 out of the scratch); the lane's d are j * 16 + 4g + [0, 4), 8 bytes of V's MC row
#pragma unroll 2
    for (int kk = 0; kk < 16; ++kk) {
      const int kl = jd * 16 + kk;
      const float pv = bf2f(*reinterpret_cast<lds_bf16*>(scr + kc_off(qi, kl)));
      const lds_char* vrow = Vt + kl * 128 + (g & 1) * 8;
      const int sw = mc_swz<8>(kl);
      if (edge_visible<kEdges>(kk, 0, qi, inv)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u32x2v w = *reinterpret_cast<lds_u32x2*>(vrow + (((2 * j + (g >> 1)) ^ sw) << 4));
          o[j][0] = fmaf(pv, __uint_as_float(w.x << 16), o[j][0]);
          o[j][1] = fmaf(pv, __uint_as_float(w.x & 0xffff0000u), o[j][1]);
          o[j][2] = fmaf(pv, __uint_as_float(w.y << 16), o[j][2]);
          o[j][3] = fmaf(pv, __uint_as_float(w.y & 0xffff0000u), o[j][3]);
        }
      }
    }
  }
}

// The forward's epilogue for an active wave: normalise, out rows q0 .. q0+15 through the scratch (16-B stores) and
// the LSE.  orow / lrow: the index of the wave's first row in out (rows of H, the head's 64 columns at col) and in
// lse.  Unpredicated: all 16 rows exist.  The packed forward keeps its row-guarded copy in its file -- behind this
// call, with the guards as a template parameter, its main loop was allocated differently (128 VGPRs for 127) and
// measured 0.2 .. 1.2 % slower.
__device__ __forceinline__ void fwd_store(lds_char* scr, const f32x4 (&o)[4], float m, float l, bf16_t* out,
                                          long long orow, int H, int col, float* lse, long long lrow, int lane) {
  const int qi = lane & 15, g = lane >> 4;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float il = 1.f / l;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v[4] = {o[j][0] * il, o[j][1] * il, o[j][2] * il, o[j][3] * il};
    st4_bf16(scr + qi * 128 + (((2 * j + (g >> 1)) ^ (qi & 7)) << 4) + (g & 1) * 8, v);
  }
  if (g == 0) lse[lrow + qi] = m + __logf(l);
  lds_fence();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + 64 * i;  // 128 chunks of 16 B: row c/8, chunk c%8
    const int row = c >> 3, ch = c & 7;
    const v8bf v = *reinterpret_cast<const lds_v8bf*>(scr + row * 128 + ((ch ^ (row & 7)) << 4));
    *reinterpret_cast<v8bf*>(out + (orow + row) * H + col + ch * 8) = v;
  }
}

// One key chunk of dQ for a wave's 16 queries (kEdges, far as in fwd_chunk).  The backward multiplies the exact
// zeros of an excluded element's dS by operands it takes to be finite.
template <int kEdges, bool kKeyMask>
__device__ __forceinline__ void dq_chunk(const lds_char* kt, const lds_char* vt, const lds_float* Mc, lds_char* scr,
                                         const v8bf (&qa)[2], const v8bf (&da)[2], f32x4 (&dq)[4], float lq, float dd,
                                         int kc, int q0, int lane, float sl2, uint32_t th, float dscale,
                                         uint32_t seed, uint32_t prow, bool far) {
  const int qi = lane & 15, g = lane >> 4;
  // (masked) the query's position in its diagonal chunk
  const int t = kEdges == 2 ? (q0 & 63) + qi : q0 + qi - kc * 64;
  const int inv = far ? -1 : 0;
  f32x4 s[4], dp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s[j] = dp[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_kc(kt, j * 16, ks, lane), qa[ks], s[j], 0, 0, 0);
      dp[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_kc(vt, j * 16, ks, lane), da[ks], dp[j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key0 = kc * 64 + j * 16 + 4 * g;
    f32x4 madd;
    if constexpr (kKeyMask) madd = *reinterpret_cast<lds_f32x4*>(Mc + j * 16 + 4 * g);
    bool kp[4] = {true, true, true, true};
    if (th) keep4_pair(seed, prow + (uint32_t)(key0 >> 1), th, kp);
    float dsv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __builtin_amdgcn_exp2f(fmaf(s[j][r], sl2, kKeyMask ? madd[r] - lq : -lq));
      float dpv = dp[j][r];
      if (th) dpv = kp[r] ? dpv * dscale : 0.f;
      dsv[r] = (!kEdges || edge_visible<kEdges>(j * 16 + r, 4 * g, t, inv)) ? p * (dpv - dd) : 0.f;
    }
    st4_bf16(scr + kc_off(qi, j * 16 + 4 * g), dsv);  // dS [16 q][64 keys] KC
  }
  lds_fence();
  const v8bf a0 = frag_kc(scr, 0, 0, lane), a1 = frag_kc(scr, 0, 1, lane);  // X_A[q][key]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    dq[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, frag_tr_kc(kt, j * 16, 0, lane), dq[j], 0, 0, 0);
    dq[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, frag_tr_kc(kt, j * 16, 1, lane), dq[j], 0, 0, 0);
  }
}

// dQ's prologue for an active wave: D = rowsum(dO * O) of its 16 rows (4 lanes per row, 16 d each), written to dw
// for dKV; the lane's query's D and LSE * log2(e) are returned.  dOg / Og are the head's columns of the record's
// row 0, v0 the index of its first LSE / D value.  kRows: a row at or beyond `rows` reads the last one and writes
// nothing.
template <bool kRows>
__device__ __forceinline__ void dq_row_terms(const bf16_t* dOg, const bf16_t* Og, const float* lse, float* dwork,
                                             long long v0, int H, int q0, int rows, int lane, float& dd, float& lq) {
  const int qi = lane & 15, row = lane >> 2, part = lane & 3;
  const int qd = (!kRows || q0 + row < rows) ? q0 + row : rows - 1;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float a[8], bb[8];
    load8_bf16(dOg + (long long)qd * H + part * 16 + c * 8, a);
    load8_bf16(Og + (long long)qd * H + part * 16 + c * 8, bb);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += a[k] * bb[k];
  }
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  if (part == 0 && (!kRows || q0 + row < rows)) dwork[v0 + q0 + row] = acc;
  dd = __shfl(acc, qi * 4, 64);
  lq = lse[v0 + ((!kRows || q0 + qi < rows) ? q0 + qi : rows - 1)] * kLog2e;
}

// dQ's bias gradient: per-wave column sums of dq * scale, combined over the workgroup in the ring (idle after the
// chunk loop's last barrier), one atomic per column.  Every wave of the workgroup calls it.
__device__ __forceinline__ void dq_dbias(lds_char* ring, const f32x4 (&dq)[4], float scale, bool active, float* dbias,
                                         int H, int h, int wave, int lane, int tid) {
  lds_float* bsum = reinterpret_cast<lds_float*>(ring);
  float sq[4] = {0.f, 0.f, 0.f, 0.f};
  if (active) colsum16(dq, scale, sq);
  if (lane < 16)
#pragma unroll
    for (int j = 0; j < 4; ++j) bsum[wave * 64 + j * 16 + lane] = sq[j];
  dbias_reduce<64, kNW>(bsum, dbias, 0, H, h, tid);
}

// One query chunk of dKV for a wave's 16 keys kb .. kb+15.  diag: the chunk straddles the wave's diagonal; far: it
// holds the other limit of a key's queries -- the window's upper edge, W queries later (kTwoEdge), or queries >= n
// (kRows).  Both wave-uniform; one body, the compares in a branch of their own, which keeps the kernel within 128
// VGPRs.  A 32-query half with no visible pair is skipped: wholly before the wave's first key on the diagonal chunk,
// wholly at or beyond its last key + W on the upper edge.  msl: the keys' mask terms * log2(e) (kKeyMask).
template <bool kTwoEdge, bool kKeyMask, bool kRows>
__device__ __forceinline__ void dkv_chunk(const lds_char* Qt, const lds_char* dOt, const lds_float* Ls,
                                          const lds_float* Ds, lds_char* scp, lds_char* scs, v8bf ka0, v8bf ka1,
                                          v8bf va0, v8bf va1, const float (&msl)[4], f32x4 (&dk)[4], f32x4 (&dv)[4],
                                          int c, int kb, int n, int bh, int S, int lane, float sl2, uint32_t th,
                                          float dscale, uint32_t seed, bool diag, bool far) {
  static_assert(!(kTwoEdge && kRows), "a row limit on the two-edged body is not built");
  const int rbase = (lane >> 4) * 4;
  const int t0 = kb & 63;  // (kTwoEdge) the first key's position in its diagonal chunk
  const bool masked = diag || far, up = !diag;
  const int inv = up ? -1 : 0;
#pragma unroll
  for (int kq = 0; kq < 2; ++kq) {  // 32-query halves of the chunk
    if (kTwoEdge ? masked && (up ? kq * 32 >= t0 + 15 : kq * 32 + 31 < t0) : diag && c * 64 + kq * 32 + 31 < kb)
      continue;  // wave-uniform
    f32x4 st[2], dpt[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      // B fragments (16 queries x 32 d) read row-wise out of the MC tiles (undoing their swizzle)
      const int qrow = kq * 32 + ni * 16 + (lane & 15), cb = lane >> 4;
      const int sw = mc_swz<8>(qrow);
      const lds_char* qt = Qt + qrow * 128;
      const lds_char* dt = dOt + qrow * 128;
      const v8bf qb0 = *reinterpret_cast<const lds_v8bf*>(qt + ((cb ^ sw) << 4));
      const v8bf qb1 = *reinterpret_cast<const lds_v8bf*>(qt + (((4 + cb) ^ sw) << 4));
      const v8bf db0 = *reinterpret_cast<const lds_v8bf*>(dt + ((cb ^ sw) << 4));
      const v8bf db1 = *reinterpret_cast<const lds_v8bf*>(dt + (((4 + cb) ^ sw) << 4));
      f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
      z = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka0, qb0, z, 0, 0, 0);
      st[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka1, qb1, z, 0, 0, 0);
      z = f32x4{0.f, 0.f, 0.f, 0.f};
      z = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va0, db0, z, 0, 0, 0);
      dpt[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va1, db1, z, 0, 0, 0);
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int ql = ni * 16 + (lane & 15), qs = kq * 32 + ql, q = c * 64 + qs;
      const float lq = Ls[qs], dq = Ds[qs];
      const uint32_t pidx =
          ((uint32_t)bh * (uint32_t)S + (uint32_t)q) * (uint32_t)(S >> 1) + (uint32_t)((kb + rbase) >> 1);
      float pd[4], dsv[4];
      bool kp[4] = {true, true, true, true};
      if (th) keep4_pair(seed, pidx, th, kp);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(st[ni][r], sl2, kKeyMask ? msl[r] - lq : -lq));
        float pv = p, dp = dpt[ni][r];
        if (th) {
          pv = kp[r] ? p * dscale : 0.f;
          dp = kp[r] ? dp * dscale : 0.f;
        }
        pd[r] = pv;
        dsv[r] = p * (dp - dq);
      }
      if (masked) {
        // one edge: query >= key and (kRows) query < n; off the diagonal the first always holds (q >= kb + 15).
        // Two edges: the key's in-chunk position <= the query's is visible on the diagonal chunk, invisible on the
        // upper edge (the xor: see edge_visible)
        const int lim = (!kRows || q < n) ? q - kb - rbase : -1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool vis = kTwoEdge ? edge_visible<2>(r, t0 + rbase, qs, inv) : r <= lim;
          pd[r] = vis ? pd[r] : 0.f;
          dsv[r] = vis ? dsv[r] : 0.f;
        }
      }
      st4_bf16(scp + ql * 32 + rbase * 2, pd);
      st4_bf16(scs + ql * 32 + rbase * 2, dsv);
    }
    lds_fence();
    const v8bf pa = frag_mc<16>(scp, 0, 0, lane);  // dropout(P)^T [16 keys][32 q]
    const v8bf sa = frag_mc<16>(scs, 0, 0, lane);  // dS^T [16 keys][32 q]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dv[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, frag_mc<64>(dOt, j * 16, kq, lane), dv[j], 0, 0, 0);
      dk[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sa, frag_mc<64>(Qt, j * 16, kq, lane), dk[j], 0, 0, 0);
    }
    lds_fence();  // scratches rewritten by the next half
  }
}

// dKV's bias gradient (see dq_dbias): column sums of dk * scale and of dv
__device__ __forceinline__ void dkv_dbias(lds_char* ring, const f32x4 (&dk)[4], const f32x4 (&dv)[4], float scale,
                                          bool has_keys, float* dbias, int H, int h, int wave, int lane, int tid) {
  lds_float* bsum = reinterpret_cast<lds_float*>(ring);
  float sk[4] = {0.f, 0.f, 0.f, 0.f}, sv[4] = {0.f, 0.f, 0.f, 0.f};
  if (has_keys) {
    colsum16(dk, scale, sk);
    colsum16(dv, 1.f, sv);
  }
  if (lane < 16)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bsum[wave * 128 + j * 16 + lane] = sk[j];
      bsum[wave * 128 + 64 + j * 16 + lane] = sv[j];
    }
  dbias_reduce<128, kNW>(bsum, dbias, 1, H, h, tid);
}

// dropout threshold and 1 / (1 - p) of a launch
struct DropArgs {
  uint32_t th;
  float dscale;
};
inline DropArgs drop_args(float p) { return {drop_th(p), p > 0.f ? 1.f / (1.f - p) : 1.f}; }

}  // namespace attn
}  // namespace dtg
