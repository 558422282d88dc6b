// Causal (lower-triangular) fused attention on PACKED token rows, forward and backward, for 64 <= S <= kStreamMaxS,
// S % 64 == 0: head dim 64, bf16, pair-hash dropout, NO mask operand.  The addressing is attention_stream_packed.hip's
// (qkv [T_alloc, 3H], ctx [T_alloc, H], dQKV [T_alloc, 3H] and the fp32 LSE / D rows [nh, T_alloc] through cu;
// record_rows: no row outside [0, T_alloc) is read or written; the last record's block-0 workgroups zero the rows
// cu[B] .. T_alloc - 1 before they test n), the triangle schedule is attention_causal.hip's, over the record's own
// geometry.  With (base, n) of record b and nb = ceil(n / 128) blocks of 128 rows:
//
//   forward, dQ (a wave owns queries q0 .. q0+15 of query block y):
//     a workgroup with blockIdx.y >= nb leaves before its first barrier; the others map blockIdx.y onto y = nb - 1 -
//     blockIdx.y (heavy first: the record's last block has the most chunks) and visit key chunks 0 .. min(ceil(n/64),
//     2y + 2) - 1.  A wave skips the arithmetic of a chunk that starts beyond its last query, runs the plain body on a
//     chunk wholly at or below its first query, and pays the compare key <= q on its one diagonal chunk, behind a
//     wave-uniform branch (two instances of the chunk body).
//   dKV (a wave owns keys kb .. kb+15 of key block y = blockIdx.y: the first block is the heaviest):
//     query chunks 2y .. ceil(n/64) - 1, starting in ring slot 0 (2y is even); a wave skips a chunk that ends below its
//     first key and pays the compare on the chunk that straddles the diagonal.
//   8 waves, 64-row chunks through the 2-slot LDS ring, chunk c + 1's LDS-DMA issued before chunk c's MFMAs, one
//   barrier per chunk; a wave whose 16 rows start at or beyond n stays in the loop for the staging and the barriers.
//
// Why there is no mask.  The padded causal kernel, fed the re-padded operands and the length as additive mask, gives a
// real query q < n the keys <= q, and every one of those is a real key (key <= q < n): its mask term is + 0.0f, which
// changes no score (fmaf(s, scale, 0.f) is kept here so that the rounding is the same), and a key > q is EXCLUDED
// there as here -- out of the running max and the row sum, P = 0 exactly.  So no -10000 ever reaches a real row of
// the padded kernel, and the length only decides which rows exist:
//   * chunks at or beyond ceil(n/64) are computed by no wave that owns a real row in forward / dQ (a wave computes
//     chunk kc only if 64 kc <= q0 < n); in dKV they hold padding queries only, whose dO = 0 and hence D = 0, dS = 0
//     and dropout(P)^T dO = 0 in the padded kernel: exact zeros added to dK / dV;
//   * a query >= n inside the last chunk of dKV is the same exact zero: dropout(P) and dS are forced to 0 here;
//   * rows of a wave's 16 at or beyond n are computed on clamped copies of row n - 1 and never stored; softmax rows
//     are independent, so they do not touch the real ones; dQ zeroes them before the dbias column sums; in dKV a key
//     >= n is seen by queries >= n only, which are forced, so those accumulator rows are exactly zero.
// On rows < T, ctx, LSE and dQKV therefore carry attn_causal_*'s bits.
//
// Rows at or beyond n are never loaded: KC tiles and register fragments read row n - 1 instead (DenseKC<true>,
// gfrag_clamp), MC tiles the zero page (DenseMC<true>), the LSE / D values that travel with a dKV chunk are clamped
// to the record's rows, every 16-row store is guarded by row.  The forward is NaN-proof against the keys a query must
// not see, as in attention_causal.hip: on the diagonal chunk the V fragments of the 16-key blocks at and above the
// wave's diagonal block are replaced by zeros and the diagonal 16 x 16 block is accumulated on the VALU under key <=
// q, so an excluded key's K and V never reach a visible query's out or LSE whatever their bits -- and no row of
// another record is loaded at all.
//
// Dropout: the pair index stays in PADDED coordinates, ((b*nh + h)*S + q) * (S/2) + key/2 in wrapping uint32.
// D = rowsum(dO * O): fp32 workspace [nh, T_alloc]; the dQ launch writes the rows below n, the dKV launch reads them,
// so the launch order is dQ, then dKV.  dbias (optional): per-wave column sums, combined over the workgroup in the
// idle ring, one atomic per column and workgroup.  No atomics on dqkv.
#include "dtg/common.h"
#include "dtg/kernels.h"
#include "dtg/attn_common.cuh"
#include "dtg/mfma_gemm.cuh"

namespace dtg {
using namespace gemm;
using namespace attn;

namespace {
constexpr int kNW = 8;                 // waves per workgroup
constexpr int kBlk = 16 * kNW;         // queries (forward, dQ) / keys (dKV) per workgroup
constexpr int kTile = 8192;            // one [64][64] bf16 tile
constexpr int kSlot = 2 * kTile;       // a ring slot: two tiles
constexpr int kRing = 2;
constexpr int kVec = 512;              // dKV: per-slot fp32 values travelling with a chunk (LSE | D)
constexpr int kScr = 2048;             // per-wave scratch
constexpr size_t kLdsQ = (size_t)kRing * kSlot + kNW * kScr;            // forward, dQ: 48.0 KiB
constexpr size_t kLdsKV = (size_t)kRing * (kSlot + kVec) + kNW * kScr;  // dKV: 49.0 KiB; three workgroups per CU
constexpr float kLog2e = 1.4426950408889634f;

typedef const __attribute__((address_space(3))) bf16_t lds_bf16;
typedef const __attribute__((address_space(3))) u32x2v lds_u32x2;

// One key chunk of the forward for a wave's 16 queries.  kDiag: the chunk holds the wave's diagonal (q0 - 64 kc in
// {0, 16, 32, 48}); lane (qi, g) holds query q0 + qi against keys j * 16 + 4g + [0, 4) of each 16-key block j.
template <bool kDiag>
__device__ __forceinline__ void fwd_chunk(const lds_char* Kt, const lds_char* Vt, lds_char* scr, const v8bf (&qa)[2],
                                          float& m, float& l, f32x4 (&o)[4], int kc, int q0, int lane, float scale,
                                          uint32_t th, float dscale, uint32_t seed, uint32_t prow) {
  const int qi = lane & 15, g = lane >> 4;
  const int jd = (q0 - kc * 64) >> 4;  // (kDiag) the 16-key block on the diagonal
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
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = fmaf(s[j][r], scale, 0.f);  // the padded kernel's rounding with a real key's mask term
      // excluded: out of the max here, and P = exp(-inf - finite) = 0 below (a select, whatever K held)
      s[j][r] = (!kDiag || j * 16 + 4 * g + r <= jd * 16 + qi) ? v : -INFINITY;
      mx = fmaxf(mx, s[j][r]);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  // every chunk a wave computes holds a visible key of each of its rows (its first key is <= q0), so mx is finite
  const float mn = fmaxf(m, mx);
  const float alpha = __expf(m - mn);
  m = mn;
  float rs = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key0 = kc * 64 + j * 16 + 4 * g;
    float pd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pd[r] = __expf(s[j][r] - mn);
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
  // the lane's 8 keys of a V^T fragment lie in 16-key block 2 ks + (g >> 1): on the diagonal chunk only the blocks
  // below the diagonal one go through the MFMA
  const v8bf zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v8bf v0 = frag_mc<64>(Vt, j * 16, 0, lane), v1 = frag_mc<64>(Vt, j * 16, 1, lane);
    if (kDiag) {
      if ((g >> 1) >= jd) v0 = zero;
      if (2 + (g >> 1) >= jd) v1 = zero;
    }
    o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, pb0, o[j], 0, 0, 0);
    o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v1, pb1, o[j], 0, 0, 0);
  }
  if (kDiag) {
    // the diagonal 16 x 16 block: O^T[d][q] += V[key][d] * P[q][key] for key <= q only, P as the MFMA would read it
    // (bf16 out of the scratch); the lane's d are j * 16 + 4g + [0, 4), 8 bytes of V's MC row
#pragma unroll 2
    for (int kk = 0; kk < 16; ++kk) {
      const int kl = jd * 16 + kk;
      const float pv = bf2f(*reinterpret_cast<lds_bf16*>(scr + kc_off(qi, kl)));
      const lds_char* vrow = Vt + kl * 128 + (g & 1) * 8;
      const int sw = mc_swz<8>(kl);
      if (kk <= qi) {
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

// One key chunk of dQ for a wave's 16 queries (kDiag as in fwd_chunk)
template <bool kDiag>
__device__ __forceinline__ void dq_chunk(const lds_char* kt, const lds_char* vt, lds_char* scr, const v8bf (&qa)[2],
                                         const v8bf (&da)[2], f32x4 (&dq)[4], float lq, float dd, int kc, int q0,
                                         int lane, float sl2, uint32_t th, float dscale, uint32_t seed,
                                         uint32_t prow) {
  const int qi = lane & 15, g = lane >> 4;
  const int qrel = q0 + qi - kc * 64;  // (kDiag) the query's position in the chunk
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
    bool kp[4] = {true, true, true, true};
    if (th) keep4_pair(seed, prow + (uint32_t)(key0 >> 1), th, kp);
    float dsv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __builtin_amdgcn_exp2f(fmaf(s[j][r], sl2, -lq));
      float dpv = dp[j][r];
      if (th) dpv = kp[r] ? dpv * dscale : 0.f;
      dsv[r] = (!kDiag || j * 16 + 4 * g + r <= qrel) ? p * (dpv - dd) : 0.f;
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

// One query chunk of dKV for a wave's 16 keys kb .. kb+15.  kDiag: the chunk straddles the diagonal; kEdge: it does,
// or it holds queries >= n (both wave-uniform; one body, the compares in a branch of their own, which keeps the
// kernel within 128 VGPRs).  A 32-query half wholly before the wave's first key is skipped; under kEdge an element
// pays n > q >= key.
__device__ __forceinline__ void dkv_chunk(const lds_char* Qt, const lds_char* dOt, const lds_float* Ls,
                                          const lds_float* Ds, lds_char* scp, lds_char* scs, v8bf ka0, v8bf ka1,
                                          v8bf va0, v8bf va1, f32x4 (&dk)[4], f32x4 (&dv)[4], int c, int kb, int n,
                                          int bh, int S, int lane, float sl2, uint32_t th, float dscale,
                                          uint32_t seed, bool kDiag, bool kEdge) {
  const int rbase = (lane >> 4) * 4;
#pragma unroll
  for (int kq = 0; kq < 2; ++kq) {  // 32-query halves of the chunk
    if (kDiag && c * 64 + kq * 32 + 31 < kb) continue;  // wave-uniform
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
        const float p = __builtin_amdgcn_exp2f(fmaf(st[ni][r], sl2, -lq));
        float pv = p, dp = dpt[ni][r];
        if (th) {
          pv = kp[r] ? p * dscale : 0.f;
          dp = kp[r] ? dp * dscale : 0.f;
        }
        pd[r] = pv;
        dsv[r] = p * (dp - dq);
      }
      if (kEdge) {
        // query >= key and query < n; off the diagonal the first always holds (q >= kb + 15)
        const int lim = q < n ? q - kb - rbase : -1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool vis = r <= lim;
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
}  // namespace

// ---------------------------------------------------------------------------------------------
// Forward: ring slots {K as KC tile | V as MC tile}
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) __launch_bounds__(64 * kNW)
attn_pcausal_fwd_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ cu, bf16_t* __restrict__ out,
                        float* __restrict__ lse, int B, int S, int nh, int T_alloc, float scale, uint32_t th,
                        float dscale, uint32_t seed, int flip) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (b == B - 1 && blockIdx.y == 0) zero_tail(out, H, h * 64, 1, 0, cu, B, T_alloc, tid, 64 * kNW);
  int base, n;
  record_rows(cu, b, S, T_alloc, base, n);
  const int nb = (n + kBlk - 1) / kBlk;  // the record's query blocks
  if ((int)blockIdx.y >= nb) return;     // uniform, before any barrier (n = 0 included)
  const int yb = flip ? nb - 1 - (int)blockIdx.y : (int)blockIdx.y;
  const bf16_t* Qg = qkv + (long long)base * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  lds_char* ring = smem;                                // kRing x {K KC | V MC}
  lds_char* scr = smem + kRing * kSlot + wave * kScr;   // per-wave [16][64] bf16
  const int nkc = min((n + 63) >> 6, 2 * yb + 2);       // the block's last query sees nothing beyond chunk 2 yb + 1
  const DenseKC<true> ks_{Kg, ld, n, 64};               // rows >= n: row n - 1
  const DenseMC<true> vs_{Vg, ld, 64, n};               // rows >= n: the zero page
  const int q0 = yb * kBlk + wave * 16;
  const bool active = q0 < n;  // wave-uniform
  v8bf qa[2];
  if (active) {
    qa[0] = gfrag_clamp(Qg, ld, q0, n, 0, lane);
    qa[1] = gfrag_clamp(Qg, ld, q0, n, 1, lane);
  }
  stage_kc<64, DenseKC<true>, kNW>(ks_, ring, 0, 0, wave, lane);
  stage_mc<64, DenseMC<true>, kNW>(vs_, ring + kTile, 0, 0, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int qi = lane & 15, g = lane >> 4;
  // pair index of (q, key 0) in padded coordinates, wrapping
  const uint32_t prow = ((uint32_t)bh * (uint32_t)S + (uint32_t)(q0 + qi)) * (uint32_t)(S >> 1);
#pragma unroll 1
  for (int kc = 0; kc < nkc; ++kc) {
    const int cur = kc & 1, nxt = cur ^ 1;
    if (kc + 1 < nkc) {
      stage_kc<64, DenseKC<true>, kNW>(ks_, ring + nxt * kSlot, (kc + 1) * 64, 0, wave, lane);
      stage_mc<64, DenseMC<true>, kNW>(vs_, ring + nxt * kSlot + kTile, 0, (kc + 1) * 64, wave, lane);
    }
    if (active && kc * 64 <= q0) {  // (q0 % 16 == 0: the chunk starts at or below the wave's last query)
      const lds_char* Kt = ring + cur * kSlot;
      if (kc * 64 + 63 <= q0)
        fwd_chunk<false>(Kt, Kt + kTile, scr, qa, m, l, o, kc, q0, lane, scale, th, dscale, seed, prow);
      else
        fwd_chunk<true>(Kt, Kt + kTile, scr, qa, m, l, o, kc, q0, lane, scale, th, dscale, seed, prow);
    }
    // chunk kc + 1 has landed and every wave is done with slot cur, which the next iteration refills
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (!active) return;  // (no barrier below this point)
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float il = 1.f / l;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v[4] = {o[j][0] * il, o[j][1] * il, o[j][2] * il, o[j][3] * il};
    st4_bf16(scr + qi * 128 + (((2 * j + (g >> 1)) ^ (qi & 7)) << 4) + (g & 1) * 8, v);
  }
  // queries >= n (clamped copies of row n - 1) stay here
  if (g == 0 && q0 + qi < n) lse[(long long)h * T_alloc + base + q0 + qi] = m + __logf(l);
  lds_fence();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + 64 * i;  // 128 chunks of 16 B: row c/8, chunk c%8
    const int row = c >> 3, ch = c & 7;
    const v8bf v = *reinterpret_cast<const lds_v8bf*>(scr + row * 128 + ((ch ^ (row & 7)) << 4));
    if (q0 + row < n) *reinterpret_cast<v8bf*>(out + ((long long)base + q0 + row) * H + h * 64 + ch * 8) = v;
  }
}

// ---------------------------------------------------------------------------------------------
// dQ: ring slots {K | V}, both KC.  The wave's Q / dO fragments and its O / LSE rows are clamped to row n - 1; D of
// the rows below n is written to the workspace.
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) __launch_bounds__(64 * kNW)
attn_pcausal_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout,
                       const float* __restrict__ lse, const int* __restrict__ cu, bf16_t* __restrict__ dqkv,
                       float* __restrict__ dwork, int B, int S, int nh, int T_alloc, float scale, uint32_t th,
                       float dscale, uint32_t seed, float* __restrict__ dbias, int flip) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (b == B - 1 && blockIdx.y == 0) zero_tail(dqkv, ld, h * 64, 1, 0, cu, B, T_alloc, tid, 64 * kNW);
  int base, n;
  record_rows(cu, b, S, T_alloc, base, n);
  const int nb = (n + kBlk - 1) / kBlk;
  if ((int)blockIdx.y >= nb) return;  // uniform, before any barrier (n = 0 included)
  const int yb = flip ? nb - 1 - (int)blockIdx.y : (int)blockIdx.y;
  const bf16_t* Qg = qkv + (long long)base * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* Og = o + (long long)base * H + h * 64;
  const bf16_t* dOg = dout + (long long)base * H + h * 64;
  const long long vrow = (long long)h * T_alloc + base;  // the record's LSE / D values
  lds_char* ring = smem;                                // kRing x {K KC | V KC}
  lds_char* scr = smem + kRing * kSlot + wave * kScr;   // dS [16 q][64 keys] KC
  const int nkc = min((n + 63) >> 6, 2 * yb + 2);
  const DenseKC<true> ks_{Kg, ld, n, 64};               // rows >= n: row n - 1
  const DenseKC<true> vs_{Vg, ld, n, 64};
  const int q0 = yb * kBlk + wave * 16;
  const bool active = q0 < n;  // wave-uniform
  const int qi = lane & 15;
  v8bf qa[2], da[2];
  float lq = 0.f, dd = 0.f;
  if (active) {
    qa[0] = gfrag_clamp(Qg, ld, q0, n, 0, lane);
    qa[1] = gfrag_clamp(Qg, ld, q0, n, 1, lane);
    da[0] = gfrag_clamp(dOg, (long long)H, q0, n, 0, lane);
    da[1] = gfrag_clamp(dOg, (long long)H, q0, n, 1, lane);
    // D of the wave's 16 rows: 4 lanes per row, 16 d each; kept for the lane's query and written for dKV
    const int row = lane >> 2, part = lane & 3;
    const int qd = q0 + row < n ? q0 + row : n - 1;
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
    if (part == 0 && q0 + row < n) dwork[vrow + q0 + row] = acc;
    dd = __shfl(acc, qi * 4, 64);
    lq = lse[vrow + (q0 + qi < n ? q0 + qi : n - 1)] * kLog2e;
  }
  stage_kc<64, DenseKC<true>, kNW>(ks_, ring, 0, 0, wave, lane);
  stage_kc<64, DenseKC<true>, kNW>(vs_, ring + kTile, 0, 0, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const float sl2 = scale * kLog2e;
  const uint32_t prow = ((uint32_t)bh * (uint32_t)S + (uint32_t)(q0 + qi)) * (uint32_t)(S >> 1);
  f32x4 dq[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int kc = 0; kc < nkc; ++kc) {
    const int cur = kc & 1, nxt = cur ^ 1;
    if (kc + 1 < nkc) {
      stage_kc<64, DenseKC<true>, kNW>(ks_, ring + nxt * kSlot, (kc + 1) * 64, 0, wave, lane);
      stage_kc<64, DenseKC<true>, kNW>(vs_, ring + nxt * kSlot + kTile, (kc + 1) * 64, 0, wave, lane);
    }
    if (active && kc * 64 <= q0) {
      const lds_char* kt = ring + cur * kSlot;
      if (kc * 64 + 63 <= q0)
        dq_chunk<false>(kt, kt + kTile, scr, qa, da, dq, lq, dd, kc, q0, lane, sl2, th, dscale, seed, prow);
      else
        dq_chunk<true>(kt, kt + kTile, scr, qa, da, dq, lq, dd, kc, q0, lane, sl2, th, dscale, seed, prow);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (active) {
    // accumulator rows >= n (clamped copies of row n - 1): not stored, and out of the bias gradient
    const int rleft = n - q0 - (lane >> 4) * 4;  // the lane's rows r < rleft are real
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) dq[j][r] = r < rleft ? dq[j][r] : 0.f;
    store_rows16_n(scr, dq, scale, dqkv + ((long long)base + q0) * ld + h * 64, ld, lane, n - q0);
  }
  if (dbias) {  // (kernel argument: uniform) the ring is idle after the loop's last barrier
    lds_float* bsum = reinterpret_cast<lds_float*>(ring);
    float sq[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) colsum16(dq, scale, sq);
    if (lane < 16)
#pragma unroll
      for (int j = 0; j < 4; ++j) bsum[wave * 64 + j * 16 + lane] = sq[j];
    dbias_reduce<64, kNW>(bsum, dbias, 0, H, h, tid);
  }
}

// ---------------------------------------------------------------------------------------------
// dKV: a wave's 16 keys stay in registers (rows >= n: row n - 1; only queries >= n would see them, and those are
// forced to 0); ring slots {Q | dO}, both MC (rows >= n: the zero page), with the chunk's 64 LSE and D values.
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) __launch_bounds__(64 * kNW)
attn_pcausal_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                        const float* __restrict__ lse, const int* __restrict__ cu, bf16_t* __restrict__ dqkv,
                        const float* __restrict__ dwork, int B, int S, int nh, int T_alloc, float scale, uint32_t th,
                        float dscale, uint32_t seed, float* __restrict__ dbias, int flip) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (b == B - 1 && blockIdx.y == 0) zero_tail(dqkv, ld, H + h * 64, 2, H, cu, B, T_alloc, tid, 64 * kNW);
  int base, n;
  record_rows(cu, b, S, T_alloc, base, n);
  const int nb = (n + kBlk - 1) / kBlk;  // the record's key blocks
  if ((int)blockIdx.y >= nb) return;     // uniform, before any barrier (n = 0 included)
  const int yb = flip ? nb - 1 - (int)blockIdx.y : (int)blockIdx.y;
  const bf16_t* Qg = qkv + (long long)base * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* dOg = dout + (long long)base * H + h * 64;
  lds_char* ring = smem;                                                     // kRing x {Q MC | dO MC}
  lds_float* LD = reinterpret_cast<lds_float*>(smem + kRing * kSlot);        // kRing x {64 LSE * log2(e) | 64 D}
  lds_char* scr = smem + kRing * (kSlot + kVec) + wave * kScr;               // [32 q][16 keys] x {P, dS}
  const int nqc = (n + 63) >> 6;  // query chunks the record has
  const int c0 = 2 * yb;          // the first query chunk that sees the block's keys (128 yb < n: c0 < nqc); even
  const DenseMC<true> qs_{Qg, ld, 64, n};               // rows >= n: the zero page
  const DenseMC<true> ds_{dOg, (long long)H, 64, n};
  // threads 0-63 carry the chunk's LSE, 64-127 its D; a query >= n reads row n - 1's (unused: it is forced to 0)
  const float* vsrc = (tid < 64 ? lse : dwork) + (long long)h * T_alloc + base;
  const float vmul = tid < 64 ? kLog2e : 1.f;
  const int vq = tid & 63;
  const int kb = yb * kBlk + wave * 16;
  const bool has_keys = kb < n;  // wave-uniform
  v8bf ka0, ka1, va0, va1;
  if (has_keys) {
    ka0 = gfrag_clamp(Kg, ld, kb, n, 0, lane), ka1 = gfrag_clamp(Kg, ld, kb, n, 1, lane);
    va0 = gfrag_clamp(Vg, ld, kb, n, 0, lane), va1 = gfrag_clamp(Vg, ld, kb, n, 1, lane);
  }
  stage_mc<64, DenseMC<true>, kNW>(qs_, ring, 0, c0 * 64, wave, lane);
  stage_mc<64, DenseMC<true>, kNW>(ds_, ring + kTile, 0, c0 * 64, wave, lane);
  if (tid < 128) {
    const int q = c0 * 64 + vq;
    LD[tid] = vsrc[q < n ? q : n - 1] * vmul;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const float sl2 = scale * kLog2e;
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dk[j] = dv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = c0; c < nqc; ++c) {
    const int cur = c & 1, nxt = cur ^ 1;
    const bool more = c + 1 < nqc;
    float vnext = 0.f;
    if (more) {
      stage_mc<64, DenseMC<true>, kNW>(qs_, ring + nxt * kSlot, 0, (c + 1) * 64, wave, lane);
      stage_mc<64, DenseMC<true>, kNW>(ds_, ring + nxt * kSlot + kTile, 0, (c + 1) * 64, wave, lane);
      const int q = (c + 1) * 64 + vq;
      if (tid < 128) vnext = vsrc[q < n ? q : n - 1] * vmul;
    }
    if (has_keys && c * 64 + 63 >= kb) {  // the chunk's last query sees the wave's first key
      const lds_char* Qt = ring + cur * kSlot;
      const lds_float* Ls = LD + cur * 128;
      const bool diag = c * 64 < kb + 15;
      dkv_chunk(Qt, Qt + kTile, Ls, Ls + 64, scr, scr + 1024, ka0, ka1, va0, va1, dk, dv, c, kb, n, bh, S, lane, sl2,
                th, dscale, seed, diag, diag || c * 64 + 63 >= n);
    }
    if (tid < 128 && more) LD[nxt * 128 + tid] = vnext;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (has_keys) {  // rows >= n of dk / dv are exactly zero: only forced queries see those keys
    bf16_t* gk = dqkv + ((long long)base + kb) * ld + H + h * 64;
    store_rows16_n(scr, dk, scale, gk, ld, lane, n - kb);
    store_rows16_n(scr, dv, 1.f, gk + H, ld, lane, n - kb);
  }
  if (dbias) {  // (kernel argument: uniform) the ring is idle after the loop's last barrier
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
}

int attn_packed_causal_supported(int S, int dh) { return dh == 64 && S >= 64 && S % 64 == 0 && S <= kStreamMaxS; }

void attn_packed_causal_fwd(const bf16_t* qkv, const int* cu, bf16_t* out, float* lse, int B, int S, int nh,
                            long long T_alloc, float p, uint32_t seed, hipStream_t st) {
  if (B <= 0) return;
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  hipLaunchKernelGGL(attn_pcausal_fwd_kernel, grid, dim3(64 * kNW), kLdsQ, st, qkv, cu, out, lse, B, S, nh,
                     (int)T_alloc, 0.125f, th, ds, seed, attn_causal_heavy_first_get()); DTG_LAUNCH_CHECK();
}

void attn_packed_causal_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* dout, const float* lse, const int* cu,
                            bf16_t* dqkv, float* dwork, int B, int S, int nh, long long T_alloc, float p,
                            uint32_t seed, float* dbias, hipStream_t st) {
  if (B <= 0) return;
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  const int heavy = attn_causal_heavy_first_get();
  // dQ first: it writes D = rowsum(dO * O) into dwork, which dKV reads.  The heaviest blocks first: the record's last
  // query blocks in dQ, its first key blocks in dKV.
  hipLaunchKernelGGL(attn_pcausal_dq_kernel, grid, dim3(64 * kNW), kLdsQ, st, qkv, o, dout, lse, cu, dqkv, dwork, B, S,
                     nh, (int)T_alloc, 0.125f, th, ds, seed, dbias, heavy); DTG_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_pcausal_dkv_kernel, grid, dim3(64 * kNW), kLdsKV, st, qkv, dout, lse, cu, dqkv, dwork, B, S,
                     nh, (int)T_alloc, 0.125f, th, ds, seed, dbias, !heavy); DTG_LAUNCH_CHECK();
}

}  // namespace dtg
