// Sliding-window causal fused attention, forward and backward, for 64 <= S <= kStreamMaxS, S % 64 == 0, and a window
// W % 64 == 0, 64 <= W < S (W >= S is plain causal attention: the launchers hand it to attention_causal.hip): head dim
// 64, bf16, optional additive key mask, pair-hash dropout.  Query q sees key k iff q - W < k <= q: W keys, itself
// included.  Operands, results, LDS layout and the chunk schedule are those of attention_causal.hip (64-row chunks
// through a 2-slot LDS ring, chunk c + 1's LDS-DMA in flight under chunk c's MFMAs, one barrier per chunk, all 8 waves
// stage and meet at every barrier); what differs is that the chunk loop has a moving bound at BOTH ends, so the work
// of a block is W/64 + 2 chunks whatever S is.  With w = W/64:
//
//   forward, dQ (a wave owns queries q0 .. q0+15 of query block y = 128y .. 128y+127):
//     the workgroup visits key chunks max(0, 2y - w) .. min(S/64, 2y + 2) - 1; chunks outside are neither staged nor
//     waited for.  The first chunk has the parity of w, so a chunk's ring slot is its own parity (c & 1), the
//     prologue's included.  The wave's diagonal chunk is kd = q0 / 64, its lower-edge chunk kd - w (none while
//     q0 < W); it skips the arithmetic of every chunk above kd or below kd - w, runs the unmasked body strictly
//     between the two and the masked body on both.
//   dKV (a wave owns keys k0 .. k0+15 of key block y):
//     the workgroup visits query chunks 2y .. min(S/64 - 1, 2y + 1 + w).  The wave's diagonal chunk is cd = k0 / 64,
//     its upper-edge chunk cd + w; it skips every chunk below cd or above cd + w and pays the compares on those two.
//
// The two edges share one masked body.  W % 64 == 0 puts the lower edge's partial 16-key block at the SAME in-chunk
// block index jd = (q0 % 64) / 16 as the diagonal block, with the exact complement of the diagonal predicate: with
// t = q0 % 64 + qi (the query's position in its diagonal chunk) a key at in-chunk position x is visible iff x <= t on
// the diagonal chunk and iff x > t on the lower-edge chunk; in dKV a query at in-chunk position x sees the key at
// in-chunk position t iff x >= t on the diagonal chunk and iff x < t on the upper-edge chunk.  The body takes a
// wave-uniform flag and inverts the compare ((x <= t) != lo).  The kernels hold two body instances (unmasked, masked)
// in 128 VGPRs, as the causal ones do; a third does not fit.
//
// An invisible key is EXCLUDED, not given an additive constant: out of the running max and the row sum, P = 0
// exactly, dropout(P) = dS = 0.  The causal invariant "every chunk a wave computes holds a visible key of each row"
// does not survive the lower edge: on it, row qi = 15 with jd = 3 sees no key at all (x > 63), its chunk maximum is
// -inf and, the edge chunk being the wave's first, so is its running maximum.  The masked body therefore subtracts 0
// instead of a -inf maximum: alpha = exp(-inf) = 0 on l = 0 and o = 0, P = exp(-inf) = 0, and m stays -inf for the
// next chunk, which every row shares (each row sees itself, so l > 0 at the end).
//   Forward NaN-proofing holds at both edges: on a masked chunk the V^T fragments of the 16-key blocks the wave may not
// see (diagonal: at and above jd; lower edge: at and below jd) are replaced by zeros and block jd itself is
// accumulated on the VALU under the predicate, so an excluded key's K and V never reach a visible query's out or LSE,
// whatever their bits.  Chunks wholly outside a wave's window are not read by it at all.  The backward multiplies the
// exact zeros of dS and dropout(P) by operands it takes to be finite.
//
// Dropout: the pair index stays ((b*nh + h)*S + q) * (S/2) + key/2 in wrapping uint32, so a visible element's draw is
// attn_dropout_keep's for the full [S, S] layout.
//
// Balance.  Blocks with 2y >= w all visit w + 2 chunks (forward / dQ; dKV: all but the last ceil(w/2) blocks); only
// the first blocks of forward / dQ are lighter.  blockIdx.y keeps attention_causal.hip's mapping and its switch
// (attn_causal_heavy_first): reversed for forward / dQ, identity for dKV.
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
constexpr int kVec = 512;              // per-slot fp32 values travelling with a chunk (mask, or LSE | D)
constexpr int kScr = 2048;             // per-wave scratch
constexpr size_t kLds = (size_t)kRing * (kSlot + kVec) + kNW * kScr;  // 49.0 KiB: three workgroups per CU
constexpr float kLog2e = 1.4426950408889634f;

typedef const __attribute__((address_space(3))) f32x4 lds_f32x4;
typedef const __attribute__((address_space(3))) bf16_t lds_bf16;
typedef const __attribute__((address_space(3))) u32x2v lds_u32x2;

// One key chunk of the forward for a wave's 16 queries.  kMask: the chunk is the wave's diagonal chunk (lo = false) or
// its lower-edge chunk (lo = true, wave-uniform); lane (qi, g) holds query q0 + qi against keys j * 16 + 4g + [0, 4)
// of each 16-key block j.
template <bool kMask>
__device__ __forceinline__ void fwd_chunk(const lds_char* Kt, const lds_char* Vt, const lds_float* Mc, lds_char* scr,
                                          const v8bf (&qa)[2], float& m, float& l, f32x4 (&o)[4], int kc, int q0,
                                          int lane, float scale, uint32_t th, float dscale, uint32_t seed,
                                          uint32_t prow, bool lo) {
  const int qi = lane & 15, g = lane >> 4;
  const int jd = (q0 & 63) >> 4;  // (kMask) the partial 16-key block, at either edge
  // (kMask) key x of the chunk against the query's position t = jd * 16 + qi: x <= t is (x - t - 1) < 0, and x > t is
  // ~(x - t - 1) < 0, so the edge's inversion is an xor with a wave-uniform word, in the VALU (a compare inverted in
  // the lane masks keeps 16 loop-invariant masks alive in SGPRs, which then spill)
  const int inv = lo ? -1 : 0, xt = 4 * g - jd * 16 - qi - 1;
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
    const f32x4 madd = *reinterpret_cast<lds_f32x4*>(Mc + j * 16 + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = fmaf(s[j][r], scale, madd[r]);
      // excluded: out of the max here, and P = exp(-inf - finite) = 0 below (a select, whatever K held)
      s[j][r] = (!kMask || ((j * 16 + r + xt) ^ inv) < 0) ? v : -INFINITY;
      mx = fmaxf(mx, s[j][r]);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float mn = fmaxf(m, mx);
  // an unmasked or diagonal chunk holds a visible key of each row; the lower edge's row 15 of jd = 3 holds none, and
  // with m still -inf the subtrahend is 0: alpha = 0 on l = o = 0, P = 0, m stays -inf
  const float mref = (kMask && mn == -INFINITY) ? 0.f : mn;
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
  // inside the window go through the MFMA (diagonal: below jd; lower edge: above jd)
  const v8bf zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const int b0 = g >> 1, b1 = 2 + (g >> 1);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v8bf v0 = frag_mc<64>(Vt, j * 16, 0, lane), v1 = frag_mc<64>(Vt, j * 16, 1, lane);
    if (kMask) {
      if (b0 == jd || (b0 > jd) != lo) v0 = zero;
      if (b1 == jd || (b1 > jd) != lo) v1 = zero;
    }
    o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, pb0, o[j], 0, 0, 0);
    o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v1, pb1, o[j], 0, 0, 0);
  }
  if (kMask) {
    // the partial 16 x 16 block: O^T[d][q] += V[key][d] * P[q][key] for the visible keys only, P as the MFMA would
    // read it (bf16 out of the scratch); the lane's d are j * 16 + 4g + [0, 4), 8 bytes of V's MC row
#pragma unroll 2
    for (int kk = 0; kk < 16; ++kk) {
      const int kl = jd * 16 + kk;
      const float pv = bf2f(*reinterpret_cast<lds_bf16*>(scr + kc_off(qi, kl)));
      const lds_char* vrow = Vt + kl * 128 + (g & 1) * 8;
      const int sw = mc_swz<8>(kl);
      if (((kk - qi - 1) ^ inv) < 0) {
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

// One key chunk of dQ for a wave's 16 queries (attn_causal_dq_kernel's body; kMask and lo as in fwd_chunk)
template <bool kMask>
__device__ __forceinline__ void dq_chunk(const lds_char* kt, const lds_char* vt, const lds_float* Mc, lds_char* scr,
                                         const v8bf (&qa)[2], const v8bf (&da)[2], f32x4 (&dq)[4], float lq, float dd,
                                         int kc, int q0, int lane, float sl2, uint32_t th, float dscale,
                                         uint32_t seed, uint32_t prow, bool lo) {
  const int qi = lane & 15, g = lane >> 4;
  // (kMask) t = q0 % 64 + qi is the query's position in its diagonal chunk; the compare as in fwd_chunk
  const int inv = lo ? -1 : 0, xt = 4 * g - (q0 & 63) - qi - 1;
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
    const f32x4 madd = *reinterpret_cast<lds_f32x4*>(Mc + j * 16 + 4 * g);
    bool kp[4] = {true, true, true, true};
    if (th) keep4_pair(seed, prow + (uint32_t)(key0 >> 1), th, kp);
    float dsv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __builtin_amdgcn_exp2f(fmaf(s[j][r], sl2, madd[r] - lq));
      float dpv = dp[j][r];
      if (th) dpv = kp[r] ? dpv * dscale : 0.f;
      dsv[r] = (!kMask || ((j * 16 + r + xt) ^ inv) < 0) ? p * (dpv - dd) : 0.f;
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

// One query chunk of dKV for a wave's 16 keys kb .. kb+15 (attn_causal_dkv_kernel's body).  masked: the chunk is the
// wave's diagonal chunk (up = false) or its upper-edge chunk, W queries later (up = true); both wave-uniform, one
// body, the compare in a branch of its own.  A 32-query half with no visible pair is skipped: wholly before the
// wave's first key on the diagonal chunk, wholly at or beyond its last key + W on the upper edge.
__device__ __forceinline__ void dkv_chunk(const lds_char* Qt, const lds_char* dOt, const lds_float* Ls,
                                          const lds_float* Ds, lds_char* scp, lds_char* scs, v8bf ka0, v8bf ka1,
                                          v8bf va0, v8bf va1, const float (&msl)[4], f32x4 (&dk)[4], f32x4 (&dv)[4],
                                          int c, int kb, int bh, int S, int lane, float sl2, uint32_t th,
                                          float dscale, uint32_t seed, bool masked, bool up) {
  const int rbase = (lane >> 4) * 4;
  const int t0 = kb & 63;  // the first key's position in its diagonal chunk
  const int inv = up ? -1 : 0;
#pragma unroll
  for (int kq = 0; kq < 2; ++kq) {  // 32-query halves of the chunk
    if (masked && (up ? kq * 32 >= t0 + 15 : kq * 32 + 31 < t0)) continue;  // wave-uniform
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
        const float p = __builtin_amdgcn_exp2f(fmaf(st[ni][r], sl2, msl[r] - lq));
        float pv = p, dp = dpt[ni][r];
        if (th) {
          pv = kp[r] ? p * dscale : 0.f;
          dp = kp[r] ? dp * dscale : 0.f;
        }
        pd[r] = pv;
        dsv[r] = p * (dp - dq);
      }
      if (masked) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // the key's in-chunk position <= the query's: visible on the diagonal chunk, invisible on the upper edge
          const bool vis = ((t0 + rbase + r - qs - 1) ^ inv) < 0;  // (the xor: see fwd_chunk)
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
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) __launch_bounds__(64 * kNW)
attn_window_fwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ mask, bf16_t* __restrict__ out,
                       float* __restrict__ lse, int S, int nh, int w64, float scale, uint32_t th, float dscale,
                       uint32_t seed, int flip) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int yb = flip ? (int)(gridDim.y - 1 - blockIdx.y) : (int)blockIdx.y;  // the query block
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bf16_t* Qg = qkv + (long long)b * S * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  lds_char* ring = smem;                                                     // kRing x {K KC | V MC}
  lds_float* Mk = reinterpret_cast<lds_float*>(smem + kRing * kSlot);        // kRing x 64 mask values (stride 128)
  lds_char* scr = smem + kRing * (kSlot + kVec) + wave * kScr;               // per-wave [16][64] bf16
  const int kc0 = max(0, 2 * yb - w64);     // the block's first query sees nothing below chunk 2 yb - w64
  const int nkc = min(S / 64, 2 * yb + 2);  // its last query sees nothing beyond chunk 2 yb + 1
  const DenseKC<false> ks_{Kg, ld, S, 64};
  const DenseMC<false> vs_{Vg, ld, 64, S};
  const float* mrow = mask ? mask + (long long)b * S : nullptr;
  const int q0 = yb * kBlk + wave * 16;
  const bool active = q0 < S;  // wave-uniform
  const int kd = q0 >> 6, klo = kd - w64;  // the wave's diagonal and lower-edge chunks (klo < 0: no lower edge)
  const int kfirst = max(klo, 0);
  v8bf qa[2];
  if (active) {
    qa[0] = gfrag(Qg, ld, q0, 0, lane);
    qa[1] = gfrag(Qg, ld, q0, 1, lane);
  }
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int qi = lane & 15, g = lane >> 4;
  // pair index of (q, key 0), wrapping (see the head of attention_stream.hip)
  const uint32_t prow = ((uint32_t)bh * (uint32_t)S + (uint32_t)(q0 + qi)) * (uint32_t)(S >> 1);
#pragma unroll 1
  // the pass at kc0 - 1 is the prologue: it stages chunk kc0 and computes nothing (kc0 - 1 < kfirst), so the first
  // chunk takes the slot of its own parity by the loop's one staging sequence
  for (int kc = kc0 - 1; kc < nkc; ++kc) {
    const int cur = kc & 1, nxt = cur ^ 1;
    const bool more = kc + 1 < nkc;
    float mnext = 0.f;
    if (more) {
      stage_kc<64, DenseKC<false>, kNW>(ks_, ring + nxt * kSlot, (kc + 1) * 64, 0, wave, lane);
      stage_mc<64, DenseMC<false>, kNW>(vs_, ring + nxt * kSlot + kTile, 0, (kc + 1) * 64, wave, lane);
      if (wave == 0 && mrow) mnext = mrow[(kc + 1) * 64 + lane];
    }
    if (active && kc <= kd && kc >= kfirst) {  // (wave-uniform) the chunk meets the wave's window
      const lds_char* Kt = ring + cur * kSlot;
      if (kc < kd && kc > klo)
        fwd_chunk<false>(Kt, Kt + kTile, Mk + cur * 128, scr, qa, m, l, o, kc, q0, lane, scale, th, dscale, seed, prow,
                         false);
      else
        fwd_chunk<true>(Kt, Kt + kTile, Mk + cur * 128, scr, qa, m, l, o, kc, q0, lane, scale, th, dscale, seed, prow,
                        kc != kd);
    }
    if (wave == 0 && more) Mk[nxt * 128 + lane] = mnext;
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
  if (g == 0) lse[(long long)bh * S + q0 + qi] = m + __logf(l);
  lds_fence();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = lane + 64 * i;  // 128 chunks of 16 B: row c/8, chunk c%8
    const int row = c >> 3, ch = c & 7;
    const v8bf v = *reinterpret_cast<const lds_v8bf*>(scr + row * 128 + ((ch ^ (row & 7)) << 4));
    *reinterpret_cast<v8bf*>(out + ((long long)b * S + q0 + row) * H + h * 64 + ch * 8) = v;
  }
}

// ---------------------------------------------------------------------------------------------
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) __launch_bounds__(64 * kNW)
attn_window_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout,
                      const float* __restrict__ lse, const float* __restrict__ mask, bf16_t* __restrict__ dqkv,
                      float* __restrict__ dwork, int S, int nh, int w64, float scale, uint32_t th, float dscale,
                      uint32_t seed, float* __restrict__ dbias, int flip) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int yb = flip ? (int)(gridDim.y - 1 - blockIdx.y) : (int)blockIdx.y;  // the query block
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bf16_t* Qg = qkv + (long long)b * S * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* Og = o + (long long)b * S * H + h * 64;
  const bf16_t* dOg = dout + (long long)b * S * H + h * 64;
  lds_char* ring = smem;                                                     // kRing x {K KC | V KC}
  lds_float* Mk = reinterpret_cast<lds_float*>(smem + kRing * kSlot);        // kRing x 64 mask values * log2(e)
  lds_char* scr = smem + kRing * (kSlot + kVec) + wave * kScr;               // dS [16 q][64 keys] KC
  const int kc0 = max(0, 2 * yb - w64);
  const int nkc = min(S / 64, 2 * yb + 2);
  const DenseKC<false> ks_{Kg, ld, S, 64};
  const DenseKC<false> vs_{Vg, ld, S, 64};
  const float* mrow = mask ? mask + (long long)b * S : nullptr;
  const int q0 = yb * kBlk + wave * 16;
  const bool active = q0 < S;  // wave-uniform
  const int kd = q0 >> 6, klo = kd - w64;
  const int kfirst = max(klo, 0);
  const int qi = lane & 15;
  v8bf qa[2], da[2];
  float lq = 0.f, dd = 0.f;
  if (active) {
    qa[0] = gfrag(Qg, ld, q0, 0, lane);
    qa[1] = gfrag(Qg, ld, q0, 1, lane);
    da[0] = gfrag(dOg, (long long)H, q0, 0, lane);
    da[1] = gfrag(dOg, (long long)H, q0, 1, lane);
    // D of the wave's 16 rows: 4 lanes per row, 16 d each; kept for the lane's query and written for dKV
    const int row = lane >> 2, part = lane & 3;
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float a[8], bb[8];
      load8_bf16(dOg + (long long)(q0 + row) * H + part * 16 + c * 8, a);
      load8_bf16(Og + (long long)(q0 + row) * H + part * 16 + c * 8, bb);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += a[k] * bb[k];
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    if (part == 0) dwork[(long long)bh * S + q0 + row] = acc;
    dd = __shfl(acc, qi * 4, 64);
    lq = lse[(long long)bh * S + q0 + qi] * kLog2e;
  }
  const float sl2 = scale * kLog2e;
  const uint32_t prow = ((uint32_t)bh * (uint32_t)S + (uint32_t)(q0 + qi)) * (uint32_t)(S >> 1);
  f32x4 dq[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int kc = kc0 - 1; kc < nkc; ++kc) {  // (kc0 - 1: the prologue pass, as in the forward)
    const int cur = kc & 1, nxt = cur ^ 1;
    const bool more = kc + 1 < nkc;
    float mnext = 0.f;
    if (more) {
      stage_kc<64, DenseKC<false>, kNW>(ks_, ring + nxt * kSlot, (kc + 1) * 64, 0, wave, lane);
      stage_kc<64, DenseKC<false>, kNW>(vs_, ring + nxt * kSlot + kTile, (kc + 1) * 64, 0, wave, lane);
      if (wave == 0 && mrow) mnext = mrow[(kc + 1) * 64 + lane] * kLog2e;
    }
    if (active && kc <= kd && kc >= kfirst) {
      const lds_char* kt = ring + cur * kSlot;
      if (kc < kd && kc > klo)
        dq_chunk<false>(kt, kt + kTile, Mk + cur * 128, scr, qa, da, dq, lq, dd, kc, q0, lane, sl2, th, dscale, seed,
                        prow, false);
      else
        dq_chunk<true>(kt, kt + kTile, Mk + cur * 128, scr, qa, da, dq, lq, dd, kc, q0, lane, sl2, th, dscale, seed,
                       prow, kc != kd);
    }
    if (wave == 0 && more) Mk[nxt * 128 + lane] = mnext;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (active) store_rows16(scr, dq, scale, dqkv + ((long long)b * S + q0) * ld + h * 64, ld, lane);
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
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) __launch_bounds__(64 * kNW)
attn_window_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                       const float* __restrict__ mask, bf16_t* __restrict__ dqkv, const float* __restrict__ dwork,
                       int S, int nh, int w64, float scale, uint32_t th, float dscale, uint32_t seed,
                       float* __restrict__ dbias, int flip) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int yb = flip ? (int)(gridDim.y - 1 - blockIdx.y) : (int)blockIdx.y;  // the key block
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bf16_t* Qg = qkv + (long long)b * S * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* dOg = dout + (long long)b * S * H + h * 64;
  lds_char* ring = smem;                                                     // kRing x {Q MC | dO MC}
  lds_float* LD = reinterpret_cast<lds_float*>(smem + kRing * kSlot);        // kRing x {64 LSE * log2(e) | 64 D}
  lds_char* scr = smem + kRing * (kSlot + kVec) + wave * kScr;               // [32 q][16 keys] x {P, dS}
  const int c0 = 2 * yb;  // the first query chunk that sees the block's keys; even, so slot parity is c & 1
  const int nqc = min(S / 64, 2 * yb + 2 + w64);  // the block's last key is seen by nothing beyond chunk 2 yb + 1 + w64
  const DenseMC<false> qs_{Qg, ld, 64, S};
  const DenseMC<false> ds_{dOg, (long long)H, 64, S};
  // threads 0-63 carry the chunk's LSE, 64-127 its D
  const float* vsrc = (tid < 64 ? lse : dwork) + (long long)bh * S + (tid & 63);
  const float vmul = tid < 64 ? kLog2e : 1.f;
  const int kb = yb * kBlk + wave * 16;
  const bool has_keys = kb < S;  // wave-uniform
  const int cd = kb >> 6, cup = cd + w64;  // the wave's diagonal and upper-edge chunks
  const int rbase = (lane >> 4) * 4;
  float msl[4] = {0.f, 0.f, 0.f, 0.f};
  v8bf ka0, ka1, va0, va1;
  if (has_keys) {
    if (mask) {
#pragma unroll
      for (int r = 0; r < 4; ++r) msl[r] = mask[(long long)b * S + kb + rbase + r] * kLog2e;
    }
    ka0 = gfrag(Kg, ld, kb, 0, lane), ka1 = gfrag(Kg, ld, kb, 1, lane);
    va0 = gfrag(Vg, ld, kb, 0, lane), va1 = gfrag(Vg, ld, kb, 1, lane);
  }
  const float sl2 = scale * kLog2e;
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dk[j] = dv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = c0 - 1; c < nqc; ++c) {  // (c0 - 1 < cd: the prologue pass stages chunk c0 and computes nothing)
    const int cur = c & 1, nxt = cur ^ 1;
    const bool more = c + 1 < nqc;
    float vnext = 0.f;
    if (more) {
      stage_mc<64, DenseMC<false>, kNW>(qs_, ring + nxt * kSlot, 0, (c + 1) * 64, wave, lane);
      stage_mc<64, DenseMC<false>, kNW>(ds_, ring + nxt * kSlot + kTile, 0, (c + 1) * 64, wave, lane);
      if (tid < 128) vnext = vsrc[(c + 1) * 64] * vmul;
    }
    if (has_keys && c >= cd && c <= cup) {  // (wave-uniform) a query of the chunk sees a key of the wave
      const lds_char* Qt = ring + cur * kSlot;
      const lds_float* Ls = LD + cur * 128;
      dkv_chunk(Qt, Qt + kTile, Ls, Ls + 64, scr, scr + 1024, ka0, ka1, va0, va1, msl, dk, dv, c, kb, bh, S, lane, sl2,
                th, dscale, seed, c == cd || c == cup, c != cd);
    }
    if (tid < 128 && more) LD[nxt * 128 + tid] = vnext;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (has_keys) {
    bf16_t* gk = dqkv + ((long long)b * S + kb) * ld + H + h * 64;
    store_rows16(scr, dk, scale, gk, ld, lane);
    store_rows16(scr, dv, 1.f, gk + H, ld, lane);
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

int attn_window_supported(int S, int W, int dh) {
  return attn_causal_supported(S, dh) && W >= 64 && W % 64 == 0;
}

void attn_window_fwd(const bf16_t* qkv, const float* mask, bf16_t* out, float* lse, int B, int S, int nh, int window,
                     float p, uint32_t seed, hipStream_t st) {
  if (window >= S) return attn_causal_fwd(qkv, mask, out, lse, B, S, nh, p, seed, st);  // every key <= q is in reach
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  hipLaunchKernelGGL(attn_window_fwd_kernel, grid, dim3(64 * kNW), kLds, st, qkv, mask, out, lse, S, nh, window / 64,
                     0.125f, th, ds, seed, attn_causal_heavy_first_get()); DTG_LAUNCH_CHECK();
}

void attn_window_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* dout, const float* lse, const float* mask,
                     bf16_t* dqkv, float* dwork, int B, int S, int nh, int window, float p, uint32_t seed,
                     float* dbias, hipStream_t st) {
  if (window >= S) return attn_causal_bwd(qkv, o, dout, lse, mask, dqkv, dwork, B, S, nh, p, seed, dbias, st);
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  const int heavy = attn_causal_heavy_first_get();
  // dQ first: it writes D = rowsum(dO * O) into dwork, which dKV reads
  hipLaunchKernelGGL(attn_window_dq_kernel, grid, dim3(64 * kNW), kLds, st, qkv, o, dout, lse, mask, dqkv, dwork, S,
                     nh, window / 64, 0.125f, th, ds, seed, dbias, heavy); DTG_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_window_dkv_kernel, grid, dim3(64 * kNW), kLds, st, qkv, dout, lse, mask, dqkv, dwork, S, nh,
                     window / 64, 0.125f, th, ds, seed, dbias, !heavy); DTG_LAUNCH_CHECK();
}

}  // namespace dtg
