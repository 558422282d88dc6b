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
// in-chunk position t iff x >= t on the diagonal chunk and iff x < t on the upper-edge chunk.  The two-edged bodies of
// dtg/attn_causal_common.cuh (kEdges = 2) take a wave-uniform flag and invert the compare.  The kernels hold two body
// instances (unmasked, masked) in 128 VGPRs, as the causal ones do; a third does not fit.
//
// An invisible key is EXCLUDED, not given an additive constant: out of the running max and the row sum, P = 0
// exactly, dropout(P) = dS = 0.  The causal invariant "every chunk a wave computes holds a visible key of each row"
// does not survive the lower edge: on it, row qi = 15 with jd = 3 sees no key at all (x > 63), its chunk maximum is
// -inf and, the edge chunk being the wave's first, so is its running maximum; fwd_chunk's empty-row guard covers it,
// and m stays -inf for the next chunk, which every row shares (each row sees itself, so l > 0 at the end).
//   Forward NaN-proofing holds at both edges (fwd_chunk); chunks wholly outside a wave's window are not read by it at
// all.
//
// Dropout: the pair index stays ((b*nh + h)*S + q) * (S/2) + key/2 in wrapping uint32, so a visible element's draw is
// attn_dropout_keep's for the full [S, S] layout.
//
// Balance.  Blocks with 2y >= w all visit w + 2 chunks (forward / dQ; dKV: all but the last ceil(w/2) blocks); only
// the first blocks of forward / dQ are lighter.  blockIdx.y keeps attention_causal.hip's mapping and its switch
// (attn_causal_heavy_first): reversed for forward / dQ, identity for dKV.
#include "dtg/common.h"
#include "dtg/kernels.h"
#include "dtg/attn_causal_common.cuh"
#include "dtg/mfma_gemm.cuh"

namespace dtg {
using namespace gemm;
using namespace attn;
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
  const int qi = lane & 15;
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
        fwd_chunk<0, true>(Kt, Kt + kTile, Mk + cur * 128, scr, qa, m, l, o, kc, q0, lane, scale, th, dscale, seed,
                           prow, false);
      else
        fwd_chunk<2, true>(Kt, Kt + kTile, Mk + cur * 128, scr, qa, m, l, o, kc, q0, lane, scale, th, dscale, seed,
                           prow, kc != kd);
    }
    if (wave == 0 && more) Mk[nxt * 128 + lane] = mnext;
    // chunk kc + 1 has landed and every wave is done with slot cur, which the next iteration refills
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (!active) return;  // (no barrier below this point)
  fwd_store(scr, o, m, l, out, (long long)b * S + q0, H, h * 64, lse, (long long)bh * S + q0, lane);
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
    dq_row_terms<false>(dOg, Og, lse, dwork, (long long)bh * S, H, q0, S, lane, dd, lq);
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
        dq_chunk<0, true>(kt, kt + kTile, Mk + cur * 128, scr, qa, da, dq, lq, dd, kc, q0, lane, sl2, th, dscale, seed,
                          prow, false);
      else
        dq_chunk<2, true>(kt, kt + kTile, Mk + cur * 128, scr, qa, da, dq, lq, dd, kc, q0, lane, sl2, th, dscale, seed,
                          prow, kc != kd);
    }
    if (wave == 0 && more) Mk[nxt * 128 + lane] = mnext;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (active) store_rows16(scr, dq, scale, dqkv + ((long long)b * S + q0) * ld + h * 64, ld, lane);
  if (dbias) dq_dbias(ring, dq, scale, active, dbias, H, h, wave, lane, tid);  // (kernel argument: uniform)
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
      dkv_chunk<true, true, false>(Qt, Qt + kTile, Ls, Ls + 64, scr, scr + 1024, ka0, ka1, va0, va1, msl, dk, dv, c,
                                   kb, S, bh, S, lane, sl2, th, dscale, seed, c == cd, c == cup);
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
  if (dbias) dkv_dbias(ring, dk, dv, scale, has_keys, dbias, H, h, wave, lane, tid);  // (kernel argument: uniform)
}

int attn_window_supported(int S, int W, int dh) {
  return attn_causal_supported(S, dh) && W >= 64 && W % 64 == 0;
}

void attn_window_fwd(const bf16_t* qkv, const float* mask, bf16_t* out, float* lse, int B, int S, int nh, int window,
                     float p, uint32_t seed, hipStream_t st) {
  if (window >= S) return attn_causal_fwd(qkv, mask, out, lse, B, S, nh, p, seed, st);  // every key <= q is in reach
  const DropArgs d = drop_args(p);
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  hipLaunchKernelGGL(attn_window_fwd_kernel, grid, dim3(64 * kNW), kLds, st, qkv, mask, out, lse, S, nh, window / 64,
                     0.125f, d.th, d.dscale, seed, attn_causal_heavy_first_get()); DTG_LAUNCH_CHECK();
}

void attn_window_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* dout, const float* lse, const float* mask,
                     bf16_t* dqkv, float* dwork, int B, int S, int nh, int window, float p, uint32_t seed,
                     float* dbias, hipStream_t st) {
  if (window >= S) return attn_causal_bwd(qkv, o, dout, lse, mask, dqkv, dwork, B, S, nh, p, seed, dbias, st);
  const DropArgs d = drop_args(p);
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  const int heavy = attn_causal_heavy_first_get();
  // dQ first: it writes D = rowsum(dO * O) into dwork, which dKV reads
  hipLaunchKernelGGL(attn_window_dq_kernel, grid, dim3(64 * kNW), kLds, st, qkv, o, dout, lse, mask, dqkv, dwork, S,
                     nh, window / 64, 0.125f, d.th, d.dscale, seed, dbias, heavy); DTG_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_window_dkv_kernel, grid, dim3(64 * kNW), kLds, st, qkv, dout, lse, mask, dqkv, dwork, S, nh,
                     window / 64, 0.125f, d.th, d.dscale, seed, dbias, !heavy); DTG_LAUNCH_CHECK();
}

}  // namespace dtg
