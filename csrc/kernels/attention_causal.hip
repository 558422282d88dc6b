// Causal (lower-triangular) fused attention, forward and backward, for 64 <= S <= kStreamMaxS, S % 64 == 0: head dim
// 64, bf16, optional additive key mask, pair-hash dropout.  Operands, results, LDS layout and the chunk schedule are
// those of attention_stream.hip (64-row chunks through a 2-slot LDS ring, chunk c + 1's LDS-DMA in flight under chunk
// c's MFMAs, one barrier per chunk, all 8 waves stage and meet at every barrier); what differs is which chunks a
// workgroup and a wave touch at all:
//
//   forward, dQ (a wave owns queries q0 .. q0+15 of query block y = 128y .. 128y+127):
//     the workgroup's loop ends after key chunk min(S/64, 2y + 2) - 1: later chunks are neither staged nor waited for;
//     a wave skips the arithmetic of a chunk that starts beyond its last query (64c > q0 + 15: waves 0..3 on the
//     block's last chunk), runs the unmasked body on a chunk wholly at or below its first query (64c + 63 <= q0), and
//     pays the compare key <= q only on its one diagonal chunk, behind a wave-uniform branch.
//   dKV (a wave owns keys k0 .. k0+15 of key block y):
//     the loop starts at query chunk 2y (ring slot parity is the chunk's: 2y is even); a wave skips a chunk that ends
//     below its first key (64c + 63 < k0: waves 4..7 on chunk 2y) and pays the compare on the chunk that straddles the
//     diagonal (64c <= k0 + 15 and the skip did not apply).
//
// A key > q is EXCLUDED, not given an additive constant: it takes no part in the running max or the row sum, P = 0
// exactly, dropout(P) = dS = 0.  A row whose visible keys are all key-masked (-10000) therefore normalises over the
// visible keys alone.  Key 0 is visible to every query, so the running max is finite after chunk 0.
// An excluded key's K and V never reach a visible query's out or LSE, whatever their bits (fwd_chunk in
// dtg/attn_causal_common.cuh, where the chunk bodies and the frame-independent epilogues of these kernels live).
//
// Dropout: the pair index stays ((b*nh + h)*S + q) * (S/2) + key/2 in wrapping uint32 (attention_stream.hip's head
// comment), so a visible element's draw is attn_dropout_keep's for the full [S, S] layout.
//
// Balance.  Work per workgroup grows with y in forward / dQ and falls with y in dKV.  With heavy_first (the default)
// blockIdx.y is mapped so that the heaviest blocks are dispatched first: reversed for forward / dQ, identity for dKV;
// attn_causal_heavy_first(0) maps the other way round (the A/B switch of tools/bench_attention.py --causal).
#include "dtg/common.h"
#include "dtg/kernels.h"
#include "dtg/attn_causal_common.cuh"
#include "dtg/mfma_gemm.cuh"

namespace dtg {
using namespace gemm;
using namespace attn;

namespace {
int g_heavy_first = 1;
}  // namespace

// ---------------------------------------------------------------------------------------------
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) __launch_bounds__(64 * kNW) attn_causal_fwd_kernel(const bf16_t* __restrict__ qkv,
                                                                   const float* __restrict__ mask,
                                                                   bf16_t* __restrict__ out, float* __restrict__ lse,
                                                                   int S, int nh, float scale, uint32_t th,
                                                                   float dscale, uint32_t seed, int flip) {
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
  const int nkc = min(S / 64, 2 * yb + 2);  // the block's last query sees nothing beyond chunk 2 yb + 1
  const DenseKC<false> ks_{Kg, ld, S, 64};
  const DenseMC<false> vs_{Vg, ld, 64, S};
  const float* mrow = mask ? mask + (long long)b * S : nullptr;
  const int q0 = yb * kBlk + wave * 16;
  const bool active = q0 < S;  // wave-uniform
  v8bf qa[2];
  if (active) {
    qa[0] = gfrag(Qg, ld, q0, 0, lane);
    qa[1] = gfrag(Qg, ld, q0, 1, lane);
  }
  stage_kc<64, DenseKC<false>, kNW>(ks_, ring, 0, 0, wave, lane);
  stage_mc<64, DenseMC<false>, kNW>(vs_, ring + kTile, 0, 0, wave, lane);
  if (wave == 0) Mk[lane] = mrow ? mrow[lane] : 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int qi = lane & 15;
  // pair index of (q, key 0), wrapping (see the head of attention_stream.hip)
  const uint32_t prow = ((uint32_t)bh * (uint32_t)S + (uint32_t)(q0 + qi)) * (uint32_t)(S >> 1);
#pragma unroll 1
  for (int kc = 0; kc < nkc; ++kc) {
    const int cur = kc & 1, nxt = cur ^ 1;
    const bool more = kc + 1 < nkc;
    float mnext = 0.f;
    if (more) {
      stage_kc<64, DenseKC<false>, kNW>(ks_, ring + nxt * kSlot, (kc + 1) * 64, 0, wave, lane);
      stage_mc<64, DenseMC<false>, kNW>(vs_, ring + nxt * kSlot + kTile, 0, (kc + 1) * 64, wave, lane);
      if (wave == 0 && mrow) mnext = mrow[(kc + 1) * 64 + lane];
    }
    if (active && kc * 64 <= q0) {  // (q0 % 16 == 0: the chunk starts at or below the wave's last query)
      const lds_char* Kt = ring + cur * kSlot;
      if (kc * 64 + 63 <= q0)
        fwd_chunk<0, true>(Kt, Kt + kTile, Mk + cur * 128, scr, qa, m, l, o, kc, q0, lane, scale, th, dscale, seed,
                           prow, false);
      else
        fwd_chunk<1, true>(Kt, Kt + kTile, Mk + cur * 128, scr, qa, m, l, o, kc, q0, lane, scale, th, dscale, seed,
                           prow, false);
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
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) __launch_bounds__(64 * kNW) attn_causal_dq_kernel(const bf16_t* __restrict__ qkv,
                                                                  const bf16_t* __restrict__ o,
                                                                  const bf16_t* __restrict__ dout,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ mask,
                                                                  bf16_t* __restrict__ dqkv, float* __restrict__ dwork,
                                                                  int S, int nh, float scale, uint32_t th,
                                                                  float dscale, uint32_t seed,
                                                                  float* __restrict__ dbias, int flip) {
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
  const int nkc = min(S / 64, 2 * yb + 2);
  const DenseKC<false> ks_{Kg, ld, S, 64};
  const DenseKC<false> vs_{Vg, ld, S, 64};
  const float* mrow = mask ? mask + (long long)b * S : nullptr;
  const int q0 = yb * kBlk + wave * 16;
  const bool active = q0 < S;  // wave-uniform
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
  stage_kc<64, DenseKC<false>, kNW>(ks_, ring, 0, 0, wave, lane);
  stage_kc<64, DenseKC<false>, kNW>(vs_, ring + kTile, 0, 0, wave, lane);
  if (wave == 0) Mk[lane] = mrow ? mrow[lane] * kLog2e : 0.f;
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
    const bool more = kc + 1 < nkc;
    float mnext = 0.f;
    if (more) {
      stage_kc<64, DenseKC<false>, kNW>(ks_, ring + nxt * kSlot, (kc + 1) * 64, 0, wave, lane);
      stage_kc<64, DenseKC<false>, kNW>(vs_, ring + nxt * kSlot + kTile, (kc + 1) * 64, 0, wave, lane);
      if (wave == 0 && mrow) mnext = mrow[(kc + 1) * 64 + lane] * kLog2e;
    }
    if (active && kc * 64 <= q0) {
      const lds_char* kt = ring + cur * kSlot;
      if (kc * 64 + 63 <= q0)
        dq_chunk<0, true>(kt, kt + kTile, Mk + cur * 128, scr, qa, da, dq, lq, dd, kc, q0, lane, sl2, th, dscale, seed,
                          prow, false);
      else
        dq_chunk<1, true>(kt, kt + kTile, Mk + cur * 128, scr, qa, da, dq, lq, dd, kc, q0, lane, sl2, th, dscale, seed,
                          prow, false);
    }
    if (wave == 0 && more) Mk[nxt * 128 + lane] = mnext;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (active) store_rows16(scr, dq, scale, dqkv + ((long long)b * S + q0) * ld + h * 64, ld, lane);
  if (dbias) dq_dbias(ring, dq, scale, active, dbias, H, h, wave, lane, tid);  // (kernel argument: uniform)
}

// ---------------------------------------------------------------------------------------------
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) __launch_bounds__(64 * kNW) attn_causal_dkv_kernel(const bf16_t* __restrict__ qkv,
                                                                   const bf16_t* __restrict__ dout,
                                                                   const float* __restrict__ lse,
                                                                   const float* __restrict__ mask,
                                                                   bf16_t* __restrict__ dqkv,
                                                                   const float* __restrict__ dwork, int S, int nh,
                                                                   float scale, uint32_t th, float dscale,
                                                                   uint32_t seed, float* __restrict__ dbias,
                                                                   int flip) {
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
  const int nqc = S / 64;
  const int c0 = 2 * yb;  // the first query chunk that sees the block's keys; even, so slot parity is c & 1
  const DenseMC<false> qs_{Qg, ld, 64, S};
  const DenseMC<false> ds_{dOg, (long long)H, 64, S};
  // threads 0-63 carry the chunk's LSE, 64-127 its D
  const float* vsrc = (tid < 64 ? lse : dwork) + (long long)bh * S + (tid & 63);
  const float vmul = tid < 64 ? kLog2e : 1.f;
  const int kb = yb * kBlk + wave * 16;
  const bool has_keys = kb < S;  // wave-uniform
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
  stage_mc<64, DenseMC<false>, kNW>(qs_, ring, 0, c0 * 64, wave, lane);
  stage_mc<64, DenseMC<false>, kNW>(ds_, ring + kTile, 0, c0 * 64, wave, lane);
  if (tid < 128) LD[tid] = vsrc[c0 * 64] * vmul;
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
      stage_mc<64, DenseMC<false>, kNW>(qs_, ring + nxt * kSlot, 0, (c + 1) * 64, wave, lane);
      stage_mc<64, DenseMC<false>, kNW>(ds_, ring + nxt * kSlot + kTile, 0, (c + 1) * 64, wave, lane);
      if (tid < 128) vnext = vsrc[(c + 1) * 64] * vmul;
    }
    if (has_keys && c * 64 + 63 >= kb) {  // the chunk's last query sees the wave's first key
      const lds_char* Qt = ring + cur * kSlot;
      const lds_float* Ls = LD + cur * 128;
      dkv_chunk<false, true, false>(Qt, Qt + kTile, Ls, Ls + 64, scr, scr + 1024, ka0, ka1, va0, va1, msl, dk, dv, c,
                                    kb, S, bh, S, lane, sl2, th, dscale, seed, c * 64 < kb + 15, false);
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

int attn_causal_supported(int S, int dh) { return dh == 64 && S >= 64 && S % 64 == 0 && S <= kStreamMaxS; }

void attn_causal_heavy_first(int on) { g_heavy_first = on != 0; }
int attn_causal_heavy_first_get() { return g_heavy_first; }

void attn_causal_fwd(const bf16_t* qkv, const float* mask, bf16_t* out, float* lse, int B, int S, int nh, float p,
                     uint32_t seed, hipStream_t st) {
  const DropArgs d = drop_args(p);
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  hipLaunchKernelGGL(attn_causal_fwd_kernel, grid, dim3(64 * kNW), kLds, st, qkv, mask, out, lse, S, nh, 0.125f, d.th,
                     d.dscale, seed, g_heavy_first); DTG_LAUNCH_CHECK();
}

void attn_causal_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* dout, const float* lse, const float* mask,
                     bf16_t* dqkv, float* dwork, int B, int S, int nh, float p, uint32_t seed, float* dbias,
                     hipStream_t st) {
  const DropArgs d = drop_args(p);
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  // dQ first: it writes D = rowsum(dO * O) into dwork, which dKV reads.  The heaviest blocks first: the last query
  // blocks of dQ, the first key blocks of dKV.
  hipLaunchKernelGGL(attn_causal_dq_kernel, grid, dim3(64 * kNW), kLds, st, qkv, o, dout, lse, mask, dqkv, dwork, S,
                     nh, 0.125f, d.th, d.dscale, seed, dbias, g_heavy_first); DTG_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_causal_dkv_kernel, grid, dim3(64 * kNW), kLds, st, qkv, dout, lse, mask, dqkv, dwork, S, nh,
                     0.125f, d.th, d.dscale, seed, dbias, !g_heavy_first); DTG_LAUNCH_CHECK();
}

}  // namespace dtg
