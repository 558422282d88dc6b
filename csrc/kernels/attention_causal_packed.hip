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
// not see, as in attention_causal.hip (the shared fwd_chunk of dtg/attn_causal_common.cuh, instantiated without a
// mask operand) -- and no row of another record is loaded at all.
//
// Dropout: the pair index stays in PADDED coordinates, ((b*nh + h)*S + q) * (S/2) + key/2 in wrapping uint32.
// D = rowsum(dO * O): fp32 workspace [nh, T_alloc]; the dQ launch writes the rows below n, the dKV launch reads them,
// so the launch order is dQ, then dKV.  dbias (optional): per-wave column sums, combined over the workgroup in the
// idle ring, one atomic per column and workgroup.  No atomics on dqkv.
#include "dtg/common.h"
#include "dtg/kernels.h"
#include "dtg/attn_causal_common.cuh"
#include "dtg/mfma_gemm.cuh"

namespace dtg {
using namespace gemm;
using namespace attn;

namespace {
constexpr size_t kLdsQ = (size_t)kRing * kSlot + kNW * kScr;            // forward, dQ: 48.0 KiB
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
  const int qi = lane & 15;
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
        fwd_chunk<0, false>(Kt, Kt + kTile, nullptr, scr, qa, m, l, o, kc, q0, lane, scale, th, dscale, seed, prow,
                            false);
      else
        fwd_chunk<1, false>(Kt, Kt + kTile, nullptr, scr, qa, m, l, o, kc, q0, lane, scale, th, dscale, seed, prow,
                            false);
    }
    // chunk kc + 1 has landed and every wave is done with slot cur, which the next iteration refills
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (!active) return;  // (no barrier below this point)
  // the forward epilogue, row-guarded: kept here, not behind fwd_store (see there)
  const int g = lane >> 4;
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
    dq_row_terms<true>(dOg, Og, lse, dwork, vrow, H, q0, n, lane, dd, lq);
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
        dq_chunk<0, false>(kt, kt + kTile, nullptr, scr, qa, da, dq, lq, dd, kc, q0, lane, sl2, th, dscale, seed,
                           prow, false);
      else
        dq_chunk<1, false>(kt, kt + kTile, nullptr, scr, qa, da, dq, lq, dd, kc, q0, lane, sl2, th, dscale, seed,
                           prow, false);
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
  if (dbias) dq_dbias(ring, dq, scale, active, dbias, H, h, wave, lane, tid);  // (kernel argument: uniform)
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
      const float no_mask[4] = {};
      dkv_chunk<false, false, true>(Qt, Qt + kTile, Ls, Ls + 64, scr, scr + 1024, ka0, ka1, va0, va1, no_mask, dk, dv,
                                    c, kb, n, bh, S, lane, sl2, th, dscale, seed, c * 64 < kb + 15,
                                    c * 64 + 63 >= n);
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
  if (dbias) dkv_dbias(ring, dk, dv, scale, has_keys, dbias, H, h, wave, lane, tid);  // (kernel argument: uniform)
}

int attn_packed_causal_supported(int S, int dh) { return dh == 64 && S >= 64 && S % 64 == 0 && S <= kStreamMaxS; }

void attn_packed_causal_fwd(const bf16_t* qkv, const int* cu, bf16_t* out, float* lse, int B, int S, int nh,
                            long long T_alloc, float p, uint32_t seed, hipStream_t st) {
  if (B <= 0) return;
  const DropArgs d = drop_args(p);
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  hipLaunchKernelGGL(attn_pcausal_fwd_kernel, grid, dim3(64 * kNW), kLdsQ, st, qkv, cu, out, lse, B, S, nh,
                     (int)T_alloc, 0.125f, d.th, d.dscale, seed, attn_causal_heavy_first_get()); DTG_LAUNCH_CHECK();
}

void attn_packed_causal_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* dout, const float* lse, const int* cu,
                            bf16_t* dqkv, float* dwork, int B, int S, int nh, long long T_alloc, float p,
                            uint32_t seed, float* dbias, hipStream_t st) {
  if (B <= 0) return;
  const DropArgs d = drop_args(p);
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  const int heavy = attn_causal_heavy_first_get();
  // dQ first: it writes D = rowsum(dO * O) into dwork, which dKV reads.  The heaviest blocks first: the record's last
  // query blocks in dQ, its first key blocks in dKV.
  hipLaunchKernelGGL(attn_pcausal_dq_kernel, grid, dim3(64 * kNW), kLdsQ, st, qkv, o, dout, lse, cu, dqkv, dwork, B, S,
                     nh, (int)T_alloc, 0.125f, d.th, d.dscale, seed, dbias, heavy); DTG_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_pcausal_dkv_kernel, grid, dim3(64 * kNW), kLds, st, qkv, dout, lse, cu, dqkv, dwork, B, S,
                     nh, (int)T_alloc, 0.125f, d.th, d.dscale, seed, dbias, !heavy); DTG_LAUNCH_CHECK();
}

}  // namespace dtg
