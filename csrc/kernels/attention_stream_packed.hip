// Streaming fused attention on PACKED token rows for 512 < S <= kStreamMaxS (dtg/kernels.h): head dim 64, bf16, the
// length as mask, pair-hash dropout.  The schedule is attention_stream.hip's (grid [B*nh, ceil(S/128)], 8 waves, the
// streamed operand in 64-row chunks through a 2-slot LDS ring, chunk c + 1's LDS-DMA in flight under chunk c's MFMAs,
// one barrier per chunk, all 8 waves stage and meet at every barrier); the addressing is attention_packed.hip's: qkv
// [T_alloc, 3H], ctx [T_alloc, H], dQKV [T_alloc, 3H] through cu, with that file's record geometry (record_rows: no
// row outside [0, T_alloc) is read or written), its LSE layout (fp32 [nh, T_alloc], lse[h * T_alloc + base + q]) and
// its tail rule (the last record's block-0 workgroups zero the rows cu[B] .. T_alloc - 1 before they test n).
//
// What the length removes, against the padded kernels on the re-padded operands:
//   * a workgroup whose 128 queries (forward, dQ) / keys (dKV) start at or beyond n leaves before its first barrier;
//   * the chunk loops run over ceil(n/64) chunks, not S/64 (ring parity as before: chunk c sits in slot c & 1);
//   * a wave whose 16 rows start at or beyond n stays in the loop and only skips the arithmetic.
// There is no mask operand and no per-chunk mask vector in LDS: a key >= n of the last visited chunk gets kMasked from
// its index.  Operand rows at or beyond n are never loaded: KC tiles and register fragments read row n - 1 instead
// (DenseKC<true>, gfrag_clamp), MC tiles the zero page (DenseMC<true>); the LSE / D values that travel with a dKV
// chunk are clamped to the record's rows.  A query >= n has dropout(P) and dS forced to 0, so every accumulator row
// >= n of dQ / dK / dV is exactly zero: it is not stored (every 16-row store is guarded by row -- the next record's
// first row is the very next packed row) and the dbias column sums over a wave's 16 rows are the record's.
// On the real rows the chunks are visited in the padded kernels' order with their arithmetic, and what is skipped,
// clamped or forced added exact zeros there (the argument at the head of attention_packed.hip), so ctx, LSE and dQKV
// equal attn_stream_* on the re-padded operands.
//
// D = rowsum(dO * O): fp32 workspace [nh, T_alloc], addressed like the LSE; the dQ launch writes the rows below n,
// the dKV launch reads them, so the launch order is dQ, then dKV.
// Dropout: the pair index stays in PADDED coordinates, ((b*nh + h)*S + q)*(S/2) + key/2 in wrapping uint32 (the head
// of attention_stream.hip), so the packed and the padded path drop the same probabilities.
// dbias (optional): per-wave column sums, combined over the workgroup in the idle ring, one atomic per column and
// workgroup.  No atomics on dqkv.
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
constexpr size_t kLdsQ = (size_t)kRing * kSlot + kNW * kScr;           // forward, dQ: 48.0 KiB
constexpr size_t kLdsKV = (size_t)kRing * (kSlot + kVec) + kNW * kScr;  // dKV: 49.0 KiB; three workgroups per CU
constexpr float kLog2e = 1.4426950408889634f;
}  // namespace

// ---------------------------------------------------------------------------------------------
// Forward: a wave owns 16 queries; ring slots {K as KC tile | V as MC tile} (attn_stream_fwd_kernel's transposed form).
__global__ void __launch_bounds__(64 * kNW) attn_pstream_fwd_kernel(const bf16_t* __restrict__ qkv,
                                                                    const int* __restrict__ cu,
                                                                    bf16_t* __restrict__ out, float* __restrict__ lse,
                                                                    int B, int S, int nh, int T_alloc, float scale,
                                                                    uint32_t th, float dscale, uint32_t seed) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (b == B - 1 && blockIdx.y == 0) zero_tail(out, H, h * 64, 1, 0, cu, B, T_alloc, tid, 64 * kNW);
  int base, n;
  record_rows(cu, b, S, T_alloc, base, n);
  if ((int)blockIdx.y * kBlk >= n) return;  // uniform, before any barrier (n = 0 included)
  const bf16_t* Qg = qkv + (long long)base * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  lds_char* ring = smem;                                // kRing x {K KC | V MC}
  lds_char* scr = smem + kRing * kSlot + wave * kScr;   // per-wave [16][64] bf16
  const int nkc = (n + 63) >> 6;                        // key chunks the record has
  const DenseKC<true> ks_{Kg, ld, n, 64};               // rows >= n: row n - 1
  const DenseMC<true> vs_{Vg, ld, 64, n};               // rows >= n: the zero page
  const int q0 = blockIdx.y * kBlk + wave * 16;
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
  // lane (q = lane & 15, g = lane >> 4): one query against keys j * 16 + 4g + [0, 4) of each 16-key block j
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
    if (active) {
      const lds_char* Kt = ring + cur * kSlot;
      const lds_char* Vt = Kt + kTile;
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
        const int key0 = kc * 64 + j * 16 + 4 * g;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[j][r] = fmaf(s[j][r], scale, key0 + r < n ? 0.f : kMasked);
          mx = fmaxf(mx, s[j][r]);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // every visited chunk has a real key (64 * kc < n), so mx is a real score and a masked key has P = 0
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
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_mc<64>(Vt, j * 16, 0, lane), pb0, o[j], 0, 0, 0);
        o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_mc<64>(Vt, j * 16, 1, lane), pb1, o[j], 0, 0, 0);
      }
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
// dQ: a wave owns 16 queries; ring slots {K | V}, both KC (attn_stream_dq_kernel's transposed form).  The wave's Q /
// dO fragments and its O / LSE rows are clamped to row n - 1; D of the rows below n is written to the workspace.
__global__ void __launch_bounds__(64 * kNW) attn_pstream_dq_kernel(const bf16_t* __restrict__ qkv,
                                                                   const bf16_t* __restrict__ o,
                                                                   const bf16_t* __restrict__ dout,
                                                                   const float* __restrict__ lse,
                                                                   const int* __restrict__ cu,
                                                                   bf16_t* __restrict__ dqkv, float* __restrict__ dwork,
                                                                   int B, int S, int nh, int T_alloc, float scale,
                                                                   uint32_t th, float dscale, uint32_t seed,
                                                                   float* __restrict__ dbias) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (b == B - 1 && blockIdx.y == 0) zero_tail(dqkv, ld, h * 64, 1, 0, cu, B, T_alloc, tid, 64 * kNW);
  int base, n;
  record_rows(cu, b, S, T_alloc, base, n);
  if ((int)blockIdx.y * kBlk >= n) return;  // uniform, before any barrier (n = 0 included)
  const bf16_t* Qg = qkv + (long long)base * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* Og = o + (long long)base * H + h * 64;
  const bf16_t* dOg = dout + (long long)base * H + h * 64;
  const long long vrow = (long long)h * T_alloc + base;  // the record's LSE / D values
  lds_char* ring = smem;                                // kRing x {K KC | V KC}
  lds_char* scr = smem + kRing * kSlot + wave * kScr;   // dS [16 q][64 keys] KC
  const int nkc = (n + 63) >> 6;
  const DenseKC<true> ks_{Kg, ld, n, 64};               // rows >= n: row n - 1
  const DenseKC<true> vs_{Vg, ld, n, 64};
  const int q0 = blockIdx.y * kBlk + wave * 16;
  const bool active = q0 < n;  // wave-uniform
  const int qi = lane & 15, g = lane >> 4;
  const bool qreal = q0 + qi < n;
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
    lq = lse[vrow + (qreal ? q0 + qi : n - 1)] * kLog2e;
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
    if (active) {
      const lds_char* kt = ring + cur * kSlot;
      const lds_char* vt = kt + kTile;
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
          const float mk = (key0 + r < n ? 0.f : kMasked) * kLog2e;
          const float p = __builtin_amdgcn_exp2f(fmaf(s[j][r], sl2, mk - lq));
          float dpv = dp[j][r];
          if (th) dpv = kp[r] ? dpv * dscale : 0.f;
          dsv[r] = qreal ? p * (dpv - dd) : 0.f;
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
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (active) store_rows16_n(scr, dq, scale, dqkv + ((long long)base + q0) * ld + h * 64, ld, lane, n - q0);
  if (dbias) {  // (kernel argument: uniform) the ring is idle after the loop's last barrier
    lds_float* bsum = reinterpret_cast<lds_float*>(ring);
    float sq[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) colsum16(dq, scale, sq);  // rows >= n are exactly zero
    if (lane < 16)
#pragma unroll
      for (int j = 0; j < 4; ++j) bsum[wave * 64 + j * 16 + lane] = sq[j];
    dbias_reduce<64, kNW>(bsum, dbias, 0, H, h, tid);
  }
}

// ---------------------------------------------------------------------------------------------
// dKV: a wave owns 16 keys whose K / V fragments stay in registers (rows >= n: row n - 1, masked); ring slots
// {Q | dO}, both MC (rows >= n: the zero page), with the chunk's 64 LSE and D values (attn_stream_dkv_kernel's
// chunk body).  D is read from the workspace the dQ launch wrote.
__global__ void __launch_bounds__(64 * kNW) attn_pstream_dkv_kernel(const bf16_t* __restrict__ qkv,
                                                                    const bf16_t* __restrict__ dout,
                                                                    const float* __restrict__ lse,
                                                                    const int* __restrict__ cu,
                                                                    bf16_t* __restrict__ dqkv,
                                                                    const float* __restrict__ dwork, int B, int S,
                                                                    int nh, int T_alloc, float scale, uint32_t th,
                                                                    float dscale, uint32_t seed,
                                                                    float* __restrict__ dbias) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (b == B - 1 && blockIdx.y == 0) zero_tail(dqkv, ld, H + h * 64, 2, H, cu, B, T_alloc, tid, 64 * kNW);
  int base, n;
  record_rows(cu, b, S, T_alloc, base, n);
  if ((int)blockIdx.y * kBlk >= n) return;  // uniform, before any barrier (n = 0 included)
  const bf16_t* Qg = qkv + (long long)base * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* dOg = dout + (long long)base * H + h * 64;
  lds_char* ring = smem;                                                     // kRing x {Q MC | dO MC}
  lds_float* LD = reinterpret_cast<lds_float*>(smem + kRing * kSlot);        // kRing x {64 LSE * log2(e) | 64 D}
  lds_char* scr = smem + kRing * (kSlot + kVec) + wave * kScr;               // [32 q][16 keys] x {P, dS}
  const int nqc = (n + 63) >> 6;                        // query chunks the record has
  const DenseMC<true> qs_{Qg, ld, 64, n};               // rows >= n: the zero page
  const DenseMC<true> ds_{dOg, (long long)H, 64, n};
  // threads 0-63 carry the chunk's LSE, 64-127 its D; a query >= n reads row n - 1's (unused: its dS is forced to 0)
  const float* vsrc = (tid < 64 ? lse : dwork) + (long long)h * T_alloc + base;
  const float vmul = tid < 64 ? kLog2e : 1.f;
  const int vq = tid & 63;
  const int kb = blockIdx.y * kBlk + wave * 16;
  const bool has_keys = kb < n;  // wave-uniform
  const int rbase = (lane >> 4) * 4;
  float msl[4] = {0.f, 0.f, 0.f, 0.f};
  v8bf ka0, ka1, va0, va1;
  if (has_keys) {
#pragma unroll
    for (int r = 0; r < 4; ++r) msl[r] = (kb + rbase + r < n ? 0.f : kMasked) * kLog2e;
    ka0 = gfrag_clamp(Kg, ld, kb, n, 0, lane), ka1 = gfrag_clamp(Kg, ld, kb, n, 1, lane);
    va0 = gfrag_clamp(Vg, ld, kb, n, 0, lane), va1 = gfrag_clamp(Vg, ld, kb, n, 1, lane);
  }
  stage_mc<64, DenseMC<true>, kNW>(qs_, ring, 0, 0, wave, lane);
  stage_mc<64, DenseMC<true>, kNW>(ds_, ring + kTile, 0, 0, wave, lane);
  if (tid < 128) LD[tid] = vsrc[vq < n ? vq : n - 1] * vmul;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const float sl2 = scale * kLog2e;
  lds_char* scp = scr;
  lds_char* scs = scr + 1024;
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dk[j] = dv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = 0; c < nqc; ++c) {
    const int cur = c & 1, nxt = cur ^ 1;
    const bool more = c + 1 < nqc;
    float vnext = 0.f;
    if (more) {
      stage_mc<64, DenseMC<true>, kNW>(qs_, ring + nxt * kSlot, 0, (c + 1) * 64, wave, lane);
      stage_mc<64, DenseMC<true>, kNW>(ds_, ring + nxt * kSlot + kTile, 0, (c + 1) * 64, wave, lane);
      const int q = (c + 1) * 64 + vq;
      if (tid < 128) vnext = vsrc[q < n ? q : n - 1] * vmul;
    }
    if (has_keys) {
      const lds_char* Qt = ring + cur * kSlot;
      const lds_char* dOt = Qt + kTile;
      const lds_float* Ls = LD + cur * 128;
      const lds_float* Ds = Ls + 64;
#pragma unroll
      for (int kq = 0; kq < 2; ++kq) {  // 32-query halves of the chunk
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
          const bool qreal = q < n;
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
            pd[r] = qreal ? pv : 0.f;
            dsv[r] = qreal ? p * (dp - dq) : 0.f;
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
    if (tid < 128 && more) LD[nxt * 128 + tid] = vnext;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (has_keys) {  // rows >= n of dk / dv are exactly zero: a masked key has P = 0
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

int attn_packed_stream_supported(int S, int dh) { return dh == 64 && S % 64 == 0 && S > 512 && S <= kStreamMaxS; }

void attn_packed_stream_fwd(const bf16_t* qkv, const int* cu, bf16_t* out, float* lse, int B, int S, int nh,
                            long long T_alloc, float p, uint32_t seed, hipStream_t st) {
  if (B <= 0) return;
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  hipLaunchKernelGGL(attn_pstream_fwd_kernel, grid, dim3(64 * kNW), kLdsQ, st, qkv, cu, out, lse, B, S, nh,
                     (int)T_alloc, 0.125f, th, ds, seed); DTG_LAUNCH_CHECK();
}

void attn_packed_stream_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* dout, const float* lse, const int* cu,
                            bf16_t* dqkv, float* dwork, int B, int S, int nh, long long T_alloc, float p,
                            uint32_t seed, float* dbias, hipStream_t st) {
  if (B <= 0) return;
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  // dQ first: it writes D = rowsum(dO * O) into dwork, which dKV reads
  hipLaunchKernelGGL(attn_pstream_dq_kernel, grid, dim3(64 * kNW), kLdsQ, st, qkv, o, dout, lse, cu, dqkv, dwork, B, S,
                     nh, (int)T_alloc, 0.125f, th, ds, seed, dbias); DTG_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_pstream_dkv_kernel, grid, dim3(64 * kNW), kLdsKV, st, qkv, dout, lse, cu, dqkv, dwork, B, S,
                     nh, (int)T_alloc, 0.125f, th, ds, seed, dbias); DTG_LAUNCH_CHECK();
}

}  // namespace dtg
