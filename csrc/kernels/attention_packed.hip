// Fused attention on PACKED token rows (head dim 64): the forward and the one-launch backward of attention.hip at
// S in {64, 128}, and at 128 < S <= 512 (S % 64 == 0) the same forward over ceil(S/128) query blocks with the dKV + dQ
// backward pair (the "long" entry points at the end of the file), reading qkv [T_alloc, 3H] and writing ctx
// [T_alloc, H] / dQKV [T_alloc, 3H] addressed through cu (ops/seqpack.py) -- no re-padding copies around the kernels,
// and no work on [PAD] key chunks or query blocks.
//
// Geometry of record b (the convention of seqpack.hip: no row outside [0, T_alloc) is read or written):
//   base = cu[b],  n = clamp(cu[b+1] - cu[b], 0, min(S, T_alloc - base));  base outside [0, T_alloc): n = 0.
//   n = 0: the record's workgroups leave before their first barrier and write nothing.
// There is no mask operand: the length is the mask.  A key >= n inside a visited chunk gets the additive -10000 that
// mask_additive gives a [PAD] key; operand rows at or beyond n are never loaded (row index clamped to n - 1 for
// register fragments and KC tiles, the zero page for MC tiles).  The dropout index stays in PADDED coordinates
// ((b*nh + h)*S + q)*S + key, so the packed and the padded path drop the same probabilities.
// On the real rows the results are those of the padded kernels, bit for bit: a skipped all-masked key chunk has
// alpha = exp(0) = 1 and adds P = 0; a masked key in a visited chunk has P = exp(x - 10000 - m) = 0 in fp32 whatever
// finite row was loaded for it; a query >= n has dropout(P) and dS forced to 0, where the padded path has dO = 0.
// LSE: fp32 [nh, T_alloc], lse[h * T_alloc + base + q].
// Tail rows cu[B] .. T_alloc - 1 belong to no record: the workgroups of the LAST record write zeros there (their
// head's columns) before anything else, so every row of [0, T_alloc) is written exactly once per call and the GEMMs
// that read ctx / dQKV over all T_alloc rows never see an uninitialised row.
#include "dtg/common.h"
#include "dtg/kernels.h"
#include "dtg/attn_common.cuh"
#include "dtg/mfma_gemm.cuh"

namespace dtg {
using namespace gemm;
using namespace attn;

namespace {

constexpr int kWaves = 8;
constexpr float kMasked = -10000.f;  // mask_additive's value of a [PAD] key

// (base, n) of record b, uniform over the workgroup
__device__ __forceinline__ void record_rows(const int* __restrict__ cu, int b, int S, int T_alloc, int& base, int& n) {
  base = cu[b];
  int len = cu[b + 1] - base;
  len = len < S ? len : S;
  const bool inside = base >= 0 && base < T_alloc;
  const int room = inside ? T_alloc - base : 0;
  len = len < room ? len : room;
  n = len > 0 ? len : 0;
  if (!inside) base = 0;
}

// zeros on columns [col0, col0 + 64) (x nseg segments, seg_stride apart) of the rows cu[B] .. T_alloc - 1
__device__ __forceinline__ void zero_tail(bf16_t* dst, long long ldd, int col0, int nseg, int seg_stride,
                                          const int* __restrict__ cu, int B, int T_alloc, int tid, int nthreads) {
  int t0 = cu[B];
  t0 = t0 < 0 ? 0 : (t0 < T_alloc ? t0 : T_alloc);
  const int per_row = nseg * 8;  // 16-byte chunks of a row
  const long long total = (long long)(T_alloc - t0) * per_row;
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4v;
  const u32x4v z = {0u, 0u, 0u, 0u};
  for (long long i = tid; i < total; i += nthreads) {
    const long long row = t0 + i / per_row;
    const int c = (int)(i % per_row);
    *reinterpret_cast<u32x4v*>(dst + row * ldd + col0 + (c >> 3) * seg_stride + (c & 7) * 8) = z;
  }
}

// ---------------------------------------------------------------------------------------------
// Forward: grid [B*nh, ceil(S/128)], 8 waves, a wave owns 16 queries (attn_fwd_kernel's schedule; see there).
__global__ void __launch_bounds__(64 * kWaves) attn_packed_fwd_kernel(const bf16_t* __restrict__ qkv,
                                                                      const int* __restrict__ cu,
                                                                      bf16_t* __restrict__ out, float* __restrict__ lse,
                                                                      int B, int S, int nh, int T_alloc, float scale,
                                                                      uint32_t th, float dscale, uint32_t seed) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b == B - 1 && blockIdx.y == 0) zero_tail(out, H, h * 64, 1, 0, cu, B, T_alloc, threadIdx.x, 64 * kWaves);
  int base, n;
  record_rows(cu, b, S, T_alloc, base, n);
  if ((int)blockIdx.y * (16 * kWaves) >= n) return;  // uniform, before any barrier (n = 0 included)
  const bf16_t* Qg = qkv + (long long)base * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  lds_char* Kt = smem;                      // [S][64] KC
  lds_char* Vt = smem + S * 128;            // S/64 MC tiles [64 keys][64 d]
  lds_char* scr = smem + 2 * S * 128 + wave * 2048;  // per-wave [16][64] bf16
  const int nkc = (n + 63) >> 6;  // key chunks the record has
  {
    DenseKC<true> ks_{Kg, ld, n, 64};   // rows >= n: row n - 1
    DenseMC<true> vs_{Vg, ld, 64, n};   // rows >= n: the zero page
    for (int c = 0; c < nkc; ++c) {
      stage_kc<64, DenseKC<true>, kWaves>(ks_, Kt + c * 8192, c * 64, 0, wave, lane);
      stage_mc<64, DenseMC<true>, kWaves>(vs_, Vt + c * 8192, 0, c * 64, wave, lane);
    }
  }
  const int q0 = blockIdx.y * (16 * kWaves) + wave * 16;
  const bool active = q0 < n;
  v8bf qa[2];
  if (active) {
    qa[0] = gfrag_clamp(Qg, ld, q0, n, 0, lane);
    qa[1] = gfrag_clamp(Qg, ld, q0, n, 1, lane);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (!active) return;  // (no barrier below this point)
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int qi = lane & 15, g = lane >> 4;
  const uint32_t qrow = ((uint32_t)bh * (uint32_t)S + (uint32_t)(q0 + qi)) * (uint32_t)S;  // padded coordinates
  for (int kc = 0; kc < nkc; ++kc) {
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_kc(Kt + kc * 8192, j * 16, ks, lane), qa[ks], s[j], 0, 0, 0);
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
        const uint32_t pidx = (qrow + (uint32_t)key0) >> 1;
        const uint32_t h0 = pair_hash(seed, pidx), h1 = pair_hash(seed, pidx + 1u);
        pd[0] = (h0 & 0xffffu) >= th ? pd[0] * dscale : 0.f;
        pd[1] = (h0 >> 16) >= th ? pd[1] * dscale : 0.f;
        pd[2] = (h1 & 0xffffu) >= th ? pd[2] * dscale : 0.f;
        pd[3] = (h1 >> 16) >= th ? pd[3] * dscale : 0.f;
      }
      st4_bf16(scr + kc_off(qi, j * 16 + 4 * g), pd);  // P [16 q][64 keys] KC: 4 keys in one 16-B chunk
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
      o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_mc<64>(Vt + kc * 8192, j * 16, 0, lane), pb0, o[j], 0, 0, 0);
      o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_mc<64>(Vt + kc * 8192, j * 16, 1, lane), pb1, o[j], 0, 0, 0);
    }
    lds_fence();  // the scratch is rewritten by the next chunk
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float il = 1.f / l;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v[4] = {o[j][0] * il, o[j][1] * il, o[j][2] * il, o[j][3] * il};
    st4_bf16(scr + qi * 128 + (((2 * j + (g >> 1)) ^ (qi & 7)) << 4) + (g & 1) * 8, v);
  }
  // a lane group's 16 queries are contiguous in [nh, T_alloc]; queries >= n (clamped copies of row n - 1) stay here
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
// Backward: one workgroup (8 waves) per (b, h), attn_bwd_kernel's two phases (see there) over the record's rows.
//   n32 = n rounded up to 32: phase 1 runs the 32-query chunks below n32 on the key waves below n32; phase 2 reads
//   dS over the keys below n32 only.  Inside that square every entry of dS is written: a query >= n has dropout(P)
//   and dS forced to exactly 0 (its Q / dO rows are the zero page, its LSE and D are taken as 0), a key >= n has
//   P = exp2(x - 10000 log2(e) - lse) = 0 and with it dS = 0 (its K / V rows are finite copies of row n - 1).  So
//   every accumulator row >= n of dQ / dK / dV is exactly zero: it is not stored, and the dbias column sums over
//   the wave's 16 rows are the sums over the record's rows.  Key waves at or beyond n32 only meet the barriers.
template <int S_>
__global__ void __launch_bounds__(512) attn_packed_bwd_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o,
                                                              const bf16_t* __restrict__ dout,
                                                              const float* __restrict__ lse, const int* __restrict__ cu,
                                                              bf16_t* __restrict__ dqkv, int B, int nh, int T_alloc,
                                                              float scale, uint32_t th, float dscale, uint32_t seed,
                                                              float* __restrict__ dbias) {
  constexpr int S = S_, NW = kWaves;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (b == B - 1) zero_tail(dqkv, ld, h * 64, 3, H, cu, B, T_alloc, tid, 64 * NW);
  int base, n;
  record_rows(cu, b, S, T_alloc, base, n);
  if (n == 0) return;  // uniform, before any barrier
  const int n32 = (n + 31) & ~31;
  const bf16_t* Qg = qkv + (long long)base * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* Og = o + (long long)base * H + h * 64;
  const bf16_t* dOg = dout + (long long)base * H + h * 64;
  lds_char* Qt = smem;                         // MC [q][d]; phase 2: K as MC [key][d]
  lds_char* dOt = Qt + S * 128;                // MC [q][d]; phase 2: per-wave output staging
  lds_char* Kt = Qt;
  lds_char* dSq = dOt + S * 128;               // dS [S q][S key] bf16, MC-swizzled rows
  lds_float* Ds = reinterpret_cast<lds_float*>(dSq + S * S * 2);
  lds_float* Ls = Ds + S;
  lds_char* scr0 = reinterpret_cast<lds_char*>(Ls + S);
  lds_char* scr = scr0 + wave * 1024;          // [32 q][16 keys]
  {
    DenseMC<true> qs_{Qg, ld, 64, n};          // rows >= n: the zero page
    DenseMC<true> ds_{dOg, (long long)H, 64, n};
#pragma unroll
    for (int c = 0; c < S / 64; ++c) {
      if (c * 64 < n) {
        stage_mc<64, DenseMC<true>, NW>(qs_, Qt + c * 8192, 0, c * 64, wave, lane);
        stage_mc<64, DenseMC<true>, NW>(ds_, dOt + c * 8192, 0, c * 64, wave, lane);
      }
    }
  }
  if (tid < 2 * S) {  // D[q] = sum_d dO[q, d] * O[q, d]: two threads per row; 0 for q >= n
    const int q = tid >> 1, half = tid & 1;
    float acc = 0.f;
    if (q < n) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float a[8], bb[8];
        load8_bf16(dOg + (long long)q * H + half * 32 + c * 8, a);
        load8_bf16(Og + (long long)q * H + half * 32 + c * 8, bb);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += a[k] * bb[k];
      }
    }
    acc += __shfl_xor(acc, 1, 64);
    if (half == 0) Ds[q] = acc;
  }
  if (tid < S) Ls[tid] = tid < n ? lse[(long long)h * T_alloc + base + tid] : 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int rbase = (lane >> 4) * 4;
  const int kb = wave * 16;
  const bool has_keys = kb < n32;
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dk[j] = dv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (has_keys) {
    constexpr float kLog2e = 1.4426950408889634f;
    // the lane's 4 keys are fixed for the whole pass: their mask terms (base-2 units) live in registers
    float msl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) msl[r] = (kb + rbase + r < n ? 0.f : kMasked) * kLog2e;
    const float sl2 = scale * kLog2e;
    const v8bf ka0 = gfrag_clamp(Kg, ld, kb, n, 0, lane), ka1 = gfrag_clamp(Kg, ld, kb, n, 1, lane);
    const v8bf va0 = gfrag_clamp(Vg, ld, kb, n, 0, lane), va1 = gfrag_clamp(Vg, ld, kb, n, 1, lane);
#pragma unroll 1
    for (int qc = 0; qc < n32; qc += 32) {
      const int tq = qc >> 6, kq = (qc & 63) >> 5;
      f32x4 st[2], dpt[2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int qrow = (qc & 63) + ni * 16 + (lane & 15), cb = lane >> 4;
        const int sw = mc_swz<8>(qrow);
        const lds_char* qt = Qt + tq * 8192 + qrow * 128;
        const lds_char* dt = dOt + tq * 8192 + qrow * 128;
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
        const int ql = ni * 16 + (lane & 15), q = qc + ql;
        const bool qreal = q < n;
        const float lq = Ls[q] * kLog2e, dq = Ds[q];
        const uint32_t ib = ((uint32_t)bh * (uint32_t)S + (uint32_t)q) * (uint32_t)S + (uint32_t)(kb + rbase);
        float pd[4], dsv[4];
        bool kp[4] = {true, true, true, true};
        if (th) keep4_attn(seed, ib, th, kp);  // ib even: kb + rbase is a multiple of 4
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
        st4_bf16(scr + ql * 32 + rbase * 2, pd);
        const int key0 = kb + rbase;
        st4_bf16(dSq + q * (S * 2) + ((((key0 >> 3) ^ mc_swz<S / 8>(q))) << 4) + (key0 & 7) * 2, dsv);
      }
      lds_fence();
      const v8bf pa = frag_mc<16>(scr, 0, 0, lane);        // dropout(P)^T [16 keys][32 q]
      const v8bf sa = frag_mc<S>(dSq, kb, qc >> 5, lane);   // dS^T [16 keys][32 q]
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dv[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, frag_mc<64>(dOt + tq * 8192, j * 16, kq, lane), dv[j], 0,
                                                        0, 0);
        dk[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sa, frag_mc<64>(Qt + tq * 8192, j * 16, kq, lane), dk[j], 0,
                                                        0, 0);
      }
      lds_fence();  // scratch rewritten by the next chunk
    }
  }
  __syncthreads();  // dS complete; the Q / dO tiles are free
  {  // K for dQ = dS K into the Q tile: its DMA is in flight while dK / dV are stored
    DenseMC<true> kss{Kg, ld, 64, n};
#pragma unroll
    for (int c = 0; c < S / 64; ++c)
      if (c * 64 < n) stage_mc<64, DenseMC<true>, NW>(kss, Kt + c * 8192, 0, c * 64, wave, lane);
  }
  lds_char* stg = dOt + wave * 2048;  // per-wave output staging inside the dO tile (16 or 32 KB)
  lds_float* bsum = reinterpret_cast<lds_float*>(scr);  // the wave's [dQ | dK | dV] column sums
  if (dbias) {
    float sk[4] = {0.f, 0.f, 0.f, 0.f}, sv[4] = {0.f, 0.f, 0.f, 0.f};
    if (has_keys) {
      colsum16(dk, scale, sk);
      colsum16(dv, 1.f, sv);
    }
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bsum[64 + j * 16 + lane] = sk[j];
        bsum[128 + j * 16 + lane] = sv[j];
      }
    }
  }
  if (kb < n) {
    bf16_t* gk = dqkv + ((long long)base + kb) * ld + H + h * 64;
    store_rows16_n(stg, dk, scale, gk, ld, lane, n - kb);
    store_rows16_n(stg, dv, 1.f, gk + H, ld, lane, n - kb);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // K staged by every wave
  const int qr = wave * 16;
  if (qr < n) {
    f32x4 dq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) dq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int qa_ = qr + (lane & 15);
#pragma unroll
    for (int kk = 0; kk < S / 32; ++kk) {
      if (kk * 32 < n) {
        const int c = kk * 4 + (lane >> 4);
        const v8bf a = *reinterpret_cast<const lds_v8bf*>(dSq + qa_ * (S * 2) + ((c ^ mc_swz<S / 8>(qa_)) << 4));
#pragma unroll
        for (int j = 0; j < 4; ++j)
          dq[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, frag_mc<64>(Kt + (kk >> 1) * 8192, j * 16, kk & 1, lane),
                                                          dq[j], 0, 0, 0);
      }
    }
    store_rows16_n(stg, dq, scale, dqkv + ((long long)base + qr) * ld + h * 64, ld, lane, n - qr);
    if (dbias) {
      float sq[4];
      colsum16(dq, scale, sq);
      if (lane < 16)
#pragma unroll
        for (int j = 0; j < 4; ++j) bsum[j * 16 + lane] = sq[j];
    }
  } else if (dbias && lane < 16) {
#pragma unroll
    for (int j = 0; j < 4; ++j) bsum[j * 16 + lane] = 0.f;
  }
  if (dbias) {  // (kernel argument: uniform) 8 wave partials -> one atomic per column
    __syncthreads();
    if (tid < 192) {
      const int part = tid >> 6, c = tid & 63;
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += reinterpret_cast<lds_float*>(scr0)[w * 256 + tid];
      atomicAdd(dbias + part * H + h * 64 + c, t);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Backward at 128 < S <= 512: attention.hip's dKV + dQ pair (see there) over the record's rows, grid [B*nh,
// ceil(S/128)] each.  A workgroup whose 128 keys (dKV) / queries (dQ) start at or beyond n leaves before its first
// barrier.  The chunk order, the MFMA operand roles and the D summation are those of the padded kernels, and what is
// skipped or clamped adds exact zeros there (file header), so the real rows carry the padded kernels' bits.
// Accumulator rows >= n are exactly zero in both kernels -- dKV: a key >= n has P = exp2(x - 10000 log2(e) - lse) = 0
// for every real query (the record has a real key, so lse is within the scores' range) and a query >= n has
// dropout(P) and dS forced to 0; dQ: a query >= n has dS forced to 0 -- so they are not stored, and the dbias column
// sums over a wave's 16 rows (one atomic per column and wave, as in the padded pair) are sums over the record's rows.
constexpr int kLongRows = 128;  // keys (dKV) / queries (dQ) per workgroup

// dKV: wave w owns keys 128*y + 16w + [0, 16) and runs the 32-query chunks below n32 = roundup(n, 32); Q / dO rows
// >= n are the zero page, their LSE and D are taken as 0.  Waves whose keys start at or beyond n32 only meet the
// barriers.  The last record's y = 0 workgroups zero the K and V segments of the tail rows.
__global__ void __launch_bounds__(512) attn_packed_bwd_dkv_kernel(const bf16_t* __restrict__ qkv,
                                                                  const bf16_t* __restrict__ o,
                                                                  const bf16_t* __restrict__ dout,
                                                                  const float* __restrict__ lse,
                                                                  const int* __restrict__ cu, bf16_t* __restrict__ dqkv,
                                                                  int B, int S, int nh, int T_alloc, float scale,
                                                                  uint32_t th, float dscale, uint32_t seed,
                                                                  float* __restrict__ dbias) {
  constexpr int NW = kWaves;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (b == B - 1 && blockIdx.y == 0) zero_tail(dqkv, ld, H + h * 64, 2, H, cu, B, T_alloc, tid, 64 * NW);
  int base, n;
  record_rows(cu, b, S, T_alloc, base, n);
  if ((int)blockIdx.y * kLongRows >= n) return;  // uniform, before any barrier (n = 0 included)
  const int n32 = (n + 31) & ~31, n64 = (n + 63) & ~63;  // n64 <= S: S % 64 == 0
  const bf16_t* Qg = qkv + (long long)base * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* Og = o + (long long)base * H + h * 64;
  const bf16_t* dOg = dout + (long long)base * H + h * 64;
  lds_char* Qt = smem;                          // S/64 MC tiles [64 q][64 d], those below n staged
  lds_char* dOt = Qt + S * 128;                 // same for dO; after the loop: per-wave output staging
  lds_float* Ds = reinterpret_cast<lds_float*>(dOt + S * 128);
  lds_float* Ls = Ds + S;
  lds_char* scr = reinterpret_cast<lds_char*>(Ls + S) + wave * 2048;  // [32 q][16 keys] x {P, dS}
  const int kb = blockIdx.y * kLongRows + wave * 16;
  const bool has_keys = kb < n32;  // wave-uniform
  const int rbase = (lane >> 4) * 4;
  constexpr float kLog2e = 1.4426950408889634f;
  float msl[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) msl[r] = (kb + rbase + r < n ? 0.f : kMasked) * kLog2e;
  {
    DenseMC<true> qs_{Qg, ld, 64, n};           // rows >= n: the zero page
    DenseMC<true> ds_{dOg, (long long)H, 64, n};
    for (int c = 0; c * 64 < n; ++c) {
      stage_mc<64, DenseMC<true>, NW>(qs_, Qt + c * 8192, 0, c * 64, wave, lane);
      stage_mc<64, DenseMC<true>, NW>(ds_, dOt + c * 8192, 0, c * 64, wave, lane);
    }
  }
  for (int i = tid; i < 2 * n64; i += 64 * NW) {  // D[q] = sum_d dO[q, d] * O[q, d]: two threads per row; 0 for q >= n
    const int q = i >> 1, half = i & 1;
    float acc = 0.f;
    if (q < n) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float a[8], bb[8];
        load8_bf16(dOg + (long long)q * H + half * 32 + c * 8, a);
        load8_bf16(Og + (long long)q * H + half * 32 + c * 8, bb);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += a[k] * bb[k];
      }
    }
    acc += __shfl_xor(acc, 1, 64);
    if (half == 0) Ds[q] = acc;
  }
  for (int i = tid; i < n64; i += 64 * NW) Ls[i] = i < n ? lse[(long long)h * T_alloc + base + i] : 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  f32x4 dk[4], dv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dk[j] = dv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (has_keys) {
    const float sl2 = scale * kLog2e;
    const v8bf ka0 = gfrag_clamp(Kg, ld, kb, n, 0, lane), ka1 = gfrag_clamp(Kg, ld, kb, n, 1, lane);
    const v8bf va0 = gfrag_clamp(Vg, ld, kb, n, 0, lane), va1 = gfrag_clamp(Vg, ld, kb, n, 1, lane);
    lds_char* scp = scr;
    lds_char* scs = scr + 1024;
#pragma unroll 1
    for (int qc = 0; qc < n32; qc += 32) {
      const int tq = qc >> 6, kq = (qc & 63) >> 5;
      f32x4 st[2], dpt[2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int qrow = (qc & 63) + ni * 16 + (lane & 15), cb = lane >> 4;
        const int sw = mc_swz<8>(qrow);
        const lds_char* qt = Qt + tq * 8192 + qrow * 128;
        const lds_char* dt = dOt + tq * 8192 + qrow * 128;
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
        const int ql = ni * 16 + (lane & 15), q = qc + ql;
        const bool qreal = q < n;
        const float lq = Ls[q] * kLog2e, dq = Ds[q];
        const uint32_t ib = ((uint32_t)bh * (uint32_t)S + (uint32_t)q) * (uint32_t)S + (uint32_t)(kb + rbase);
        float pd[4], dsv[4];
        bool kp[4] = {true, true, true, true};
        if (th) keep4_attn(seed, ib, th, kp);  // ib even: kb + rbase is a multiple of 4
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
        dv[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, frag_mc<64>(dOt + tq * 8192, j * 16, kq, lane), dv[j], 0,
                                                        0, 0);
        dk[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sa, frag_mc<64>(Qt + tq * 8192, j * 16, kq, lane), dk[j], 0,
                                                        0, 0);
      }
      lds_fence();  // scratches rewritten by the next chunk
    }
  }
  __syncthreads();  // every wave is done with the Q / dO tiles
  if (kb < n) {
    lds_char* stg = dOt + wave * 2048;
    bf16_t* gk = dqkv + ((long long)base + kb) * ld + H + h * 64;
    store_rows16_n(stg, dk, scale, gk, ld, lane, n - kb);
    store_rows16_n(stg, dv, 1.f, gk + H, ld, lane, n - kb);
    if (dbias) {  // rows >= n of dk / dv are exactly zero (above): the 16-row sums are the record's
      float sk[4], sv[4];
      colsum16(dk, scale, sk);
      colsum16(dv, 1.f, sv);
      if (lane < 16)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          atomicAdd(dbias + H + h * 64 + j * 16 + lane, sk[j]);
          atomicAdd(dbias + 2 * H + h * 64 + j * 16 + lane, sv[j]);
        }
    }
  }
}

// dQ: wave w owns queries 128*y + 16w + [0, 16); K / V as KC tiles for the ceil(n/64) key chunks the record has (rows
// >= n: copies of row n - 1, masked).  The wave's Q / dO fragments and its LSE / D / O rows are clamped to row n - 1:
// no row at or beyond base + n is loaded; a query >= n has dS forced to 0.  Waves with q0 >= n return after the
// barrier.  The last record's y = 0 workgroups zero the Q segment of the tail rows.
__global__ void __launch_bounds__(512) attn_packed_bwd_dq_kernel(const bf16_t* __restrict__ qkv,
                                                                 const bf16_t* __restrict__ o,
                                                                 const bf16_t* __restrict__ dout,
                                                                 const float* __restrict__ lse,
                                                                 const int* __restrict__ cu, bf16_t* __restrict__ dqkv,
                                                                 int B, int S, int nh, int T_alloc, float scale,
                                                                 uint32_t th, float dscale, uint32_t seed,
                                                                 float* __restrict__ dbias) {
  constexpr int NW = kWaves;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (b == B - 1 && blockIdx.y == 0) zero_tail(dqkv, ld, h * 64, 1, 0, cu, B, T_alloc, tid, 64 * NW);
  int base, n;
  record_rows(cu, b, S, T_alloc, base, n);
  if ((int)blockIdx.y * kLongRows >= n) return;  // uniform, before any barrier (n = 0 included)
  const bf16_t* Qg = qkv + (long long)base * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* Og = o + (long long)base * H + h * 64;
  const bf16_t* dOg = dout + (long long)base * H + h * 64;
  lds_char* Kt = smem;                        // S/64 KC tiles [64 keys][64 d], those below n staged
  lds_char* Vt = smem + S * 128;              // same for V
  lds_char* scr = smem + 2 * S * 128 + wave * 2048;  // dS [16 q][64 keys] KC
  const int nkc = (n + 63) >> 6;
  {
    DenseKC<true> ks_{Kg, ld, n, 64};         // rows >= n: row n - 1
    DenseKC<true> vs_{Vg, ld, n, 64};
    for (int c = 0; c < nkc; ++c) {
      stage_kc<64, DenseKC<true>, NW>(ks_, Kt + c * 8192, c * 64, 0, wave, lane);
      stage_kc<64, DenseKC<true>, NW>(vs_, Vt + c * 8192, c * 64, 0, wave, lane);
    }
  }
  constexpr float kLog2e = 1.4426950408889634f;
  const int q0 = blockIdx.y * kLongRows + wave * 16;
  const bool active = q0 < n;  // wave-uniform
  const int rbase = (lane >> 4) * 4;
  v8bf qa[2], da[2];
  float lq[4], dd[4];
  if (active) {
    qa[0] = gfrag_clamp(Qg, ld, q0, n, 0, lane);
    qa[1] = gfrag_clamp(Qg, ld, q0, n, 1, lane);
    da[0] = gfrag_clamp(dOg, (long long)H, q0, n, 0, lane);
    da[1] = gfrag_clamp(dOg, (long long)H, q0, n, 1, lane);
    // D of the wave's 16 rows: 4 lanes per row, 16 d each
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
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + rbase + r;
      dd[r] = __shfl(acc, (rbase + r) * 4, 64);
      lq[r] = lse[(long long)h * T_alloc + base + (q < n ? q : n - 1)] * kLog2e;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (!active) return;  // (no barrier below this point)
  const float sl2 = scale * kLog2e;
  f32x4 dq[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int kc = 0; kc < nkc; ++kc) {
    const lds_char* kt = Kt + kc * 8192;
    const lds_char* vt = Vt + kc * 8192;
    f32x4 s[4], dp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = dp[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ks], frag_kc(kt, j * 16, ks, lane), s[j], 0, 0, 0);
        dp[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[ks], frag_kc(vt, j * 16, ks, lane), dp[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = kc * 64 + j * 16 + (lane & 15);
      const float mk = (key < n ? 0.f : kMasked) * kLog2e;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(s[j][r], sl2, mk - lq[r]));
        float dpv = dp[j][r];
        if (th) {
          const uint32_t idx = ((uint32_t)bh * (uint32_t)S + (uint32_t)(q0 + rbase + r)) * (uint32_t)S + (uint32_t)key;
          dpv = keep_attn(seed, idx, th) ? dpv * dscale : 0.f;
        }
        st_bf16(scr, kc_off(rbase + r, j * 16 + (lane & 15)), q0 + rbase + r < n ? p * (dpv - dd[r]) : 0.f);
      }
    }
    lds_fence();
    const v8bf a0 = frag_kc(scr, 0, 0, lane), a1 = frag_kc(scr, 0, 1, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dq[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, frag_tr_kc(kt, j * 16, 0, lane), dq[j], 0, 0, 0);
      dq[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, frag_tr_kc(kt, j * 16, 1, lane), dq[j], 0, 0, 0);
    }
    lds_fence();  // the scratch is rewritten by the next chunk
  }
  store_rows16_n(scr, dq, scale, dqkv + ((long long)base + q0) * ld + h * 64, ld, lane, n - q0);
  if (dbias) {  // rows >= n of dq are exactly zero (dS forced to 0): the 16-row sums are the record's
    float sq[4];
    colsum16(dq, scale, sq);
    if (lane < 16)
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(dbias + h * 64 + j * 16 + lane, sq[j]);
  }
}

size_t fwd_lds(int S) { return (size_t)2 * S * 128 + kWaves * 2048; }
size_t bwd_lds(int S) { return (size_t)2 * S * 128 + (size_t)S * S * 2 + 2 * S * 4 + 8 * 1024; }
size_t dkv_lds(int S) { return (size_t)2 * S * 128 + (size_t)2 * S * 4 + kWaves * 2048; }
size_t dq_lds(int S) { return (size_t)2 * S * 128 + kWaves * 2048; }

}  // namespace

int attn_packed_supported(int S, int dh) { return dh == 64 && (S == 64 || S == 128); }

void attn_packed_fwd(const bf16_t* qkv, const int* cu, bf16_t* out, float* lse, int B, int S, int nh, long long T_alloc,
                     float p, uint32_t seed, hipStream_t st) {
  if (B <= 0) return;
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  dim3 grid(B * nh, (S + 16 * kWaves - 1) / (16 * kWaves));
  hipLaunchKernelGGL(attn_packed_fwd_kernel, grid, dim3(64 * kWaves), fwd_lds(S), st, qkv, cu, out, lse, B, S, nh,
                     (int)T_alloc, 0.125f, th, ds, seed); DTG_LAUNCH_CHECK();
}

void attn_packed_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* dout, const float* lse, const int* cu,
                     bf16_t* dqkv, int B, int S, int nh, long long T_alloc, float p, uint32_t seed, float* dbias,
                     hipStream_t st) {
  if (B <= 0) return;
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  static bool attr = false;
  if (!attr) {
    DTG_HIP_CHECK(hipFuncSetAttribute((const void*)attn_packed_bwd_kernel<128>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)bwd_lds(128)));
    attr = true;
  }
  if (S == 64) {
    hipLaunchKernelGGL(attn_packed_bwd_kernel<64>, dim3(B * nh), dim3(512), bwd_lds(64), st, qkv, o, dout, lse, cu,
                       dqkv, B, nh, (int)T_alloc, 0.125f, th, ds, seed, dbias); DTG_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(attn_packed_bwd_kernel<128>, dim3(B * nh), dim3(512), bwd_lds(128), st, qkv, o, dout, lse, cu,
                       dqkv, B, nh, (int)T_alloc, 0.125f, th, ds, seed, dbias); DTG_LAUNCH_CHECK();
  }
}

// ---- 128 < S <= 512: the same forward kernel over ceil(S/128) query blocks, the dKV + dQ pair ------------------------
int attn_packed_long_supported(int S, int dh) { return dh == 64 && S % 64 == 0 && S > 128 && S <= 512; }

void attn_packed_long_fwd(const bf16_t* qkv, const int* cu, bf16_t* out, float* lse, int B, int S, int nh,
                          long long T_alloc, float p, uint32_t seed, hipStream_t st) {
  if (B <= 0) return;
  static bool attr = false;
  if (!attr) {  // K and V of a whole record: 144 KB at S = 512
    DTG_HIP_CHECK(hipFuncSetAttribute((const void*)attn_packed_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)fwd_lds(512)));
    attr = true;
  }
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  dim3 grid(B * nh, (S + 16 * kWaves - 1) / (16 * kWaves));
  hipLaunchKernelGGL(attn_packed_fwd_kernel, grid, dim3(64 * kWaves), fwd_lds(S), st, qkv, cu, out, lse, B, S, nh,
                     (int)T_alloc, 0.125f, th, ds, seed); DTG_LAUNCH_CHECK();
}

void attn_packed_long_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* dout, const float* lse, const int* cu,
                          bf16_t* dqkv, int B, int S, int nh, long long T_alloc, float p, uint32_t seed, float* dbias,
                          hipStream_t st) {
  if (B <= 0) return;
  static bool attr = false;
  if (!attr) {
    DTG_HIP_CHECK(hipFuncSetAttribute((const void*)attn_packed_bwd_dkv_kernel,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)dkv_lds(512)));
    DTG_HIP_CHECK(hipFuncSetAttribute((const void*)attn_packed_bwd_dq_kernel,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)dq_lds(512)));
    attr = true;
  }
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const dim3 grid(B * nh, (S + kLongRows - 1) / kLongRows);
  hipLaunchKernelGGL(attn_packed_bwd_dkv_kernel, grid, dim3(512), dkv_lds(S), st, qkv, o, dout, lse, cu, dqkv, B, S, nh,
                     (int)T_alloc, 0.125f, th, ds, seed, dbias); DTG_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_packed_bwd_dq_kernel, grid, dim3(512), dq_lds(S), st, qkv, o, dout, lse, cu, dqkv, B, S, nh,
                     (int)T_alloc, 0.125f, th, ds, seed, dbias); DTG_LAUNCH_CHECK();
}

}  // namespace dtg
