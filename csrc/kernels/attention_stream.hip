// Streaming fused attention for 512 < S <= kStreamMaxS (dtg/kernels.h): head dim 64, bf16, additive key mask,
// pair-hash dropout; attention.hip's operands and results, but no LDS or register array is sized by S.  The kernels of attention.hip
// keep a record's K and V (or Q and dO) resident in LDS, 2 * S * 128 bytes, which ends at S = 512; here the
// streamed operand arrives in 64-row chunks through a 2-slot LDS ring, chunk c + 1's LDS-DMA in flight under
// chunk c's MFMAs, one barrier per chunk.  All 8 waves of a workgroup stage and meet at every barrier, so a wave
// whose 16 rows lie beyond S (the last block of S = 64 * odd) stays in the loop and only skips the arithmetic.
//
// Forward (grid [B*nh, ceil(S/128)], 8 waves, a wave owns 16 queries): attn_fwd_kernel's transposed form
//   (S^T = K Q^T, per-lane online max / sum, O^T += V^T P^T) over ring slots {K as KC tile | V as MC tile}.
// Backward, two launches, no [S, S] tensor in HBM and no atomics on dqkv:
//   dQ  (same grid, a wave owns 16 queries; ring slots {K | V}, both KC): also transposed, so a lane holds one
//       query x 4 consecutive keys: P^T = exp(K Q^T * scale + mask - LSE), dP^T = V dO^T, dS = P (dropout'(dP) - D)
//       -> the wave's [16 q][64 key] KC scratch (8-byte stores) -> dQ += dS K with K read transposed out of its KC
//       image.  D = rowsum(dO * O) of the wave's rows is computed in the prologue and WRITTEN to the workspace.
//   dKV (same grid, a wave owns 16 keys whose K / V fragments stay in registers; ring slots {Q | dO}, both MC, with
//       the chunk's 64 LSE and D values): attn_bwd_dkv_kernel's chunk body; D is read from the workspace, so the
//       launch order is dQ, then dKV.
// The additive mask travels with the chunk (64 floats per slot, dQ and forward) or lives in 4 registers (dKV).
// dbias (optional): per-wave column sums (colsum16), combined over the workgroup in the idle ring, one device
// atomic per column and workgroup.
//
// Dropout.  Element (bh, q, key) has index idx = (bh*S + q)*S + key and is drawn from pair idx >> 1 (keep_attn).
// S is even, so (bh*S + q)*S is even and idx >> 1 == (bh*S + q)*(S/2) + (key >> 1) exactly, as integers.  The
// hash consumes the pair index mod 2^32 (pidx * golden + seed in uint32), and the right-hand side computed in
// wrapping uint32 arithmetic IS that residue, for any size of idx; (uint32)idx >> 1, the form of the kernels in
// attention.hip, equals it only while idx < 2^32 (it drops bit 32 of idx, which is bit 31 of the pair index).
// So the draw equals attention.hip, attn_softmax_fwd and the int64 mirror (attn_dropout_keep) wherever those are
// defined, and stays equal to the mirror beyond 2^32 elements (B*nh*S*S; BERT-base at 32 x 1024 is 4.0e8).
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
}  // namespace

// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * kNW) attn_stream_fwd_kernel(const bf16_t* __restrict__ qkv,
                                                                   const float* __restrict__ mask,
                                                                   bf16_t* __restrict__ out, float* __restrict__ lse,
                                                                   int S, int nh, float scale, uint32_t th,
                                                                   float dscale, uint32_t seed) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bf16_t* Qg = qkv + (long long)b * S * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  lds_char* ring = smem;                                                     // kRing x {K KC | V MC}
  lds_float* Mk = reinterpret_cast<lds_float*>(smem + kRing * kSlot);        // kRing x 64 mask values (stride 128)
  lds_char* scr = smem + kRing * (kSlot + kVec) + wave * kScr;               // per-wave [16][64] bf16
  const int nkc = S / 64;
  const DenseKC<false> ks_{Kg, ld, S, 64};
  const DenseMC<false> vs_{Vg, ld, 64, S};
  const float* mrow = mask ? mask + (long long)b * S : nullptr;
  const int q0 = blockIdx.y * kBlk + wave * 16;
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
  // lane (q = lane & 15, g = lane >> 4): one query against keys j * 16 + 4g + [0, 4) of each 16-key block j
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int qi = lane & 15, g = lane >> 4;
  // pair index of (q, key 0), wrapping (see the head of the file)
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
        const f32x4 madd =
            *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>(Mk + cur * 128 + j * 16 + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[j][r] = fmaf(s[j][r], scale, madd[r]);
          mx = fmaxf(mx, s[j][r]);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // a chunk of masked keys only: mx is about -10000, finite; once a real key arrives alpha = exp(-10000) = 0
      // wipes what the masked chunk left in l and o, and a later masked chunk adds exp(-10000 - m) = 0
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
__global__ void __launch_bounds__(64 * kNW) attn_stream_dq_kernel(const bf16_t* __restrict__ qkv,
                                                                  const bf16_t* __restrict__ o,
                                                                  const bf16_t* __restrict__ dout,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ mask,
                                                                  bf16_t* __restrict__ dqkv, float* __restrict__ dwork,
                                                                  int S, int nh, float scale, uint32_t th,
                                                                  float dscale, uint32_t seed,
                                                                  float* __restrict__ dbias) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bf16_t* Qg = qkv + (long long)b * S * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* Og = o + (long long)b * S * H + h * 64;
  const bf16_t* dOg = dout + (long long)b * S * H + h * 64;
  lds_char* ring = smem;                                                     // kRing x {K KC | V KC}
  lds_float* Mk = reinterpret_cast<lds_float*>(smem + kRing * kSlot);        // kRing x 64 mask values * log2(e)
  lds_char* scr = smem + kRing * (kSlot + kVec) + wave * kScr;               // dS [16 q][64 keys] KC
  const int nkc = S / 64;
  const DenseKC<false> ks_{Kg, ld, S, 64};
  const DenseKC<false> vs_{Vg, ld, S, 64};
  const float* mrow = mask ? mask + (long long)b * S : nullptr;
  const int q0 = blockIdx.y * kBlk + wave * 16;
  const bool active = q0 < S;  // wave-uniform
  const int qi = lane & 15, g = lane >> 4;
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
        const f32x4 madd =
            *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>(Mk + cur * 128 + j * 16 + 4 * g);
        bool kp[4] = {true, true, true, true};
        if (th) keep4_pair(seed, prow + (uint32_t)(key0 >> 1), th, kp);
        float dsv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[j][r], sl2, madd[r] - lq));
          float dpv = dp[j][r];
          if (th) dpv = kp[r] ? dpv * dscale : 0.f;
          dsv[r] = p * (dpv - dd);
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
__global__ void __launch_bounds__(64 * kNW) attn_stream_dkv_kernel(const bf16_t* __restrict__ qkv,
                                                                   const bf16_t* __restrict__ dout,
                                                                   const float* __restrict__ lse,
                                                                   const float* __restrict__ mask,
                                                                   bf16_t* __restrict__ dqkv,
                                                                   const float* __restrict__ dwork, int S, int nh,
                                                                   float scale, uint32_t th, float dscale,
                                                                   uint32_t seed, float* __restrict__ dbias) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_char* smem = (lds_char*)smem_raw;
  const int H = nh * 64;
  const long long ld = 3LL * H;
  const int bh = blockIdx.x, b = bh / nh, h = bh % nh;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bf16_t* Qg = qkv + (long long)b * S * ld + h * 64;
  const bf16_t* Kg = Qg + H;
  const bf16_t* Vg = Qg + 2 * H;
  const bf16_t* dOg = dout + (long long)b * S * H + h * 64;
  lds_char* ring = smem;                                                     // kRing x {Q MC | dO MC}
  lds_float* LD = reinterpret_cast<lds_float*>(smem + kRing * kSlot);        // kRing x {64 LSE * log2(e) | 64 D}
  lds_char* scr = smem + kRing * (kSlot + kVec) + wave * kScr;               // [32 q][16 keys] x {P, dS}
  const int nqc = S / 64;
  const DenseMC<false> qs_{Qg, ld, 64, S};
  const DenseMC<false> ds_{dOg, (long long)H, 64, S};
  // threads 0-63 carry the chunk's LSE, 64-127 its D
  const float* vsrc = (tid < 64 ? lse : dwork) + (long long)bh * S + (tid & 63);
  const float vmul = tid < 64 ? kLog2e : 1.f;
  const int kb = blockIdx.y * kBlk + wave * 16;
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
  stage_mc<64, DenseMC<false>, kNW>(qs_, ring, 0, 0, wave, lane);
  stage_mc<64, DenseMC<false>, kNW>(ds_, ring + kTile, 0, 0, wave, lane);
  if (tid < 128) LD[tid] = vsrc[0] * vmul;
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
      stage_mc<64, DenseMC<false>, kNW>(qs_, ring + nxt * kSlot, 0, (c + 1) * 64, wave, lane);
      stage_mc<64, DenseMC<false>, kNW>(ds_, ring + nxt * kSlot + kTile, 0, (c + 1) * 64, wave, lane);
      if (tid < 128) vnext = vsrc[(c + 1) * 64] * vmul;
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

void attn_stream_fwd(const bf16_t* qkv, const float* mask, bf16_t* out, float* lse, int B, int S, int nh, float p,
                     uint32_t seed, hipStream_t st) {
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  hipLaunchKernelGGL(attn_stream_fwd_kernel, grid, dim3(64 * kNW), kLds, st, qkv, mask, out, lse, S, nh, 0.125f, th,
                     ds, seed); DTG_LAUNCH_CHECK();
}

void attn_stream_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* dout, const float* lse, const float* mask,
                     bf16_t* dqkv, float* dwork, int B, int S, int nh, float p, uint32_t seed, float* dbias,
                     hipStream_t st) {
  const uint32_t th = drop_th(p);
  const float ds = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const dim3 grid(B * nh, (S + kBlk - 1) / kBlk);
  // dQ first: it writes D = rowsum(dO * O) into dwork, which dKV reads
  hipLaunchKernelGGL(attn_stream_dq_kernel, grid, dim3(64 * kNW), kLds, st, qkv, o, dout, lse, mask, dqkv, dwork, S,
                     nh, 0.125f, th, ds, seed, dbias); DTG_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_stream_dkv_kernel, grid, dim3(64 * kNW), kLds, st, qkv, dout, lse, mask, dqkv, dwork, S, nh,
                     0.125f, th, ds, seed, dbias); DTG_LAUNCH_CHECK();
}

}  // namespace dtg
