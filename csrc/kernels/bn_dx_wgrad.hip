// BatchNorm backward dx pass + the weight gradient of the 1x1 conv that produced the BN's input, fused:
//
//   dx  = a * dp + bx * x + c           (per channel; [M, C] bf16, the conv3 output gradient)
//   dx2 = a2 * dp + bx2 * x2 + c2       (projection blocks: the shortcut BN fed by the same dp, optional)
//   dW += dx^T act                      ([C, CI] fp32: conv3's weight gradient, act = its input [M, CI])
//
// ResNet-50's stage-1 conv3 weight gradient read dx (1.64 GB at batch 1024) back from HBM on the side stream
// right after this pass wrote it, and the backward is HBM-bound across both streams: skipping those three
// weight gradients made the step 0.9 ms faster (profiles/r04_dx_wgrad).  Here the dx tile never leaves the
// chip for the weight gradient: each persistent workgroup (4 waves) computes dx for a 32-row block in
// registers, stores it to HBM (for the conv3 dgrad) AND into LDS in the MN-contiguous layout of the wgrad
// operand (the chunk XOR of stage_mc, so frag_mc's transposed reads apply), stages the 32 x CI block of
// `act` by LDS-DMA, and accumulates dW = dx^T act for the whole kernel in registers (wave w: channels
// [64 w, +64) x all CI columns).  The per-workgroup partial is written to a slab and the slabs are summed into
// the fp32 gradient by the split-K reduction (gemm_splitk_reduce, beta = 1).
// A workgroup covers a 256-channel slice of dx (4 waves x 64 channels) and the matching 256 rows of dW: C = 256,
// CI = 64 (ResNet-50 stage 1) or C = 512, CI = 128 (stage 2: two slices per row block, the act block read by
// both from L2 -- the two workgroups of a row block are consecutive on one XCD).
//
// DG (C = 256, CI = 64: stage 1): the conv3 data gradient too.  The only other reader of dx was the dgrad GEMM
// dp2 = mask2 * (dx W3) (gemm_bn mode 3), which read the 1.64 GB straight back to multiply them by a 256 x 64
// weight.  Here the workgroup computes dp2[32, 64] from the dx image while it is in LDS (K-contiguous for this
// product: plain 16-byte reads of the same chunks), with W3 resident on chip (wave w: output columns
// [16 w, +16), 8 k-steps x 4 VGPRs per lane -- in registers, or parked in LDS: WLDS), stages the fp32 tile
// through LDS so that each thread finishes one 8-column group of one row (mode 3's epilogue: packed mask bits,
// sum(dp2) and sum(dp2 * y2) kept per thread over all the workgroup's blocks, one reduction + atomic add per
// workgroup into part[blockIdx % kBnStatSlots]), and dx is not written to HBM at all.
//
// RX (the two 256 x 64 DG forms, on the caller's word that x = bf16(act W3^T), the forward's conv3): x is not read
// either -- each block's x is formed again by MFMA from the act block and W3, both already on chip (see the kernel).
//
// Full-width DG (C = 512, CI = 128: stage 2's identity blocks): the same, in a kernel of its own
// (bn_dx_wgrad_full_kernel below) whose workgroup of 8 waves owns all 512 channels of a row block -- with two
// 256-channel slices per row block the K of dp2 = dx W3 would be split across workgroups.  It replaces the sliced
// 512 x 128 form and the dgrad GEMM behind it where the caller asks for the dgrad; its dual form is not built.
//
// Both kernels are built from one set of pieces (below, before the kernels): dx_chunk and store_mc_chunk (the
// elementwise part and its LDS image), load_w_frag and dgrad_tile (the resident W3 fragments and dp2 = dx W3),
// dgrad_epilogue and dgrad_stats_reduce (mode 3's epilogue and its BN partials), store_slab (the dW partial).  What
// differs stays in the kernels: the pipelines, how act reaches LDS, and where the W3 fragments live.  On the host,
// dx_form alone decides which kernel, grid and slab count a shape gets.
//
// The forward mirror lives here too, because it is built from the same pieces (store_mc_chunk, dgrad_tile, pack8_bf16,
// persistent_grid): bn_apply_gemm_kernel, BN3's forward apply pass that also computes the next block's conv1 from
// the output tile it holds in LDS (see the comment above it).
#include <stdexcept>

#include "dtg/common.h"
#include "dtg/kernels.h"
#include "dtg/mfma_gemm.cuh"
#include "dtg/gemm_epi.cuh"
#include "dtg/bn_apply_expr.cuh"

namespace dtg {

namespace {
using namespace gemm;

constexpr int kDC = 256;   // channels of one workgroup's slice
constexpr int kDR = 32;    // rows per block
constexpr int kDX_LDS = kDR * kDC * 2;   // 16 KB: dx block, [32 m][256 c] MC image
// DG: the staged dp2 tile, [32 m][64] fp32 with column bit 4 XORed by row bit 2 (the two 16-lane groups of a
// half-wave's accumulator write then hit different banks without a padded pitch), and the weight fragments of
// the form that keeps them in LDS (the plain one: 32 KB, which makes its static LDS exactly 64 KB)
constexpr int kDG_LD = 64;
constexpr int kDG_LDS = kDR * kDG_LD * 4;
constexpr int kDGW_LDS = 256 * 64 * 2;

// ---- the pieces both kernels are built from ----
__device__ __forceinline__ u32x4v pack8_bf16(const float (&o)[8]) {
  u32x4v w;
  w.x = pack_bf2(o[0], o[1]);
  w.y = pack_bf2(o[2], o[3]);
  w.z = pack_bf2(o[4], o[5]);
  w.w = pack_bf2(o[6], o[7]);
  return w;
}

// 8 channels of dx = a * dp + bx * x + c from the raw bf16 chunks of dp (g) and x, as bf16
__device__ __forceinline__ u32x4v dx_chunk(const float (&a)[8], const float (&bx)[8], const float (&cc)[8],
                                           const u32x4v& g, const u32x4v& x) {
  float gf[8], xf[8], o[8];
  unpack8_bf16(g, gf);
  unpack8_bf16(x, xf);
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = fmaf(a[k], gf[k], fmaf(bx[k], xf[k], cc[k]));
  return pack8_bf16(o);
}

// [m][CW c] image, 16-B chunk c8 at position c8 ^ mc_swz<CW / 8>(m) (stage_mc's layout, so frag_mc reads it)
template <int CW>
__device__ __forceinline__ void store_mc_chunk(lds_char* img, int m, int c8, const u32x4v& w) {
  *reinterpret_cast<__attribute__((address_space(3))) u32x4v*>(img + m * (CW * 2) +
                                                               ((c8 ^ mc_swz<CW / 8>(m)) << 4)) = w;
}

// one wave's B operand of dp2 = dx W for k-step ks: lane (q = l & 15, g = l >> 4) holds
// W[32 ks + 8 g + j][16 wave + q], j < 8 (2-byte loads, once per workgroup)
__device__ __forceinline__ v8bf load_w_frag(const DxDgrad& dg, int ks, int wave, int lane) {
  const bf16_t* wp = dg.w + (long long)(ks * 32 + 8 * (lane >> 4)) * dg.ldw + wave * 16 + (lane & 15);
  u32x4v t;
  t.x = (uint32_t)wp[0] | ((uint32_t)wp[dg.ldw] << 16);
  t.y = (uint32_t)wp[2 * dg.ldw] | ((uint32_t)wp[3 * dg.ldw] << 16);
  t.z = (uint32_t)wp[4 * dg.ldw] | ((uint32_t)wp[5 * dg.ldw] << 16);
  t.w = (uint32_t)wp[6 * dg.ldw] | ((uint32_t)wp[7 * dg.ldw] << 16);
  return __builtin_bit_cast(v8bf, t);
}

// dp2[16 t + .., 16 wave + ..] = dx[32, CW] W: the image is K-contiguous for this product -- lane (q, g) reads the
// 16-byte chunk 4 ks + g of row 16 t + q (the A operand's 8 k values of k-step ks); fw(ks) is the wave's W fragment
// of k-step ks, from wherever the caller keeps it (the loop is fully unrolled: ks is a constant in fw).
// Then staged [32 m][LD] fp32: lane (q, g) of tile t holds rows 16 t + 4 g + r, column 16 wave + q (column bit 4
// XOR row bit 2 = g & 1).
template <int CW, int LD, class FW>
__device__ __forceinline__ void dgrad_tile(const lds_char* sdx, lds_char* sdg, int wave, int lane, FW fw) {
  const int q = lane & 15, g = lane >> 4;
  f32x4 ad[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int ks = 0; ks < CW / 32; ++ks) {
    const v8bf w = fw(ks);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int m = t * 16 + q, ch = ks * 4 + g;
      const v8bf fd = *reinterpret_cast<const lds_v8bf*>(sdx + m * (CW * 2) + ((ch ^ mc_swz<CW / 8>(m)) << 4));
      ad[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd, w, ad[t], 0, 0, 0);
    }
  }
  lds_float* sg = reinterpret_cast<lds_float*>(sdg);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) sg[(t * 16 + g * 4 + r) * LD + ((wave * 16 + q) ^ ((g & 1) << 4))] = ad[t][r];
}

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2v;

// RX: one wave's W^T operand of x = act W^T, column tile h and k-step ks: lane (q, g) holds W[64 wave + 16 h + q][32 ks + 8 g + j],
// j < 8 -- W is [C, CI], so a fragment is one 16-byte load (as bn_apply_gemm_kernel loads W1)
__device__ __forceinline__ v8bf load_wx_frag(const DxDgrad& dg, int h, int ks, int wave, int lane) {
  return *reinterpret_cast<const v8bf*>(dg.w + (long long)(wave * 64 + h * 16 + (lane & 15)) * dg.ldw + ks * 32 +
                                        8 * (lane >> 4));
}

// RX: x[32, 256] = bf16(act[32, CI] W^T) into the dx image's chunk positions, from the act block in LDS (K-contiguous
// for this product: lane (q, g) reads the 16-byte chunk 4 ks + g of row 16 t + q, as dgrad_tile reads the dx image).
// Wave w forms channels [64 w, +64), transposed (W is the MFMA's row operand, act its column operand), so that lane
// (q, g) of tile (h, t) holds channels 64 w + 16 h + 4 g + r, r < 4, of row 16 t + q: one 8-byte store per tile, and the
// elementwise thread then finds its 8-channel chunks where store_mc_chunk will put their dx.
template <int CI>
__device__ __forceinline__ void recompute_x_tile(const lds_char* sact, lds_char* sdx, int wave, int lane,
                                                 const v8bf (&wx)[4][CI / 32]) {
  const int q = lane & 15, g = lane >> 4;
  v8bf fb[2][CI / 32];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < CI / 32; ++ks) {
      const int m = t * 16 + q, ch = ks * 4 + g;
      fb[t][ks] = *reinterpret_cast<const lds_v8bf*>(sact + m * (CI * 2) + ((ch ^ mc_swz<CI / 8>(m)) << 4));
    }
#pragma unroll
  for (int h = 0; h < 4; ++h)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 y = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < CI / 32; ++ks) y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wx[h][ks], fb[t][ks], y, 0, 0, 0);
      const int m = t * 16 + q, ch = wave * 8 + h * 2 + (g >> 1);
      u32x2v w;
      w.x = pack_bf2(y[0], y[1]);
      w.y = pack_bf2(y[2], y[3]);
      *reinterpret_cast<__attribute__((address_space(3))) u32x2v*>(sdx + m * (kDC * 2) +
                                                                   ((ch ^ mc_swz<kDC / 8>(m)) << 4) + (g & 1) * 8) = w;
    }
}

// mode 3's epilogue (bn_epi.cuh) for row er, columns [8 cg, +8) of the staged tile: d = bit ? v : 0 stored as bf16
// (dst), the statistics sum(d) / sum(d * y) in fp32 on the unrounded d, kept per thread in ds / dq
template <int CI>
__device__ __forceinline__ void dgrad_epilogue(const lds_char* sdg, int er, int cg, const u32x4v& yv, uint32_t mb,
                                               float (&ds)[8], float (&dq)[8], bf16_t* dst) {
  const lds_float* sp = reinterpret_cast<const lds_float*>(sdg) + er * CI + ((cg * 8) ^ (((er >> 2) & 1) << 4));
  float v[8], yf[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = sp[k];
  unpack8_bf16(yv, yf);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float d = ((mb >> k) & 1u) ? v[k] : 0.f;
    v[k] = d;
    ds[k] += d;
    dq[k] += d * yf[k];
  }
  *reinterpret_cast<u32x4v*>(dst) = pack8_bf16(v);
}

// once per workgroup: reduce the statistics over the 32 threads of a column group through red ([2][32 er][CI] fp32:
// 16 KB at CI = 64, 32 KB at 128), raw moment -> centred, one atomic add per column into this workgroup's partial slot
template <int CI>
__device__ __forceinline__ void dgrad_stats_reduce(lds_float* red, int tid, int er, int cg, const float (&ds)[8],
                                                   const float (&dq)[8], const DxDgrad& dg) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    red[er * CI + cg * 8 + k] = ds[k];
    red[(kDR + er) * CI + cg * 8 + k] = dq[k];
  }
  __syncthreads();
  if (tid < CI) {
    float ts = 0.f, tq = 0.f;
#pragma unroll 8
    for (int j = 0; j < kDR; ++j) {
      ts += red[j * CI + tid];
      tq += red[(kDR + j) * CI + tid];
    }
    tq = dg.invstd[tid] * (tq - dg.mean[tid] * ts);
    float* part = dg.part + (long long)(blockIdx.x % kBnStatSlots) * 2 * CI;
    atomicAdd(part + tid, ts);
    atomicAdd(part + CI + tid, tq);
  }
}

// a wave's 64 x CI block of the dW partial ([.][CI] fp32, its workgroup's rows): lane (q = l & 15, g = l >> 4) of tile
// (i, j) holds rows 64 w + 16 i + 4 g + r, column 16 j + q
template <int NJ>
__device__ __forceinline__ void store_slab(float* slab, int CI, int wave, int lane, const f32x4 (&acc)[4][NJ]) {
  const int q = lane & 15, gq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) slab[(wave * 64 + i * 16 + gq * 4 + r) * CI + j * 16 + q] = acc[i][j][r];
}

// W2 (with DUAL): also dW2 += dx2^T act2 -- the stride-1 projection shortcut's weight gradient (stage 1)
// DG: also dp2 = bits * (dx W) with its BN's backward partials, and dx itself is not stored (see above)
// RX (with DG): x is not read.  The caller vouches that it is bf16(act W^T) -- the forward's conv3 output, K = 64 --
// and the pass holds both operands: the act block in LDS for the weight gradient, W for the data gradient.  So each
// block's x is formed again by MFMA (recompute_x_tile: 16 per wave) into the dx image, where every elementwise thread
// reads its own four chunks back and overwrites them with dx: no LDS beyond the image, and x's 1.64 GB at batch 1024
// (36 % of the pass's bytes) stay in HBM.  The W^T fragments (32 registers per lane) are resident in the dual form (1
// workgroup per CU); the plain form, whose register file is full, prefetches them from L2 with each block's loads (x's
// four prefetch registers per row are free).  With fewer bytes per block in flight the pass no longer hides the
// vmcnt(0) that the compiler puts behind an LDS-DMA (first build: 3.98 TB/s, profiles/r12_dx_recompute), so this form
// takes the act block through registers too, as bn_dx_wgrad_full_kernel does: four barriers per block (act image,
// x image, dx image, dp2 tile), no hand-counted wait, and the next block's loads in flight under all of them.
template <int CI, bool DUAL, bool W2 = false, bool DG = false, bool RX = false>
__global__ void __launch_bounds__(256, (CI == 64 && !W2) ? 2 : 1) bn_dx_wgrad_kernel(const bf16_t* __restrict__ dp, const bf16_t* __restrict__ x,
                                                          const float* __restrict__ coef,
                                                          const bf16_t* __restrict__ x2,
                                                          const float* __restrict__ coef2, bf16_t* __restrict__ dx,
                                                          bf16_t* __restrict__ dx2, const bf16_t* __restrict__ act,
                                                          long long ldact, float* __restrict__ slabs, int nblk,
                                                          int C, const bf16_t* __restrict__ act2, long long ldact2,
                                                          float* __restrict__ slabs2, DxDgrad dg) {
  static_assert(!W2 || (DUAL && CI == 64), "the second weight gradient is the dual form's, at 256 x 64");
  static_assert(!DG || (CI == 64 && DUAL == W2), "the fused dgrad is 256 x 64: the plain form or the two-weight dual");
  static_assert(!RX || DG, "x is recomputed from the fused dgrad's weight");
  constexpr int kACT_LDS = kDR * CI * 2;  // act block, [32 m][CI] MC image (two slots)
  constexpr int NJ = CI / 16;             // dW column tiles per wave
  constexpr int NX = W2 ? 2 : 1;  // dx images / act slot pairs
  // DG: where the weight fragments live.  The plain form at 2 workgroups per CU has 256 registers per lane and
  // spills with 32 more of them held (255 VGPRs + 32 B of scratch), so it parks them in LDS; the dual form runs 1
  // workgroup per CU (512 registers) and keeps them in registers -- its LDS would not hold them (56.5 + 32 KB).
  constexpr bool WLDS = DG && !W2;
  __shared__ __attribute__((aligned(16))) char smem_raw[NX * (kDX_LDS + 2 * kACT_LDS) + (DG ? kDG_LDS : 0) +
                                                        (WLDS ? kDGW_LDS : 0)];
  lds_char* sdx = (lds_char*)smem_raw;
  lds_char* sact = sdx + kDX_LDS;
  lds_char* sdx2 = sact + 2 * kACT_LDS;  // W2 only
  lds_char* sact2 = sdx2 + kDX_LDS;
  lds_char* sdg = (lds_char*)smem_raw + NX * (kDX_LDS + 2 * kACT_LDS);  // DG only: dp2 tile, [32 m][kDG_LD] fp32
  // WLDS: fragment ks of this lane at swf[ks * 64] -- written and read by the same lane only, lane-linear
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = gridDim.x;  // a multiple of 8 and of the slice count (host)
  const int ns = C / kDC, gid = xcd_remap(blockIdx.x, G);
  const int sl = gid % ns;  // this workgroup's channel slice (fixed: G % ns == 0)
  // elementwise part: thread = (8-channel chunk c8, row slot rs); rows rs + 8 u, u < 4
  const int c8 = tid & 31, rs = tid >> 5, c0 = sl * kDC + c8 * 8;
  float a[8], bx[8], cc[8], a2[8], bx2[8], cc2[8];
  load8_f32(coef + c0, a);
  load8_f32(coef + C + c0, bx);
  load8_f32(coef + 2 * C + c0, cc);
  if constexpr (DUAL) {
    load8_f32(coef2 + c0, a2);
    load8_f32(coef2 + C + c0, bx2);
    load8_f32(coef2 + 2 * C + c0, cc2);
  }
  DenseMC<false> sa{act, ldact, CI, 0};
  DenseMC<false> sa2{act2, ldact2, CI, 0};
  f32x4 acc[4][NJ], acc2[W2 ? 4 : 1][W2 ? NJ : 1];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (W2) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // DG: this wave's B operand of dp2 = dx W, resident for the whole kernel: lane (q = l & 15, g = l >> 4) holds
  // W[32 ks + 8 g + j][16 wave + q], j < 8, of k-step ks (2-byte loads of a 32 KB matrix, once per workgroup);
  // the epilogue thread = (row er, 8-column group cg) keeps sum(dp2) / sum(dp2 * y) of its columns in ds / dq
  v8bf wf[(DG && !WLDS) ? 8 : 1];
  lds_v8bf* swf = reinterpret_cast<lds_v8bf*>(sdg + kDG_LDS) + wave * 8 * 64 + lane;
  float ds[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int er = tid >> 3, cg = tid & 7;
  if constexpr (DG) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const v8bf t = load_w_frag(dg, ks, wave, lane);
      if constexpr (WLDS) swf[ks * 64] = t;
      else wf[ks] = t;
    }
  }

  // Software-pipelined over this workgroup's blocks: block b+1's act DMA and dp / x loads are issued right after
  // block b's dx is stored, so they are in flight under block b's MFMAs and barriers.
  u32x4v g[4], xv[4], x2v[4];  // raw bf16 until used: 12 registers per row instead of 24
  u32x4v yv, yvn;     // DG: the epilogue thread's 8 y values of the current / the prefetched block
  uint32_t mb, mbn;   // ... and its byte of mask bits
  // RX: this wave's W^T fragments of x = act W^T (load_wx_frag); resident where the register file holds them (WXRES)
  constexpr bool WXRES = RX && W2;
  v8bf wx[RX ? 4 : 1][RX ? CI / 32 : 1];
  auto load_wx = [&]() {
#pragma unroll
    for (int h = 0; h < (RX ? 4 : 0); ++h)
#pragma unroll
      for (int ks = 0; ks < CI / 32; ++ks) wx[h][ks] = load_wx_frag(dg, h, ks, wave, lane);
  };
  if constexpr (WXRES) load_wx();
  // RX: the act block goes through registers (one 16-byte chunk per thread: row er, chunk cg; stored in stage_mc's
  // layout at the top of its block), as in bn_dx_wgrad_full_kernel: behind an LDS-DMA the compiler puts a vmcnt(0) in
  // front of the first LDS read after the barrier, and the next block's loads would not stay in flight under the MFMAs
  u32x4v av, av2;
  auto issue = [&](int b, int slot) {
    const long long m0 = (long long)b * kDR;
    if constexpr (RX && !WXRES) load_wx();  // from L2, for block b
    if constexpr (DG && !RX) {  // first: they are back before the dp / x loads the next iteration waits for anyway
      yvn = *reinterpret_cast<const u32x4v*>(dg.y + (m0 + er) * CI + cg * 8);
      mbn = dg.bits[(m0 + er) * (CI / 8) + cg];
    }
    if constexpr (RX) {
      av = *reinterpret_cast<const u32x4v*>(act + (m0 + er) * ldact + cg * 8);
      if constexpr (W2) av2 = *reinterpret_cast<const u32x4v*>(act2 + (m0 + er) * ldact2 + cg * 8);
    } else {
      stage_mc<CI, DenseMC<false>, 4, kDR>(sa, sact + slot * kACT_LDS, 0, (int)m0, wave, lane);
      if constexpr (W2) stage_mc<CI, DenseMC<false>, 4, kDR>(sa2, sact2 + slot * kACT_LDS, 0, (int)m0, wave, lane);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long off = (m0 + rs + 8 * u) * C + c0;
      g[u] = *reinterpret_cast<const u32x4v*>(dp + off);
      if constexpr (!RX) xv[u] = *reinterpret_cast<const u32x4v*>(x + off);
      if constexpr (DUAL) x2v[u] = *reinterpret_cast<const u32x4v*>(x2 + off);
    }
  };
  // tiles t = gid + it G: row block t / ns, slice t % ns = sl
  const int b0 = gid / ns, gb = G / ns;
  if (b0 < nblk) issue(b0, 0);
  int slot = 0;
  for (int b = b0; b < nblk; b += gb, slot ^= RX ? 0 : 1) {  // RX: one act slot, written at the top of the block
    const long long m0 = (long long)b * kDR;
    if constexpr (DG && !RX) {
      yv = yvn;
      mb = mbn;
    }
    if constexpr (RX) {  // this block's epilogue operands: used after the MFMAs, and older than the next block's loads
      yv = *reinterpret_cast<const u32x4v*>(dg.y + (m0 + er) * CI + cg * 8);
      mb = dg.bits[(m0 + er) * (CI / 8) + cg];
      store_mc_chunk<CI>(sact, er, cg, av);  // every wait on a load in this form is the compiler's own
      if constexpr (W2) store_mc_chunk<CI>(sact2, er, cg, av2);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // x into the (free) dx image; then each thread takes the chunks it is about to overwrite
      recompute_x_tile<CI>(sact, sdx, wave, lane, wx);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int m = rs + 8 * u;
        xv[u] = *reinterpret_cast<const __attribute__((address_space(3))) u32x4v*>(
            sdx + m * (kDC * 2) + ((c8 ^ mc_swz<kDC / 8>(m)) << 4));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = rs + 8 * u;
      const long long off = (m0 + m) * C + c0;
      const u32x4v w = dx_chunk(a, bx, cc, g[u], xv[u]);
      if constexpr (!DG) *reinterpret_cast<u32x4v*>(dx + off) = w;
      store_mc_chunk<kDC>(sdx, m, c8, w);
      if constexpr (DUAL) {
        const u32x4v w2 = dx_chunk(a2, bx2, cc2, g[u], x2v[u]);
        *reinterpret_cast<u32x4v*>(dx2 + off) = w2;
        if constexpr (W2) store_mc_chunk<kDC>(sdx2, m, c8, w2);
      }
    }
    const bool more = b + gb < nblk;
    // RX: without a branch (the last block is loaded once more for nothing), so that the waits stay counted ones
    if constexpr (RX) issue(more ? b + gb : b, 0);
    else if (more) issue(b + gb, slot ^ 1);
    // act(b) landed: younger are this block's dx stores (4, DUAL 8; DG stores no dx: 0, DUAL 4) and, when issued,
    // block b+1's DMA (CI / 64 pieces) and loads (8, DUAL 12; DG 2 more: y and the mask byte); the dx image is
    // written; then both are visible to every wave.  (DG: block b-1's dp2 store, issued after the previous
    // iteration's last barrier, is older than all of these, so the counts need not include it.)
    constexpr int PIECES = (CI / 64) * (W2 ? 2 : 1);
    constexpr int NST = (DG ? 0 : 4) + (DUAL ? 4 : 0), NLD = (DUAL ? 12 : 8) + (DG ? 2 : 0);
    // RX: no load is waited for here: only the dx image
    if constexpr (RX) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else if (more) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NST + PIECES + NLD) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NST) : "memory");
    __builtin_amdgcn_s_barrier();
    // dW[64 wave + 16 i + .., 16 j + ..] += dx^T act over the block's 32 rows (one 32-deep k-step)
    v8bf fa[4], fb[NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = frag_mc<kDC>(sdx, wave * 64 + i * 16, 0, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) fb[j] = frag_mc<CI>(sact + slot * kACT_LDS, j * 16, 0, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    if constexpr (W2) {
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = frag_mc<kDC>(sdx2, wave * 64 + i * 16, 0, lane);
#pragma unroll
      for (int j = 0; j < NJ; ++j) fb[j] = frag_mc<CI>(sact2 + slot * kACT_LDS, j * 16, 0, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc2[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc2[i][j], 0, 0, 0);
    }
    if constexpr (DG)  // the previous block's tile was last read before this iteration's first barrier
      dgrad_tile<kDC, CI>(sdx, sdg, wave, lane, [&](int ks) -> v8bf {
        if constexpr (WLDS) return swf[ks * 64];
        else return wf[ks];
      });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the dx image is free for the next block (DG: and the dp2 tile is staged)
    if constexpr (DG) dgrad_epilogue<CI>(sdg, er, cg, yv, mb, ds, dq, dg.dp + (m0 + er) * CI + cg * 8);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (DG) {  // through the (free) dx image; a workgroup without a block adds nothing
    if (b0 < nblk) dgrad_stats_reduce<CI>(reinterpret_cast<lds_float*>(sdx), tid, er, cg, ds, dq, dg);
  }
  // this workgroup's partial: rows [256 sl, +256) of slab gid / ns ([C][CI])
  store_slab<NJ>(slabs + ((long long)(gid / ns) * C + sl * kDC) * CI, CI, wave, lane, acc);
  if constexpr (W2) store_slab<NJ>(slabs2 + ((long long)(gid / ns) * C + sl * kDC) * CI, CI, wave, lane, acc2);
}

// The full-width DG form (C = 512, CI = 128: stage 2).  One workgroup of 8 waves owns all 512 channels of a
// 32-row block, so the whole K of dp2 = dx W3 is on chip: the dx image is [32 m][512 c] (32 KB), wave w accumulates
// dW rows [64 w, +64) x all 128 columns (128 registers per lane) and the dp2 columns [16 w, +16) over K = 512
// (16 k-steps).  W3 is 128 KB: each lane keeps its fragments of the first kFW_REG k-steps in registers and parks
// the rest in LDS (lane-linear, written and read by that lane only).  One workgroup per CU (2 waves per SIMD, 256
// registers per lane), so what is not needed across a block is not kept in registers: the dx coefficients live in
// LDS, and the epilogue's y / mask bytes are loaded at the top of the block they belong to.
// The act block goes through registers too (one 16-byte chunk per thread, prefetched with the next block's dp / x and
// written to LDS in stage_mc's layout next to the dx image) instead of LDS-DMA.  Every wait on a load is then the
// compiler's own, on the registers it needs: behind an LDS-DMA it puts a full vmcnt(0) in front of the first LDS read
// after the barrier, which here, with one workgroup per CU, would leave nothing in flight under the MFMAs.
constexpr int kFC = 512, kFCI = 128;
constexpr int kFW_REG = 5;                                   // k-steps of W3 in registers (4 VGPRs each)
constexpr int kFDX_LDS = kDR * kFC * 2;                      // 32 KB: dx block, [32 m][512 c] MC image
constexpr int kFACT_LDS = kDR * kFCI * 2;                    // 8 KB: act block, [32 m][128] MC image
constexpr int kFDG_LDS = kDR * kFCI * 4;                     // 16 KB: the staged dp2 tile, [32 m][128] fp32
constexpr int kFCOEF_LDS = 3 * kFC * 4;                      // 6 KB: [a | bx | c]
constexpr int kFW_LDS = (16 - kFW_REG) * 32 * kFCI * 2;      // 8 KB per parked k-step
constexpr int kF_LDS = kFDX_LDS + kFACT_LDS + kFDG_LDS + kFCOEF_LDS + kFW_LDS;  // 150 KB: dynamic
// (The dual form -- the projection block: dx2 for the shortcut BN from the same dp -- is not built: with 16 more
// registers of prefetched x2 it spilled 196 B per lane at this split and 180 B at kFW_REG = 4, and its second
// coefficient set leaves no LDS for a smaller share; profiles/r09_dx_dgrad_s2.)

__global__ void __launch_bounds__(512, 1) bn_dx_wgrad_full_kernel(const bf16_t* __restrict__ dp, const bf16_t* __restrict__ x,
                                                                  const float* __restrict__ coef,
                                                                  const bf16_t* __restrict__ act, long long ldact,
                                                                  float* __restrict__ slabs, int nblk, DxDgrad dg) {
  constexpr int C = kFC, CI = kFCI, NJ = CI / 16, KS = C / 32;
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
  lds_char* sdx = (lds_char*)smem_dyn;
  lds_char* sact = sdx + kFDX_LDS;
  lds_char* sdg = sact + kFACT_LDS;
  lds_float* scoef = reinterpret_cast<lds_float*>(sdg + kFDG_LDS);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = gridDim.x, gid = xcd_remap(blockIdx.x, G);
  // elementwise part: thread = (8-channel chunk c8 = tid & 63, row slot rs = tid >> 6); rows rs + 8 u, u < 4;
  // act: thread = (row tid >> 4, 16-byte chunk tid & 15)
  f32x4 acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // this wave's B operand of dp2 = dx W: lane (q = l & 15, g = l >> 4) holds W[32 ks + 8 g + j][16 wave + q], j < 8,
  // of k-step ks; the epilogue thread = (row er, 8-column group cg) keeps sum(dp2) / sum(dp2 * y) in ds / dq
  v8bf wf[kFW_REG];
  lds_v8bf* swf = reinterpret_cast<lds_v8bf*>(scoef + 3 * C) + wave * (KS - kFW_REG) * 64 + lane;
  float ds[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dq[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // (er = tid >> 4, cg = tid & 15)
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const v8bf t = load_w_frag(dg, ks, wave, lane);
    if (ks < kFW_REG) wf[ks < kFW_REG ? ks : 0] = t;
    else swf[(ks - kFW_REG) * 64] = t;
  }
  for (int i = tid; i < 3 * C; i += 512) scoef[i] = coef[i];
  __syncthreads();

  auto load8_lds = [](const lds_float* p, float (&o)[8]) {
    const f32x4 lo = *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>(p);
    const f32x4 hi = *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>(p + 4);
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3]; o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = hi[3];
  };
  u32x4v g[4], xv[4], av;
  auto issue = [&](int b, int t) {
    const long long m0 = (long long)b * kDR;
    av = *reinterpret_cast<const u32x4v*>(act + (m0 + (t >> 4)) * ldact + (t & 15) * 8);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long off = (m0 + (t >> 6) + 8 * u) * C + (t & 63) * 8;
      g[u] = *reinterpret_cast<const u32x4v*>(dp + off);
      xv[u] = *reinterpret_cast<const u32x4v*>(x + off);
    }
  };
  if (gid < nblk) issue(gid, tid);
  for (int b = gid; b < nblk; b += G) {
    const long long m0 = (long long)b * kDR;
    // This thread's offsets and LDS addresses are the same in every block; hoisted out of the loop they would cost
    // ~70 registers that the resident state does not leave, so they are recomputed per block from opaque copies
    int tl = tid;
    asm volatile("" : "+v"(tl));
    const int c8 = tl & 63, rs = tl >> 6, c0 = c8 * 8, er = tl >> 4, cg = tl & 15;
    // this block's epilogue operands: used after the MFMAs, and older than the next block's loads
    const u32x4v yv = *reinterpret_cast<const u32x4v*>(dg.y + (m0 + er) * CI + cg * 8);
    const uint32_t mb = dg.bits[(m0 + er) * (CI / 8) + cg];
    {
      float a[8], bx[8], cc[8];
      load8_lds(scoef + c0, a);
      load8_lds(scoef + C + c0, bx);
      load8_lds(scoef + 2 * C + c0, cc);
      // the act chunk: row er', chunk position ac ^ mc_swz<16>(er') of the [32 m][128] image
      store_mc_chunk<CI>(sact, er, cg, av);
#pragma unroll
      for (int u = 0; u < 4; ++u)  // the [m][512 c] image; dx goes nowhere else
        store_mc_chunk<C>(sdx, rs + 8 * u, c8, dx_chunk(a, bx, cc, g[u], xv[u]));
    }
    // the next block's loads, without a branch (the last block is loaded once more for nothing): where the two paths
    // met, the wait for this block's y / mask loads became a vmcnt(0) that took the next block's loads with it
    issue(b + G < nblk ? b + G : b, tl);
    // the dx image and the act block are written (no load is waited for here: the next block's stay in flight under
    // the MFMAs and the epilogue); then both are visible to every wave
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const int ln = tl & 63;
    // dW[64 wave + 16 i + .., 16 j + ..] += dx^T act over the block's 32 rows (one 32-deep k-step)
    {
      v8bf fa[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = frag_mc<C>(sdx, wave * 64 + i * 16, 0, ln);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const v8bf fb = frag_mc<CI>(sact, j * 16, 0, ln);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb, acc[i][j], 0, 0, 0);
      }
    }
    // the previous block's tile was last read before this iteration's first barrier
    dgrad_tile<C, CI>(sdx, sdg, wave, ln, [&](int ks) -> v8bf {
      if (ks < kFW_REG) return wf[ks < kFW_REG ? ks : 0];
      return swf[(ks - kFW_REG) * 64];
    });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the dx image and the act block are free for the next block, the dp2 tile is staged
    dgrad_epilogue<CI>(sdg, er, cg, yv, mb, ds, dq, dg.dp + (m0 + er) * CI + cg * 8);
  }
  // through the (free) dx image; a workgroup without a block adds nothing
  if (gid < nblk) dgrad_stats_reduce<CI>(reinterpret_cast<lds_float*>(sdx), tid, tid >> 4, tid & 15, ds, dq, dg);
  store_slab<NJ>(slabs + (long long)gid * C * CI, CI, wave, lane, acc);  // this workgroup's partial: slab gid
}

// ---- forward: BN3's apply pass + the next block's conv1 (C x N = 256 x 64 or 256 x 128: stage 1; 512 x 128: stage 2) ----
// The forward mirror of DG.  out = relu(bn3(y3) + identity) (TWO: relu(bn3(y3) + bn_d(yd)), the projection block) is
// the block output; the only other forward reader of its 1.64 GB was the next block's conv1, y1n = out W1^T
// (gemm_bn mode 1), which read them straight back.  Here a workgroup (C / 64 waves) computes out for a 32-row block with
// bn_apply8 / bn_apply2_8 (the unfused pass's own expressions), stores it and its packed mask bits to HBM -- out is
// still the residual and conv1's wgrad operand -- and into LDS (store_mc_chunk: K-contiguous for this product), then
// runs dgrad_tile against W1 fragments resident in registers (wave w: output columns [16 NT w, +16 NT), NT column
// tiles x C / 32 k-steps x 4 VGPRs per lane: 32 at 256 x 64, 64 at the other two; W1 is [N, C], so a lane's fragment is one 16-byte load), stages the
// fp32 tile through LDS and finishes 8-column groups of a row per thread: y1n as bf16 and, as bn_epi.cuh's mode 1,
// sum(r) / sum(r * r) of the rounded values, kept per thread over all the workgroup's blocks, one LDS reduction and one
// atomic add per column into part[gid % kBnStatSlots] (the remapped id).  The next block's y3 / identity tiles are prefetched
// through registers under the MFMAs and the epilogue; every wait on a load is the compiler's own.
template <int C, int N, bool TWO>
__global__ void __launch_bounds__(C, C == 256 ? 2 : 1) bn_apply_gemm_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ r,
                                                               const float* __restrict__ coef,
                                                               const float* __restrict__ coef2,
                                                               bf16_t* __restrict__ out, uint8_t* __restrict__ bits,
                                                               const bf16_t* __restrict__ w1, long long ldw,
                                                               bf16_t* __restrict__ y1n, float* __restrict__ part,
                                                               int nblk) {
  static_assert((C == 256 && (N == 64 || N == 128)) || (C == 512 && N == 128),
                "conv1 of stage 1 (64), of stage 2's first block (128), or of stage 2 (512 x 128)");
  // one thread per 8-channel chunk of 4 rows: C threads (4 or 8 waves), each wave NT 16-column tiles of y1n over KS k-steps
  constexpr int NTH = C, NT = N / 16 / (NTH / 64), KS = C / 32;
  constexpr int CG = N / 8, NR = NTH / CG, NP = kDR / NR;  // epilogue: thread = (row er0 + NR p, 8-column group cg)
  constexpr int kIMG_LDS = kDR * C * 2;                    // out block, [32 m][C c] MC image
  constexpr int kTILE_LDS = kDR * N * 4;                   // the staged y1n tile, [32 m][N] fp32 (dgrad_tile's layout)
  static_assert(2 * NR * N * 4 <= kIMG_LDS, "the statistics reduction goes through the out image");
  __shared__ __attribute__((aligned(16))) char smem_raw[kIMG_LDS + kTILE_LDS];
  lds_char* simg = (lds_char*)smem_raw;
  lds_char* stile = simg + kIMG_LDS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = gridDim.x, gid = xcd_remap(blockIdx.x, G);
  // elementwise part: thread = (8-channel chunk c8, row slot rs); rows rs + 8 u, u < 4
  const int c8 = tid % (C / 8), rs = tid / (C / 8), c0 = c8 * 8;
  float sc[8], sf[8], sc2[8];
  load8_f32(coef + c0, sc);
  load8_f32(coef + C + c0, sf);
  if constexpr (TWO) {
    float sf2[8];
    load8_f32(coef2 + c0, sc2);
    load8_f32(coef2 + C + c0, sf2);
#pragma unroll
    for (int k = 0; k < 8; ++k) sf[k] += sf2[k];
  }
  // this wave's B operand of y1n = out W1^T: lane (q = l & 15, g = l >> 4) holds W1[16 (NT wave + h) + q][32 ks + 8 g + j],
  // j < 8, of column tile h and k-step ks
  v8bf wf[NT][KS];
#pragma unroll
  for (int h = 0; h < NT; ++h)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      wf[h][ks] = *reinterpret_cast<const v8bf*>(w1 + (long long)((wave * NT + h) * 16 + (lane & 15)) * ldw + ks * 32 +
                                                 8 * (lane >> 4));
  float ss[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int er0 = tid / CG, cg = tid % CG;

  u32x4v xv[4], rv[4];  // raw bf16 until used
  auto issue = [&](int b) {
    const long long m0 = (long long)b * kDR;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long off = (m0 + rs + 8 * u) * C + c0;
      xv[u] = *reinterpret_cast<const u32x4v*>(x + off);
      rv[u] = *reinterpret_cast<const u32x4v*>(r + off);
    }
  };
  if (gid < nblk) issue(gid);
  for (int b = gid; b < nblk; b += G) {
    const long long m0 = (long long)b * kDR;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = rs + 8 * u;
      const long long off = (m0 + m) * C + c0;
      float a[8], rf[8];
      unpack8_bf16(xv[u], a);
      unpack8_bf16(rv[u], rf);
      if constexpr (TWO) bn_apply2_8(a, rf, sc, sc2, sf);
      else bn_apply8<true, true>(a, rf, sc, sf);
      const u32x4v w = pack8_bf16(a);
      *reinterpret_cast<u32x4v*>(out + off) = w;
      if (bits) store_bits(bits, off, a, c8, C);
      store_mc_chunk<C>(simg, m, c8, w);
    }
    // the next block's loads, without a branch (the last block is loaded once more for nothing), in flight under the
    // MFMAs and the epilogue
    issue(b + G < nblk ? b + G : b);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the out image is visible to every wave; the previous tile has been read
#pragma unroll
    for (int h = 0; h < NT; ++h)
      dgrad_tile<C, N>(simg, stile, wave * NT + h, lane, [&](int ks) -> v8bf { return wf[h][ks]; });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the out image is free for the next block, the y1n tile is staged
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int er = er0 + p * NR;
      const lds_float* sp = reinterpret_cast<const lds_float*>(stile) + er * N + ((cg * 8) ^ (((er >> 2) & 1) << 4));
      float v[8], rd[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = sp[k];
      const u32x4v w = pack8_bf16(v);
      unpack8_bf16(w, rd);  // statistics of what the next block's apply pass will read
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        ss[k] += rd[k];
        sq[k] += rd[k] * rd[k];
      }
      *reinterpret_cast<u32x4v*>(y1n + (m0 + er) * N + cg * 8) = w;
    }
  }
  if (gid < nblk) {  // through the (free) out image; a workgroup without a block adds nothing
    lds_float* red = reinterpret_cast<lds_float*>(simg);  // [2][NR][N]
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      red[er0 * N + cg * 8 + k] = ss[k];
      red[(NR + er0) * N + cg * 8 + k] = sq[k];
    }
    __syncthreads();
    if (tid < N) {
      float ts = 0.f, tq = 0.f;
#pragma unroll 8
      for (int j = 0; j < NR; ++j) {
        ts += red[j * N + tid];
        tq += red[(NR + j) * N + tid];
      }
      // by the remapped id: with few row blocks (gid < nblk) the workgroups that have one then spread over all the
      // slots -- at 64 blocks two adds per slot, whose order cannot change the sum -- instead of sharing the four
      // slots their blockIdx (multiples of 8: one XCD) would give them
      float* slot = part + (long long)(gid % kBnStatSlots) * 2 * N;
      atomicAdd(slot + tid, ts);
      atomicAdd(slot + N + tid, tq);
    }
  }
}

// ---- host: which form a shape gets ----
// One form of the pass: its kernel (behind a typed launcher), workgroup size and dynamic LDS, the persistent grid its
// row blocks are dealt over, and the fp32 dW slabs that grid writes (one per workgroup of a channel slice).
struct DxForm {
  void (*launch)(const DxForm& f, hipStream_t st, const bf16_t* dp, const DxSide& a, const DxSide& b, int nblk, int C,
                 const DxDgrad& d);
  int block, lds, grid, slabs;
};

// as many workgroups as the device holds at once, at most `cap` per CU: a multiple of 8 (the XCD count) and so of the
// slice count (<= 2) on any CU count
int persistent_grid(const void* kern, int block, int lds, int cap) {
  int dev = 0, cus = 0, per_cu = 0;
  DTG_HIP_CHECK(hipGetDevice(&dev));
  DTG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  if (lds) DTG_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  DTG_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, block, lds));
  if (lds && per_cu < 1) throw std::runtime_error("bn_dx_wgrad: the full-width form does not fit a CU");
  int G = cus * (per_cu < 1 ? 1 : (per_cu > cap ? cap : per_cu));
  G -= G % 8;
  return G < 8 ? 8 : G;
}

template <int CI, bool DUAL, bool W2 = false, bool DG = false, bool RX = false>
DxForm sliced_form(int C) {
  // sized by the dual kernel of the width: the slab count is asked for before dx2 is (the fused-dgrad forms are sized
  // by their own kernels: the plain one and the two-weight dual; their RX forms by the same, so that the slab count
  // does not depend on the choice -- they have the same LDS and workgroups per CU)
  static const int G = persistent_grid((const void*)bn_dx_wgrad_kernel<CI, DG ? W2 : true, W2, DG>, 256, 0, 2);
  return {[](const DxForm& f, hipStream_t st, const bf16_t* dp, const DxSide& a, const DxSide& b, int nblk, int C,
             const DxDgrad& d) {
            hipLaunchKernelGGL((bn_dx_wgrad_kernel<CI, DUAL, W2, DG, RX>), dim3(f.grid), dim3(f.block), f.lds, st, dp, a.x,
                               a.coef, b.x, b.coef, a.dx, b.dx, a.act, a.ldact, a.slabs, nblk, C, b.act, b.ldact,
                               b.slabs, d);
          },
          256, 0, G, G / (C / kDC)};
}

DxForm full_form() {
  // one workgroup per CU (LDS), one slab per workgroup
  static const int G = persistent_grid((const void*)bn_dx_wgrad_full_kernel, 512, kF_LDS, 1);
  return {[](const DxForm& f, hipStream_t st, const bf16_t* dp, const DxSide& a, const DxSide&, int nblk, int,
             const DxDgrad& d) {
            hipLaunchKernelGGL(bn_dx_wgrad_full_kernel, dim3(f.grid), dim3(f.block), f.lds, st, dp, a.x, a.coef, a.act,
                               a.ldact, a.slabs, nblk, d);
          },
          512, kF_LDS, G, G};
}

// dual: dx2 too; w2: and dW2 (the dual form at 256 x 64); dg: the fused dgrad -- at 256 x 64 one 256-channel slice per
// row block, so that the whole K of dp2 = dx W is in one workgroup (the plain form or the two-weight dual), at
// 512 x 128 the full-width form (plain only); rx: x recomputed from the dgrad's operands (the 256 x 64 dg forms)
DxForm dx_form(int C, int CI, bool dual, bool w2, bool dg, bool rx = false) {
  if (rx && !(dg && C == 256))
    throw std::invalid_argument("bn_dx_wgrad: x is recomputed in the 256 x 64 fused-dgrad forms only");
  if (dg && C == kFC) {
    if (CI != kFCI || dual || w2)
      throw std::invalid_argument("bn_dx_wgrad: the full-width fused dgrad is 512 x 128, plain form");
    return full_form();
  }
  if (dg) {
    if (C != 256 || CI != 64 || dual != w2)
      throw std::invalid_argument("bn_dx_wgrad: the fused dgrad is 256 x 64, plain or two-weight dual form");
    if (rx) return w2 ? sliced_form<64, true, true, true, true>(C) : sliced_form<64, false, false, true, true>(C);
    return w2 ? sliced_form<64, true, true, true>(C) : sliced_form<64, false, false, true>(C);
  }
  if (w2) {
    if (C != 256 || CI != 64 || !dual)
      throw std::invalid_argument("bn_dx_wgrad: the second weight gradient is the dual form's, at 256 x 64");
    return sliced_form<64, true, true>(C);
  }
  if (C == 256 && CI == 64) return dual ? sliced_form<64, true>(C) : sliced_form<64, false>(C);
  if (C == 512 && CI == 128) return dual ? sliced_form<128, true>(C) : sliced_form<128, false>(C);
  throw std::invalid_argument("bn_dx_wgrad: 256 x 64 or 512 x 128 (bn_dx_wgrad_ok)");
}

}  // namespace

bool bn_dx_wgrad_ok(long long M, int C, int CI) {
  return ((C == 256 && CI == 64) || (C == 512 && CI == 128)) && M % kDR == 0 && M >= 64LL * kDR;
}

bool bn_dx_dgrad_ok(long long M, int C, int CI) { return C == 256 && CI == 64 && bn_dx_wgrad_ok(M, C, CI); }

bool bn_dx_dgrad_full_ok(long long M, int C, int CI) { return C == kFC && CI == kFCI && bn_dx_wgrad_ok(M, C, CI); }

// both 256 x 64 fused-dgrad forms (the full-width form's is not built)
bool bn_dx_recompute_ok(long long M, int C, int CI, int dual) { return (void)dual, bn_dx_dgrad_ok(M, C, CI); }

int bn_dx_wgrad_slabs(int C, int CI, int w2, int dg) { return dx_form(C, CI, w2 != 0, w2 != 0, dg != 0).slabs; }

// dx (+ second->dx) from the finalized coefficients (bn_bwd_coef_from_part: coef = [a, bx, c]) and dW += dx^T act
// (+ with second->act: dW2 += dx2^T act2, dual form at 256 x 64 only, wgrad2 of wgrad's dtype); each side's slabs:
// bn_dx_wgrad_slabs(C, CI, w2, dg) x C x CI fp32 workspace; wgrad fp32 or bf16 (the flat gradient's compute dtype).
// With dg (bn_dx_dgrad_ok: the plain form, or the dual form with second->act; bn_dx_dgrad_full_ok: the plain form):
// dg->dp = bits * (dx W) and its BN's backward partials added into dg->part, dx is not written (main.dx may be null).
// With dg->recompute_x (bn_dx_recompute_ok): main.x is not read but formed again as bf16(main.act dg->w^T).
void bn_dx_wgrad(const bf16_t* dp, const DxSide& main, const DxSide* second, long long M, int C, int CI,
                 int wgrad_bf16, hipStream_t st, const DxDgrad* dg) {
  if (!bn_dx_wgrad_ok(M, C, CI)) throw std::invalid_argument("bn_dx_wgrad: unsupported shape (bn_dx_wgrad_ok)");
  const DxSide b = second ? *second : DxSide{};
  const bool rx = dg && dg->recompute_x;
  if (rx && !bn_dx_recompute_ok(M, C, CI, b.x != nullptr))
    throw std::invalid_argument("bn_dx_wgrad: recompute_x: unsupported shape (bn_dx_recompute_ok)");
  const DxForm f = dx_form(C, CI, b.x != nullptr, b.act != nullptr, dg != nullptr, rx);
  f.launch(f, st, dp, main, b, (int)(M / kDR), C, dg ? *dg : DxDgrad{});
  DTG_LAUNCH_CHECK();
  for (const DxSide* s : {&b, &main})
    if (s->act) {
      Epi e{s->wgrad, CI, wgrad_bf16, 1.f, 1.f, nullptr, 0};
      gemm_splitk_reduce(s->slabs, f.slabs, C, CI, e, st);
    }
}

// ---- host: the forward apply pass with the next block's conv1 ----
namespace {
// One form of the pass: its persistent grid (2 workgroups of C threads per CU at C = 256, one at C = 512) and launcher
struct ApplyGemmForm {
  int grid;
  void (*launch)(int grid, hipStream_t st, const bf16_t* x, const bf16_t* r, const float* coef, const float* coef2,
                 bf16_t* out, uint8_t* bits, const BnNextConv& nx, int nblk);
};

template <int C, int N, bool TWO>
ApplyGemmForm apply_gemm_form_of() {
  static const int G = persistent_grid((const void*)bn_apply_gemm_kernel<C, N, TWO>, C, 0, C == 256 ? 2 : 1);
  return {G, [](int grid, hipStream_t st, const bf16_t* x, const bf16_t* r, const float* coef, const float* coef2,
                bf16_t* out, uint8_t* bits, const BnNextConv& nx, int nblk) {
            hipLaunchKernelGGL((bn_apply_gemm_kernel<C, N, TWO>), dim3(grid), dim3(C), 0, st, x, r, coef, coef2, out,
                               bits, nx.w, nx.ldw, nx.y, nx.part, nblk);
          }};
}

// stage 1: 256 x 64 in both forms, 256 x 128 (its last block, an identity block, into stage 2); stage 2: 512 x 128
ApplyGemmForm apply_gemm_form(int C, int N, bool two) {
  if (C == 256 && N == 64) return two ? apply_gemm_form_of<256, 64, true>() : apply_gemm_form_of<256, 64, false>();
  if (C == 256 && N == 128 && !two) return apply_gemm_form_of<256, 128, false>();
  if (C == 512 && N == 128) return two ? apply_gemm_form_of<512, 128, true>() : apply_gemm_form_of<512, 128, false>();
  throw std::invalid_argument("bn_apply_gemm: 256 x 64, 256 x 128 (residual form) or 512 x 128 (bn_apply_gemm_ok)");
}
}  // namespace

bool bn_apply_gemm_ok(long long M, int C, int N) {
  return ((C == 256 && (N == 64 || N == 128)) || (C == 512 && N == 128)) && M % kDR == 0 && M >= 64LL * kDR &&
         M / kDR < (1LL << 31);
}

int bn_apply_gemm_grid(int C, int N, int two) { return apply_gemm_form(C, N, two != 0).grid; }

void bn_apply_gemm(const bf16_t* x, const bf16_t* r, const float* coef, const float* coef2, bf16_t* out,
                   uint8_t* bits, const BnNextConv& next, long long M, int C, hipStream_t st) {
  if (!bn_apply_gemm_ok(M, C, next.N)) throw std::invalid_argument("bn_apply_gemm: unsupported shape (bn_apply_gemm_ok)");
  if (!r || !next.w || !next.y || !next.part || next.ldw < C || next.ldw % 8)
    throw std::invalid_argument("bn_apply_gemm: missing operand or unaligned weight rows");
  const ApplyGemmForm f = apply_gemm_form(C, next.N, coef2 != nullptr);
  f.launch(f.grid, st, x, r, coef, coef2, out, bits, next, (int)(M / kDR));
  DTG_LAUNCH_CHECK();
}

}  // namespace dtg
