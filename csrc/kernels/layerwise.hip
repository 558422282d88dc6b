// Layer-wise adaptive optimizers (LARS, LAMB) and global-norm clipping over FLAT parameter buffers.
//
// The elementwise applies of optim.hip cannot give the one thing these rules need: a reduction PER PARAMETER of
// a flat group (||w||, ||g||, ||update||) and the global gradient norm.  Everything here is table driven like
// state_copy_kernel (snapshot.hip): rows[p] = (offset, numel, first chunk) per parameter, chunks[c] = (row, chunk
// within the row), one chunk per kLwChunk = 2048 elements of a parameter, both built on the host.  A workgroup
// (256 lanes x 8 elements) handles one whole chunk, reads its row and never searches.  Alignment padding between
// parameters belongs to no chunk: it is never read into a norm and never written.
//
// One table covers every flat group of an optimizer (rows and chunks are numbered across the groups, offsets are
// relative to the row's own group), so ONE seg_finalize launch sees all of them; the per-chunk kernels are
// launched per group over that group's interval [c_lo, c_lo + n_chunks) of the chunk table -- or over the
// sub-interval of a DataParallel bucket, which ends on a parameter boundary.
//
// Reductions are deterministic: every chunk writes its own partial (no atomics, nothing to zero), a lane adds
// its 8 elements serially (kLwSerial), the 256 lanes reduce through a fixed 6-level butterfly and a 2-level
// tree, and seg_finalize adds a parameter's partials in a fixed order.  r (trust ratio per parameter) and c
// (clip factor) stay in device memory; lr and the step count come through `hyper` as in optim.hip, so a step
// has no host read and stays capturable.
//
// Body accesses are 16-byte vectors (offsets are 64-element aligned, parallel/flat.py ALIGN); the lane that
// holds a parameter's last, partial 8-element group takes a predicated scalar path (constant indices only: a
// runtime-indexed register array would go through scratch).
#include "dtg/common.h"
#include "dtg/kernels.h"
#include <math.h>

namespace dtg {

static_assert(kLwChunk == 256 * kLwSerial, "a chunk is one 8-element group per lane of a 256-lane workgroup");

struct LwPos {
  long long off;  // the row's offset in its group's buffers
  int row;        // row (parameter) index, across the groups
  int e;          // this lane's first element within the row
  int cnt;        // valid elements of this lane's group: 8 on the body, 0..7 at the row's end
};

__device__ __forceinline__ LwPos lw_pos(const long long* __restrict__ rows, const int* __restrict__ chunks, int ci) {
  LwPos p;
  p.row = chunks[2 * ci];
  const int cin = chunks[2 * ci + 1];
  p.off = rows[3 * p.row];
  const int numel = (int)rows[3 * p.row + 1];
  p.e = cin * kLwChunk + threadIdx.x * 8;
  const int left = numel - p.e;
  p.cnt = left >= 8 ? 8 : (left > 0 ? left : 0);
  return p;
}

__device__ __forceinline__ void lw_load_f32(const float* p, int cnt, float (&o)[8]) {
  if (cnt == 8) {
    load8_f32(p, o);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = k < cnt ? p[k] : 0.f;
  }
}

template <bool GBF16>
__device__ __forceinline__ void lw_load_grad(const void* g, long long i, int cnt, float (&o)[8]) {
  if (cnt == 8) {
    if constexpr (GBF16) load8_bf16(reinterpret_cast<const bf16_t*>(g) + i, o);
    else load8_f32(reinterpret_cast<const float*>(g) + i, o);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k < cnt) {
        if constexpr (GBF16) o[k] = bf2f(reinterpret_cast<const bf16_t*>(g)[i + k]);
        else o[k] = reinterpret_cast<const float*>(g)[i + k];
      } else {
        o[k] = 0.f;
      }
    }
  }
}

__device__ __forceinline__ void lw_store_f32(float* p, int cnt, const float (&o)[8]) {
  if (cnt == 8) {
    store8_f32(p, o);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < cnt) p[k] = o[k];
  }
}

__device__ __forceinline__ void lw_store_bf16(bf16_t* p, int cnt, const float (&o)[8]) {
  if (cnt == 8) {
    store8_bf16(p, o);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < cnt) p[k] = f2bf(o[k]);
  }
}

template <bool GBF16>
__device__ __forceinline__ void lw_zero_grad(void* g, long long i, int cnt) {
  if (cnt == 8) {
    if constexpr (GBF16) {
      *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(g) + i) = make_uint4(0, 0, 0, 0);
    } else {
      float* p = reinterpret_cast<float*>(g) + i;
      *reinterpret_cast<float4*>(p) = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(p + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < cnt) {
        if constexpr (GBF16) reinterpret_cast<bf16_t*>(g)[i + k] = 0;
        else reinterpret_cast<float*>(g)[i + k] = 0.f;
      }
  }
}

// the workgroup's sums of a and b: 6 butterfly levels in the wave, then (s0 + s1) + (s2 + s3) over the 4 waves;
// lane 0 of the workgroup holds the result
__device__ __forceinline__ void lw_block_sum2(float& a, float& b) {
  __shared__ float sh[8];
  a = wave_sum(a);
  b = wave_sum(b);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[wv] = a;
    sh[4 + wv] = b;
  }
  __syncthreads();
  a = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  b = (sh[4] + sh[5]) + (sh[6] + sh[7]);
}

// ---------------------------------------------------------------------------------------------
// seg_sqnorm: partials[ci] = sum w^2, partials[C + ci] = sum g^2 over chunk ci (an absent input's slot is left
// as it is)
// ---------------------------------------------------------------------------------------------
template <bool GBF16>
__global__ void __launch_bounds__(256) seg_sqnorm_kernel(const float* __restrict__ w, const void* __restrict__ grad,
                                                         const long long* __restrict__ rows,
                                                         const int* __restrict__ chunks, int c_lo,
                                                         float* __restrict__ partials, int C) {
  const int ci = c_lo + blockIdx.x;
  const LwPos p = lw_pos(rows, chunks, ci);
  const long long i = p.off + p.e;
  float sw = 0.f, sg = 0.f;
  if (p.cnt > 0) {
    float v[8];
    if (w) {
      lw_load_f32(w + i, p.cnt, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) sw += v[k] * v[k];
    }
    if (grad) {
      lw_load_grad<GBF16>(grad, i, p.cnt, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) sg += v[k] * v[k];
    }
  }
  lw_block_sum2(sw, sg);
  if (threadIdx.x == 0) {
    if (w) partials[ci] = sw;
    if (grad) partials[C + ci] = sg;
  }
}

void seg_sqnorm(const float* w, const void* grad, int grad_bf16, const long long* rows, const int* chunks, int c_lo,
                int n_chunks, float* partials, int C, hipStream_t st) {
  if (n_chunks <= 0 || (!w && !grad)) return;
  if (grad_bf16) seg_sqnorm_kernel<true><<<n_chunks, 256, 0, st>>>(w, grad, rows, chunks, c_lo, partials, C);
  else seg_sqnorm_kernel<false><<<n_chunks, 256, 0, st>>>(w, grad, rows, chunks, c_lo, partials, C);
  DTG_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// LAMB.  u = m * bc1 / (sqrt(v * bc2) + eps) + wd * w  is formed in registers by both passes (storing it would
// cost the same bytes as recomputing it from m, v and w, plus a buffer).
// ---------------------------------------------------------------------------------------------
struct LambCoef {
  float b1, b2, omb1, omb2, eps, wd, bc1, bc2;  // omb = 1 - beta; bc = 1 / (1 - beta^t), in: log(beta)
  // 1 - beta and log(beta) are formed on the host in double: 0.999 rounded to fp32 is off by 1.3e-8, which is
  // 1.3e-5 of 1 - beta
  LambCoef(double b1_, double b2_, float eps_, float wd_)
      : b1((float)b1_), b2((float)b2_), omb1((float)(1.0 - b1_)), omb2((float)(1.0 - b2_)), eps(eps_), wd(wd_),
        bc1((float)log(b1_)), bc2((float)log(b2_)) {}
  // 1 - beta^t = -expm1(t * log beta): the fast pow of optim.hip's Adam loses 1 - 0.999^t to cancellation in the
  // first steps (6e-5 relative at t = 1), and ||u|| enters every element of a parameter through the trust ratio
  __device__ __forceinline__ void bias(const float* hyper) {
    const float t = hyper[1];
    bc1 = -1.f / expm1f(t * bc1);
    bc2 = -1.f / expm1f(t * bc2);
  }
  __device__ __forceinline__ float u(float w, float m, float v) const {
    return m * bc1 / (sqrtf(v * bc2) + eps) + wd * w;
  }
};

template <bool GBF16>
__global__ void __launch_bounds__(256) lamb_moments_kernel(const float* __restrict__ w, void* __restrict__ grad,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           const long long* __restrict__ rows,
                                                           const int* __restrict__ chunks, int c_lo,
                                                           float* __restrict__ partials, int C,
                                                           const float* __restrict__ hyper, LambCoef co, float gscale,
                                                           const float* __restrict__ cfac, int zero_grad) {
  co.bias(hyper);
  const float gs = cfac ? gscale * cfac[0] : gscale;
  const int ci = c_lo + blockIdx.x;
  const LwPos p = lw_pos(rows, chunks, ci);
  const long long i = p.off + p.e;
  float sw = 0.f, su = 0.f;
  if (p.cnt > 0) {
    float wv[8], gv[8], mv[8], vv[8];
    lw_load_f32(w + i, p.cnt, wv);
    lw_load_grad<GBF16>(grad, i, p.cnt, gv);
    lw_load_f32(m + i, p.cnt, mv);
    lw_load_f32(v + i, p.cnt, vv);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float g = gv[k] * gs;
      mv[k] = co.b1 * mv[k] + co.omb1 * g;
      vv[k] = co.b2 * vv[k] + co.omb2 * g * g;
      if (k < p.cnt) {  // (a lane past the row's end would add 0 / (0 + eps): NaN at eps = 0)
        const float u = co.u(wv[k], mv[k], vv[k]);
        sw += wv[k] * wv[k];
        su += u * u;
      }
    }
    lw_store_f32(m + i, p.cnt, mv);
    lw_store_f32(v + i, p.cnt, vv);
    if (zero_grad) lw_zero_grad<GBF16>(grad, i, p.cnt);
  }
  lw_block_sum2(sw, su);
  if (threadIdx.x == 0) {
    partials[ci] = sw;
    partials[C + ci] = su;
  }
}

void lamb_moments(const float* w, void* grad, int grad_bf16, float* m, float* v, const long long* rows,
                  const int* chunks, int c_lo, int n_chunks, float* partials, int C, const float* hyper, double b1,
                  double b2, float eps, float wd, float gscale, const float* cfac, int zero_grad, hipStream_t st) {
  if (n_chunks <= 0) return;
  const LambCoef co(b1, b2, eps, wd);
  if (grad_bf16)
    lamb_moments_kernel<true><<<n_chunks, 256, 0, st>>>(w, grad, m, v, rows, chunks, c_lo, partials, C, hyper, co,
                                                        gscale, cfac, zero_grad);
  else
    lamb_moments_kernel<false><<<n_chunks, 256, 0, st>>>(w, grad, m, v, rows, chunks, c_lo, partials, C, hyper, co,
                                                         gscale, cfac, zero_grad);
  DTG_LAUNCH_CHECK();
}

template <bool MIRROR>
__global__ void __launch_bounds__(256) lamb_apply_kernel(float* __restrict__ w, bf16_t* __restrict__ mirror,
                                                         const float* __restrict__ m, const float* __restrict__ v,
                                                         const long long* __restrict__ rows,
                                                         const int* __restrict__ chunks, int c_lo,
                                                         const float* __restrict__ hyper, LambCoef co,
                                                         const float* __restrict__ ratio) {
  co.bias(hyper);
  const LwPos p = lw_pos(rows, chunks, c_lo + blockIdx.x);
  if (p.cnt == 0) return;
  const float step = hyper[0] * ratio[p.row];
  const long long i = p.off + p.e;
  float wv[8], mv[8], vv[8];
  lw_load_f32(w + i, p.cnt, wv);
  lw_load_f32(m + i, p.cnt, mv);
  lw_load_f32(v + i, p.cnt, vv);
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < p.cnt) wv[k] -= step * co.u(wv[k], mv[k], vv[k]);
  lw_store_f32(w + i, p.cnt, wv);
  if constexpr (MIRROR) lw_store_bf16(mirror + i, p.cnt, wv);
}

void lamb_apply(float* w, bf16_t* mirror, const float* m, const float* v, const long long* rows, const int* chunks,
                int c_lo, int n_chunks, const float* hyper, double b1, double b2, float eps, float wd,
                const float* ratio, hipStream_t st) {
  if (n_chunks <= 0) return;
  const LambCoef co(b1, b2, eps, wd);
  if (mirror) lamb_apply_kernel<true><<<n_chunks, 256, 0, st>>>(w, mirror, m, v, rows, chunks, c_lo, hyper, co, ratio);
  else lamb_apply_kernel<false><<<n_chunks, 256, 0, st>>>(w, mirror, m, v, rows, chunks, c_lo, hyper, co, ratio);
  DTG_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// LARS: m = mu * m + lr * r[row] * (g * gscale * c + wd * w) ; w -= m
// ---------------------------------------------------------------------------------------------
template <bool GBF16, bool MIRROR>
__global__ void __launch_bounds__(256) lars_apply_kernel(float* __restrict__ w, bf16_t* __restrict__ mirror,
                                                         void* __restrict__ grad, float* __restrict__ mom,
                                                         const long long* __restrict__ rows,
                                                         const int* __restrict__ chunks, int c_lo,
                                                         const float* __restrict__ hyper, float mu, float wd,
                                                         float gscale, const float* __restrict__ cfac,
                                                         const float* __restrict__ ratio, int zero_grad) {
  const LwPos p = lw_pos(rows, chunks, c_lo + blockIdx.x);
  if (p.cnt == 0) return;
  const float gs = cfac ? gscale * cfac[0] : gscale;
  const float step = hyper[0] * ratio[p.row];
  const long long i = p.off + p.e;
  float wv[8], gv[8], mv[8];
  lw_load_f32(w + i, p.cnt, wv);
  lw_load_grad<GBF16>(grad, i, p.cnt, gv);
  lw_load_f32(mom + i, p.cnt, mv);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    mv[k] = mu * mv[k] + step * (gv[k] * gs + wd * wv[k]);
    wv[k] -= mv[k];
  }
  lw_store_f32(w + i, p.cnt, wv);
  lw_store_f32(mom + i, p.cnt, mv);
  if constexpr (MIRROR) lw_store_bf16(mirror + i, p.cnt, wv);
  if (zero_grad) lw_zero_grad<GBF16>(grad, i, p.cnt);
}

void lars_apply(float* w, bf16_t* mirror, void* grad, int grad_bf16, float* mom, const long long* rows,
                const int* chunks, int c_lo, int n_chunks, const float* hyper, float mu, float wd, float gscale,
                const float* cfac, const float* ratio, int zero_grad, hipStream_t st) {
  if (n_chunks <= 0) return;
#define DTG_L(G, M)                                                                                                \
  do {                                                                                                            \
    lars_apply_kernel<G, M><<<n_chunks, 256, 0, st>>>(w, mirror, grad, mom, rows, chunks, c_lo, hyper, mu, wd, gscale, \
                                                      cfac, ratio, zero_grad);                                     \
    DTG_LAUNCH_CHECK();                                                                                            \
  } while (0)
  if (grad_bf16) { if (mirror) DTG_L(true, true); else DTG_L(true, false); }
  else { if (mirror) DTG_L(false, true); else DTG_L(false, false); }
#undef DTG_L
}

// ---------------------------------------------------------------------------------------------
// seg_finalize: ONE small launch over every group.
//   clip_norm > 0: every workgroup sums the gradient partials partials[C .. 2C) of ALL groups in the same fixed
//     order (lane-strided, butterfly, tree), c = clip_norm / max(gscale * ||g||, clip_norm); workgroup 0 stores
//     c.  Otherwise c is read from cfac (1 when nothing clips).
//   rule != 0: one wave per parameter adds its chunk partials in chunk order (lane l takes chunks l, l + 64, ...;
//     then the butterfly) into norms[p] = (sum of slot 0, sum of slot 1) and writes the trust ratio:
//     kLwLars  r = eta * ||w|| / (gscale * c * ||g|| + wd * ||w|| + eps)
//     kLwLamb  r = ||w|| / ||u||
//     when the parameter's group adapts and both norms are > 0, else r = 1.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) seg_finalize_kernel(const float* __restrict__ partials, int C,
                                                           const long long* __restrict__ rows, int P, LwGroups grp,
                                                           int rule, float clip_norm, float gscale, float eta,
                                                           float eps, float* __restrict__ norms,
                                                           float* __restrict__ ratio, float* __restrict__ cfac) {
  __shared__ float sh[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float c;
  if (clip_norm > 0.f) {
    // four independent accumulators per lane (chunks i, i + 256, i + 512, i + 768 of each 1024): four loads in
    // flight instead of one dependent chain; the order is as fixed as before
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const float* gp = partials + C;
    int i = threadIdx.x;
    for (; i + 768 < C; i += 1024) {
      s0 += gp[i];
      s1 += gp[i + 256];
      s2 += gp[i + 512];
      s3 += gp[i + 768];
    }
    for (; i < C; i += 256) s0 += gp[i];
    float s = (s0 + s1) + (s2 + s3);
    s = wave_sum(s);
    if (lane == 0) sh[wv] = s;
    __syncthreads();
    const float gn = gscale * sqrtf((sh[0] + sh[1]) + (sh[2] + sh[3]));
    c = clip_norm / fmaxf(gn, clip_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) cfac[0] = c;
  } else {
    c = cfac[0];
  }
  if (rule == kLwNone) return;
  const int row = blockIdx.x * 4 + wv;
  if (row >= P) return;
  const int numel = (int)rows[3 * row + 1];
  const int c0 = (int)rows[3 * row + 2];
  const int k = (numel + kLwChunk - 1) / kLwChunk;
  float a = 0.f, b = 0.f;
  for (int j = lane; j < k; j += 64) {
    a += partials[c0 + j];
    b += partials[C + c0 + j];
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane != 0) return;
  norms[2 * row] = a;
  norms[2 * row + 1] = b;
  // wave-uniform select over the by-value group table (a runtime index would go through scratch)
  const int gi = row < grp.row_end[0] ? 0 : row < grp.row_end[1] ? 1 : row < grp.row_end[2] ? 2 : 3;
  const int adapt = gi == 0 ? grp.adapt[0] : gi == 1 ? grp.adapt[1] : gi == 2 ? grp.adapt[2] : grp.adapt[3];
  const float wd = gi == 0 ? grp.wd[0] : gi == 1 ? grp.wd[1] : gi == 2 ? grp.wd[2] : grp.wd[3];
  float r = 1.f;
  if (adapt && a > 0.f && b > 0.f) {
    const float n0 = sqrtf(a), n1 = sqrtf(b);
    r = rule == kLwLars ? eta * n0 / (gscale * c * n1 + wd * n0 + eps) : n0 / n1;
  }
  ratio[row] = r;
}

void seg_finalize(const float* partials, int C, const long long* rows, int P, const LwGroups& grp, int rule,
                  float clip_norm, float gscale, float eta, float eps, float* norms, float* ratio, float* cfac,
                  hipStream_t st) {
  if (rule == kLwNone && !(clip_norm > 0.f)) return;
  const int grid = rule == kLwNone ? 1 : (P + 3) / 4 > 0 ? (P + 3) / 4 : 1;
  seg_finalize_kernel<<<grid, 256, 0, st>>>(partials, C, rows, P, grp, rule, clip_norm, gscale, eta, eps, norms, ratio,
                                            cfac);
  DTG_LAUNCH_CHECK();
}

}  // namespace dtg
