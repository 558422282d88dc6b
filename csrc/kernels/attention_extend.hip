// Several new tokens per record against a KV cache: the extend / chunked-prefill / verify shape between
// attention_decode.hip (one query row) and the causal training kernels (as many keys as queries, all in qkv).  Head dim
// 64, bf16, no dropout, no additive mask.  kcache / vcache are bf16 [B, nh, S_max, 64]; record b holds len = lens0[b] +
// t cached keys before the call.  qkvT [B * T, 3H] (row layout [3][nh][64], 1 <= T <= 64) holds its new tokens: rows
// i < n (n = n_new[b] clamped to [0, T]; no n_new: T) sit at positions len + i.  Query i sees positions
// lo_i = max(0, len + i + 1 - window) .. len + i (window = 0: lo_i = 0): cached keys below len, new keys -- always
// from qkvT, never from the cache -- from len on.  Rows i >= n get zero ctx and lse and are not appended; a record
// with len < 0 or len + n > S_max is treated as n = 0 (attn_decode's rule): it writes nothing and gets zeros.
//
//   grid [B * nh, nsplit], 4 waves per workgroup, attn_decode's split of a record's 64-key chunks over blockIdx.y: with
//   lo = lo_0 (the lowest edge any query sees), c_lo = lo / 64 .. c_hi = len / 64, split s owns chunks c_lo + s * cps
//   .. c_lo + (s + 1) * cps - 1 cut at c_hi, the last split runs up to c_hi, and a split outside the range writes the
//   empty partial (m = -inf, l = 0, acc = 0).  The split count is attn_decode_splits' (and its force knob's).
//
//   Waves divide the chunks (wave w: cb + w, cb + w + 4, ...) and EVERY wave holds all NT = ceil(T / 16) query tiles,
//   so a K / V byte is read once per launch whatever T is: the Q fragments (NT x 2 x 4 VGPRs) and the fp32 O^T
//   accumulators (NT x 16 VGPRs) stay in registers for the whole loop.  The kernel is instantiated per NT, so T <= 16
//   pays for one tile.  Splitting the query tiles over the waves instead would read every chunk NT times.
//
//   S^T = K Q^T on v_mfma_f32_16x16x32_bf16.  A lane's A-operand fragment is 8 consecutive dims of one key: one
//   16-byte load straight from the cache row (or the qkvT row), so K needs no LDS and no transpose.  Lane (qi, g) then
//   holds query qi of the tile against keys 16 j + 4 g + [0, 4) of the chunk, j = 0 .. 3, as attn_causal_common.cuh's
//   fwd_chunk does, and the online softmax is its arithmetic in log2 units (scores * log2(e) / 8, exp2).
//
//   O^T += V^T P^T needs V with keys along the fragment vector: 8 keys of one dim per lane, which from global memory
//   would be 2-byte gathers.  So V goes through a per-wave LDS tile [64 keys][64 dims] in the MC layout fwd_chunk
//   consumes, filled by 8 LDS-DMA instructions per chunk (1 KiB each, no VGPR round trip, an invisible row reads the
//   zero page) and read with the CDNA4 transposing LDS reads (frag_mc: ds_read_b64_tr_b16).  The tile is per wave,
//   not per workgroup: a wave waits on its own vmcnt and the chunk loop has no barrier, so the four waves stream
//   independent chunks.  P goes through a 2 KiB per-wave scratch (C layout -> B fragment).  40 KiB of LDS per
//   workgroup: four workgroups per CU.
//
//   Exclusion is the causal kernels' rule.  An invisible key is out of the running max by a select (P = 0 exactly);
//   a row that has seen no key yet subtracts 0 while its max is still -inf.  Cache rows at or above len, or below lo_0,
//   qkvT rows at or above n, are never loaded (their K fragment is zeros, their V row the zero page).  On a chunk that
//   is not wholly visible to every row, each 16-key block is, per query tile, wholly visible (MFMA), invisible (its
//   V^T fragment half is zeros) or partly visible: then the fragment is zeros too and the block is accumulated on the
//   VALU under the predicate, so 0 * NaN never enters an MFMA.  The window's edge crosses at most two blocks of a
//   tile and the diagonal one.
//
//   The T new keys are one more chunk, at positions len .. len + n - 1, read from qkvT by the workgroup whose split
//   holds c_hi (it takes the next turn in the waves' round robin).  That workgroup also appends: the k / v rows of
//   tokens 0 .. n - 1 go to cache rows len .. with 16-byte stores.  No other workgroup reads or writes those rows in
//   this launch, so nothing needs ordering.
//
//   After the loop the waves' (m, l, O) meet in LDS (over the V tiles), one query tile at a time; 256 threads merge
//   them, 4 dims of a row each.  nsplit = 1: ctx (bf16) and lse.  nsplit > 1: the fp32 partial of row i goes to
//   ws[((bh * nsplit + s) * T + i) * 66 + {0: m (log2 units), 1: l, 2..65: acc}] and attn_extend_combine_kernel
//   (grid [B * nh, T], 64 threads) merges the splits: no atomics, no "last workgroup" scheme.
//
// emb_fwd_span_kernel is emb_fwd_at_kernel over [B, T] ids: position lens0[b] + t + i, the same order of additions and
// the same single rounding.
#include "dtg/attn_common.cuh"
#include "dtg/kernels.h"

namespace dtg {

namespace {
using namespace attn;

constexpr int kNW = 4;                 // waves per workgroup
constexpr int kPart = 66;              // floats of a partial: m, l, acc[64]
constexpr int kMaxSplits = 1024;
constexpr int kMaxT = 64;
constexpr int kVt = 8192;              // per-wave V tile: [64 keys][64 dims] bf16, MC
constexpr int kScr = 2048;             // per-wave P scratch: [16 q][64 keys] bf16, KC
constexpr int kWaveLds = kVt + kScr;
constexpr int kRedLd = 68;             // floats of a merge row: acc[64], m, l, pad (16-byte rows)
static_assert(kNW * 16 * kRedLd * 4 <= kNW * kWaveLds, "the merge area lies over the V tiles");
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

typedef const __attribute__((address_space(3))) bf16_t lds_bf16;
typedef const __attribute__((address_space(3))) u32x2v lds_u32x2;
typedef __attribute__((address_space(3))) f32x4 lds_f32x4w;

// the lowest position query i of a record with len cached keys sees
__device__ __forceinline__ int low_edge(int len, int i, int window) {
  const int lo = len + i + 1 - window;
  return (window > 0 && lo > 0) ? lo : 0;
}

// One chunk of up to 64 keys at positions k0 .. k0 + 63 for all NT query tiles of a wave.  kp / vp: the K and V
// row of position k0 (rows ld elements apart: 64 in the cache, 3H in qkvT).  kFull: every position is visible to
// every row.  Otherwise positions in [vlo, vhi) are loaded, and position x is visible to query i < n iff
// lo_i <= x <= min(len + i, vhi - 1).
template <int NT, bool kFull>
__device__ __forceinline__ void extend_chunk(const bf16_t* __restrict__ kp, const bf16_t* __restrict__ vp,
                                             long long ld, int k0, int vlo, int vhi, int len, int n, int window,
                                             lds_char* Vt, lds_char* scr, const v8bf (&qa)[NT][2], float (&m)[NT],
                                             float (&l)[NT], f32x4 (&o)[NT][4], int lane, float scale_l2) {
  const int qi = lane & 15, g = lane >> 4;
  const v8bf zero = {0, 0, 0, 0, 0, 0, 0, 0};
  lds_fence();  // the last chunk's reads of the V tile are done before the DMA rewrites it
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int kr = i * 8 + (lane >> 3);
    const int c = (lane & 7) ^ mc_swz<8>(kr);
    const bool in = kFull || (k0 + kr >= vlo && k0 + kr < vhi);
    __builtin_amdgcn_global_load_lds(sel(in, vp + kr * ld + c * 8), (lds_void*)(Vt + i * 1024), 16, 0, 0);
  }
  v8bf kf[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int kr = j * 16 + qi;
    const bool in = kFull || (k0 + kr >= vlo && k0 + kr < vhi);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      kf[j][ks] = in ? *reinterpret_cast<const v8bf*>(kp + kr * ld + ks * 32 + 8 * g) : zero;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int qt = 0; qt < NT; ++qt) {
    if (qt * 16 >= n) continue;  // (wave-uniform) a tile without rows
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[j][ks], qa[qt][ks], s[j], 0, 0, 0);
    }
    // (masked, wave-uniform) bit bk: 16-key block bk is visible to every row of the tile / to some and not all
    int full = 15, part = 0;
    const int i = qt * 16 + qi;
    const int lo_i = low_edge(len, i, window);
    const int up_i = i < n ? (len + i < vhi - 1 ? len + i : vhi - 1) : -1;
    if constexpr (!kFull) {
      const int i0 = qt * 16, i1 = i0 + 15 < n - 1 ? i0 + 15 : n - 1;
      const int lo_first = low_edge(len, i0, window), lo_last = low_edge(len, i1, window);
      const int up_first = len + i0 < vhi - 1 ? len + i0 : vhi - 1, up_last = len + i1 < vhi - 1 ? len + i1 : vhi - 1;
      full = 0;
#pragma unroll
      for (int bk = 0; bk < 4; ++bk) {
        const int p0 = k0 + bk * 16;
        const bool all = p0 >= lo_last && p0 + 15 <= up_first;
        const bool none = p0 + 15 < lo_first || p0 > up_last;
        full |= (int)all << bk;
        part |= (int)(!all && !none) << bk;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int x = k0 + j * 16 + 4 * g + r;
        const float v = s[j][r] * scale_l2;
        s[j][r] = (kFull || (x >= lo_i && x <= up_i)) ? v : -INFINITY;  // excluded: out of the max, P = 0 below
        mx = fmaxf(mx, s[j][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m[qt], mx);
    const float mref = mn == -INFINITY ? 0.f : mn;  // the row that sees no key yet: alpha = 0 on l = o = 0
    const float alpha = __builtin_amdgcn_exp2f(m[qt] - mref);
    m[qt] = mn;
    float rs = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pd[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pd[r] = __builtin_amdgcn_exp2f(s[j][r] - mref);
        rs += pd[r];
      }
      st4_bf16(scr + kc_off(qi, j * 16 + 4 * g), pd);  // P [16 q][64 keys] KC
    }
    l[qt] = l[qt] * alpha + rs;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[qt][j][r] *= alpha;
    lds_fence();
    const v8bf pb0 = frag_kc(scr, 0, 0, lane), pb1 = frag_kc(scr, 0, 1, lane);  // X_B[q][key]
    // the lane's 8 keys of a V^T fragment lie in 16-key block 2 ks + (g >> 1)
    const bool z0 = !kFull && !((full >> (g >> 1)) & 1), z1 = !kFull && !((full >> (2 + (g >> 1))) & 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v8bf v0 = frag_mc<64>(Vt, j * 16, 0, lane), v1 = frag_mc<64>(Vt, j * 16, 1, lane);
      if (z0) v0 = zero;
      if (z1) v1 = zero;
      o[qt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, pb0, o[qt][j], 0, 0, 0);
      o[qt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v1, pb1, o[qt][j], 0, 0, 0);
    }
    if constexpr (!kFull) {
      // the partly visible blocks: O^T[d][q] += V[key][d] * P[q][key] for the visible keys only, P as the MFMA would
      // read it (bf16 out of the scratch); the lane's d are 16 j + 4 g + [0, 4), 8 bytes of V's MC row
      for (int bk = 0; bk < 4; ++bk) {
        if (!((part >> bk) & 1)) continue;  // wave-uniform
#pragma unroll 2
        for (int kk = 0; kk < 16; ++kk) {
          const int kl = bk * 16 + kk, x = k0 + kl;
          const float pv = bf2f(*reinterpret_cast<lds_bf16*>(scr + kc_off(qi, kl)));
          const lds_char* vrow = Vt + kl * 128 + (g & 1) * 8;
          const int sw = mc_swz<8>(kl);
          if (x >= lo_i && x <= up_i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const u32x2v w = *reinterpret_cast<lds_u32x2*>(vrow + (((2 * j + (g >> 1)) ^ sw) << 4));
              o[qt][j][0] = fmaf(pv, __uint_as_float(w.x << 16), o[qt][j][0]);
              o[qt][j][1] = fmaf(pv, __uint_as_float(w.x & 0xffff0000u), o[qt][j][1]);
              o[qt][j][2] = fmaf(pv, __uint_as_float(w.y << 16), o[qt][j][2]);
              o[qt][j][3] = fmaf(pv, __uint_as_float(w.y & 0xffff0000u), o[qt][j][3]);
            }
          }
        }
      }
    }
  }
}

template <int NT>
__global__ void __launch_bounds__(64 * kNW) attn_extend_kernel(
    const bf16_t* __restrict__ qkvT, const int* __restrict__ lens0, int t, const int* __restrict__ n_new,
    bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache, float* __restrict__ ws, bf16_t* __restrict__ ctx,
    float* __restrict__ lse, int T, int nh, int S_max, int window, int cps, float scale_l2) {
  __shared__ __attribute__((aligned(16))) char smem_raw[kNW * kWaveLds];
  lds_char* smem = (lds_char*)smem_raw;
  const int bh = blockIdx.x, b = bh / nh, h = bh - b * nh, sp = blockIdx.y, nsplit = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, qi = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  lds_char* Vt = smem + wave * kWaveLds;
  lds_char* scr = Vt + kVt;
  const int H = nh * 64;
  const long long ld3 = 3LL * H;
  const int len = lens0[b] + t;
  int n = n_new ? n_new[b] : T;
  n = n < 0 ? 0 : (n < T ? n : T);
  if (len < 0 || len > S_max - n) n = 0;  // the refused record: no rows, nothing appended (uniform over the workgroup)
  float m[NT], l[NT];
  f32x4 o[NT][4];
#pragma unroll
  for (int qt = 0; qt < NT; ++qt) {
    m[qt] = -INFINITY;
    l[qt] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[qt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (n > 0) {
    const bf16_t* rec = qkvT + (long long)b * T * ld3 + h * 64;  // the head's q columns of the record's row 0
    const v8bf zero = {0, 0, 0, 0, 0, 0, 0, 0};
    v8bf qa[NT][2];
#pragma unroll
    for (int qt = 0; qt < NT; ++qt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        qa[qt][ks] = qt * 16 + qi < n ? *reinterpret_cast<const v8bf*>(rec + (qt * 16 + qi) * ld3 + ks * 32 + 8 * g) : zero;
    const int lo = low_edge(len, 0, window), lo_top = low_edge(len, n - 1, window);
    const int c_lo = lo >> 6, c_hi = len >> 6;
    const int cb = c_lo + sp * cps;
    const int ce = (sp == nsplit - 1 || cb + cps > c_hi) ? c_hi + 1 : cb + cps;
    const bool owner = cb <= c_hi && c_hi < ce;  // this workgroup's split holds c_hi: the new tokens are its
    const long long hb = (long long)bh * S_max * 64;
    // chunk index ce of the owner stands for the block of new keys
    for (int c = cb + wave; c < ce + (owner ? 1 : 0); c += kNW) {
      if (c == ce) {
        extend_chunk<NT, false>(rec + H, rec + 2 * H, ld3, len, len, len + n, len, n, window, Vt, scr, qa, m, l, o, lane,
                                scale_l2);
        continue;
      }
      const int k0 = c * 64;
      if (k0 >= len) continue;  // c_hi at len % 64 == 0 holds no cached key
      const bf16_t* kp = kcache + hb + (long long)k0 * 64;
      const bf16_t* vp = vcache + hb + (long long)k0 * 64;
      if (k0 >= lo_top && k0 + 64 <= len)
        extend_chunk<NT, true>(kp, vp, 64, k0, lo, len, len, n, window, Vt, scr, qa, m, l, o, lane, scale_l2);
      else
        extend_chunk<NT, false>(kp, vp, 64, k0, lo, len, len, n, window, Vt, scr, qa, m, l, o, lane, scale_l2);
    }
    if (owner) {
      // the append: 16 bytes of K and of V per thread, rows len .. len + n - 1 (len + n <= S_max)
      for (int idx = tid; idx < n * 8; idx += 64 * kNW) {
        const int row = idx >> 3, sub = idx & 7;
        const bf16_t* src = rec + row * ld3 + H + sub * 8;
        const long long dst = hb + (long long)(len + row) * 64 + sub * 8;
        *reinterpret_cast<u32x4v*>(kcache + dst) = *reinterpret_cast<const u32x4v*>(src);
        *reinterpret_cast<u32x4v*>(vcache + dst) = *reinterpret_cast<const u32x4v*>(src + H);
      }
    }
  }
  // the waves' (m, l, O) of a query tile meet in LDS; thread (q = tid / 16, dg = tid % 16) merges dims 4 dg + [0, 4)
  lds_float* red = reinterpret_cast<lds_float*>(smem);
  const int q = tid >> 4, dg = tid & 15;
  __syncthreads();  // the V tiles are no longer read
#pragma unroll
  for (int qt = 0; qt < NT; ++qt) {
    float lt = l[qt];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    lds_float* mine = red + (wave * 16 + qi) * kRedLd;
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<lds_f32x4w*>(mine + j * 16 + 4 * g) = o[qt][j];
    if (g == 0) {
      mine[64] = m[qt];
      mine[65] = lt;
    }
    __syncthreads();
    const int i = qt * 16 + q;
    float M = -INFINITY;
    if (i < n) {
#pragma unroll
      for (int w = 0; w < kNW; ++w) M = fmaxf(M, red[(w * 16 + q) * kRedLd + 64]);
    }
    float L = 0.f, a[4] = {0.f, 0.f, 0.f, 0.f};
    if (M != -INFINITY) {
#pragma unroll
      for (int w = 0; w < kNW; ++w) {
        const lds_float* row = red + (w * 16 + q) * kRedLd;
        const float f = __builtin_amdgcn_exp2f(row[64] - M);  // an idle wave: exp2(-inf) = 0
        L = fmaf(f, row[65], L);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = fmaf(f, row[dg * 4 + k], a[k]);
      }
    }
    if (i < T) {
      if (nsplit == 1) {
        // L = 0: a row at or beyond n, or a refused record: zeros
        const float il = L > 0.f ? 1.f / L : 0.f;
        u32x2v w;
        w.x = pack_bf2(a[0] * il, a[1] * il);
        w.y = pack_bf2(a[2] * il, a[3] * il);
        *reinterpret_cast<u32x2v*>(ctx + ((long long)b * T + i) * H + h * 64 + dg * 4) = w;
        if (dg == 0) lse[(long long)bh * T + i] = L > 0.f ? fmaf(M, kLn2, __logf(L)) : 0.f;
      } else {
        float* part = ws + (((long long)bh * nsplit + sp) * T + i) * kPart;
        if (dg == 0) {
          part[0] = M;
          part[1] = L;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) part[2 + dg * 4 + k] = a[k];
      }
    }
    __syncthreads();  // the merge area is rewritten by the next tile
  }
}

// merges the nsplit partials of query row blockIdx.y of a (record, head): thread d owns dim d
__global__ void __launch_bounds__(64) attn_extend_combine_kernel(const float* __restrict__ ws, bf16_t* __restrict__ ctx,
                                                                 float* __restrict__ lse, int T, int nh, int nsplit) {
  const int bh = blockIdx.x, b = bh / nh, h = bh - b * nh, i = blockIdx.y, d = threadIdx.x;
  const float* part = ws + ((long long)bh * nsplit * T + i) * kPart;
  const long long ps = (long long)T * kPart;  // from a split's partial of the row to the next split's
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, part[s * ps]);
  float L = 0.f, a = 0.f;
  if (M != -INFINITY) {
    for (int s = 0; s < nsplit; ++s) {
      const float f = __builtin_amdgcn_exp2f(part[s * ps] - M);  // an empty partial: exp2(-inf) = 0
      L = fmaf(f, part[s * ps + 1], L);
      a = fmaf(f, part[s * ps + 2 + d], a);
    }
  }
  ctx[((long long)b * T + i) * nh * 64 + h * 64 + d] = f2bf(L > 0.f ? a / L : 0.f);
  if (d == 0) lse[(long long)bh * T + i] = L > 0.f ? fmaf(M, kLn2, __logf(L)) : 0.f;
}

// a wave per (record, token); ids and positions are clamped into their tables
__global__ void __launch_bounds__(256) emb_fwd_span_kernel(const long long* __restrict__ ids,
                                                           const int* __restrict__ lens0, int t,
                                                           const bf16_t* __restrict__ word,
                                                           const bf16_t* __restrict__ pos,
                                                           const bf16_t* __restrict__ type, bf16_t* __restrict__ out,
                                                           int B, int T, int H, int V, int P) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * T) return;
  const int b = row / T, i = row - b * T;
  long long id = ids[row];
  id = id < 0 ? 0 : (id < V ? id : V - 1);
  int p = lens0[b] + t + i;
  p = p < 0 ? 0 : (p < P ? p : P - 1);
  const bf16_t* w = word + id * H;
  const bf16_t* pp = pos + (long long)p * H;
  for (int c = lane; c < (H >> 3); c += 64) {
    float x[8], y[8], z[8];
    load8_bf16(w + c * 8, x);
    load8_bf16(pp + c * 8, y);
    load8_bf16(type + c * 8, z);
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] += y[k] + z[k];
    store8_bf16(out + (long long)row * H + c * 8, x);
  }
}

// chunks a record can span (attention_decode.hip's count: the two kernels cut the same c_lo .. c_hi)
int max_chunks(int max_len, int window) {
  const int all = max_len / 64 + 1;
  if (window <= 0) return all;
  const long long w = ((long long)window + 62) / 64 + 1;
  return w < all ? (int)w : all;
}
}  // namespace

int attn_extend_supported(int dh, int S_max, int T) { return attn_decode_supported(dh, S_max) && T >= 1 && T <= kMaxT; }

void attn_extend(const bf16_t* qkvT, const int* lens0, int t, int max_len, const int* n_new, bf16_t* kcache,
                 bf16_t* vcache, float* ws, int nsplit, bf16_t* ctx, float* lse, int B, int T, int nh, int S_max,
                 int window, hipStream_t st) {
  if (B <= 0 || nh <= 0) return;
  if (!attn_extend_supported(64, S_max, T) || nsplit < 1 || nsplit > kMaxSplits || (nsplit > 1 && !ws))
    throw std::runtime_error(
        "dtg: attn_extend: 1 <= T <= 64, 1 <= S_max <= 2^30, 1 <= nsplit <= 1024 and a workspace for nsplit > 1");
  const int chunks = max_chunks(max_len < 0 ? 0 : max_len, window);
  const int cps = (chunks + nsplit - 1) / nsplit;
  const dim3 grid(B * nh, nsplit), block(64 * kNW);
  const float sl2 = kLog2e * 0.125f;
  switch ((T + 15) / 16) {
    case 1:
      hipLaunchKernelGGL(attn_extend_kernel<1>, grid, block, 0, st, qkvT, lens0, t, n_new, kcache, vcache, ws, ctx, lse,
                         T, nh, S_max, window, cps, sl2);
      break;
    case 2:
      hipLaunchKernelGGL(attn_extend_kernel<2>, grid, block, 0, st, qkvT, lens0, t, n_new, kcache, vcache, ws, ctx, lse,
                         T, nh, S_max, window, cps, sl2);
      break;
    case 3:
      hipLaunchKernelGGL(attn_extend_kernel<3>, grid, block, 0, st, qkvT, lens0, t, n_new, kcache, vcache, ws, ctx, lse,
                         T, nh, S_max, window, cps, sl2);
      break;
    default:
      hipLaunchKernelGGL(attn_extend_kernel<4>, grid, block, 0, st, qkvT, lens0, t, n_new, kcache, vcache, ws, ctx, lse,
                         T, nh, S_max, window, cps, sl2);
  }
  DTG_LAUNCH_CHECK();
  if (nsplit > 1) {
    hipLaunchKernelGGL(attn_extend_combine_kernel, dim3(B * nh, T), dim3(64), 0, st, ws, ctx, lse, T, nh, nsplit);
    DTG_LAUNCH_CHECK();
  }
}

void emb_fwd_span(const long long* ids, const int* lens0, int t, const bf16_t* word, const bf16_t* pos,
                  const bf16_t* type, bf16_t* out, int B, int T, int H, int V, int P, hipStream_t st) {
  if (B <= 0 || T <= 0) return;
  hipLaunchKernelGGL(emb_fwd_span_kernel, dim3((B * T + 3) / 4), dim3(256), 0, st, ids, lens0, t, word, pos, type, out,
                     B, T, H, V, P);
  DTG_LAUNCH_CHECK();
}

}  // namespace dtg
