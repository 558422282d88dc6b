// BERT dynamic masking, device side: one launch from the raw token record to everything the model's forward takes.
//
//   input_ids i32 [B,S], a_len / length i32 [B], index i64 [B]
//     -> ids, token_type_ids, attention_mask i64 [B,S], mlm_positions, mlm_labels i64 [B,P]
//
// The rule is integer only, so dtg/ops/mlm.py::mlm_mask_ref reproduces it bit for bit (h = data/sampler.py::hash32):
//   candidate   j < length and input_ids[j] is no special id;  n_cand = their count
//   n_pred      0 if n_cand == 0, else min(P, n_cand, max(1, (n_cand * mask_per_mille + 500) / 1000))
//   choice      the n_pred candidates with the smallest ((h(seed, epoch, index, j, 0) >> key_shift) << 32) | j
//   action      a = (h(seed, epoch, index, j, 1) * 10) >> 32:  a < 8 -> mask_id,  a == 8 -> kept,
//               a == 9 -> vocab_lo + ((h(seed, epoch, index, j, 2) * vocab_range) >> 32)
//   rows >= valid_rows (the evaluation pass's padding rows) are copied unmasked, with no prediction.
//
// Structure: a wave takes one row, a workgroup of 4 waves takes 4 rows; lane l owns positions l, l + 64, ... (a
// runtime loop over chunks of 64, so any S <= kMlmMaxSeq works).  The row's three hash words are folded once.
//   pass 1  the candidates' 32-bit keys go to the wave's LDS row (S * 4 bytes) *compacted* in position order: slot
//           = candidates in earlier chunks + popcount(ballot & lanes below).  Only candidates are stored, so no
//           in-band marker for "not a candidate" exists that a real key could equal, and since slot order is
//           position order, "j' < j" is "slot' < slot".
//   pass 2  a candidate's rank is the number of stored (key, slot) pairs below its own: every lane walks the row's
//           keys with 16-byte LDS reads of one address (a broadcast: conflict free); chosen = rank < n_pred.  The
//           ranks of a row are a permutation of 0 .. n_cand - 1, so exactly n_pred positions are chosen.  Chosen
//           positions are compacted in ascending order into mlm_positions / mlm_labels by a second ballot +
//           popcount prefix; then the chunk's ids / token types / attention mask are written.
// Every output element is written exactly once with a plain vector store; there are no atomics.  The [B,S] outputs
// are int64, so the lane-per-position layout stores 8 bytes per lane, 512 contiguous bytes per wave instruction: that
// is fully coalesced with no alignment condition beyond the element's own, so one store path serves every S and
// every output view (a 16-byte form would need two positions per lane and a second, scalar path for odd S).
// length and a_len are clamped to [0, S] here, whatever the host validated: they are never used as extents.
#include "dtg/mlm_mask.h"
#include "dtg/common.h"

namespace dtg {
namespace {

constexpr int kMlmWaves = 4;  // rows per workgroup

__device__ __forceinline__ uint32_t mlm_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

// one round of hash32: a word enters through an odd multiplier
__device__ __forceinline__ uint32_t mlm_hash_word(uint32_t h, uint32_t w) {
  return mlm_fmix32(h ^ (w * 0x9E3779B1u)) * 5u + 0xE6546B64u;
}

// hash32(seed, epoch, index, j, k) from the row's folded prefix h3
__device__ __forceinline__ uint32_t mlm_hash_tail(uint32_t h3, uint32_t j, uint32_t k) {
  return mlm_fmix32(mlm_hash_word(mlm_hash_word(h3, j), k));
}

__device__ __forceinline__ bool mlm_special(const MlmMaskArgs& g, int id) {
  bool s = false;
#pragma unroll
  for (int t = 0; t < kMlmMaxSpecial; ++t) s |= (t < g.n_special) & (id == g.special[t]);
  return s;
}

__global__ void __launch_bounds__(kMlmWaves * kWave)
mlm_mask_kernel(const int* __restrict__ in, const int* __restrict__ a_len, const int* __restrict__ length,
                const long long* __restrict__ index, long long* __restrict__ ids, long long* __restrict__ tt,
                long long* __restrict__ am, long long* __restrict__ pos, long long* __restrict__ lab, int B, int S,
                int key_stride, MlmMaskArgs g) {
  extern __shared__ __attribute__((aligned(16))) uint32_t mlm_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kMlmWaves + wave;
  const bool live = row < B;  // the last workgroup may hold fewer rows; its other waves only keep the barrier
  uint32_t* const keys = mlm_lds + (size_t)wave * key_stride;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int* src = in;
  int len = 0, alen = 0, n_cand = 0, n_pred = 0;
  uint32_t h3 = 0;
  bool masking = false;

  if (live) {
    src = in + row * S;
    len = min(max(length[row], 0), S);
    alen = min(max(a_len[row], 0), S);
    h3 = mlm_hash_word(mlm_hash_word(mlm_hash_word(0x9E3779B9u, g.seed), g.epoch), (uint32_t)index[row]);
    masking = row < g.valid_rows;
    if (masking) {
      for (int c0 = 0; c0 < len; c0 += kWave) {  // pass 1: compacted candidate keys -> LDS
        const int j = c0 + lane;
        const bool cand = j < len && !mlm_special(g, src[j]);
        const unsigned long long bal = __ballot(cand);
        if (cand) keys[n_cand + __popcll(bal & below)] = mlm_hash_tail(h3, (uint32_t)j, 0u) >> g.key_shift;
        n_cand += __popcll(bal);
      }
      if (n_cand > 0) n_pred = min(min(g.P, n_cand), max(1, (n_cand * g.mask_per_mille + 500) / 1000));
    }
  }
  __syncthreads();
  if (!live) return;

  long long* const prow = pos + row * g.P;
  long long* const lrow = lab + row * g.P;
  const uint4* const keys4 = reinterpret_cast<const uint4*>(keys);
  int seen = 0, nsel = 0;  // candidates / chosen positions in earlier chunks
  for (int c0 = 0; c0 < S; c0 += kWave) {  // pass 2
    const int j = c0 + lane;
    const bool inb = j < S;
    const int id = inb ? src[j] : 0;
    const bool cand = masking && j < len && !mlm_special(g, id);
    const unsigned long long bal = __ballot(cand);
    const int m = seen + __popcll(bal & below);  // this candidate's slot in the key row
    seen += __popcll(bal);
    bool chosen = false;
    if (n_pred > 0 && bal != 0ull) {  // wave-uniform
      const uint32_t kc = cand ? keys[m] : 0u;
      int rank = 0;
      auto less = [&](uint32_t k, int n) { return (int)((k < kc) | ((k == kc) & (n < m))); };
      const int full = n_cand >> 2;
      for (int q = 0; q < full; ++q) {
        const uint4 k4 = keys4[q];
        const int n = q << 2;
        rank += less(k4.x, n) + less(k4.y, n + 1) + less(k4.z, n + 2) + less(k4.w, n + 3);
      }
      for (int n = full << 2; n < n_cand; ++n) rank += less(keys[n], n);
      chosen = cand && rank < n_pred;
    }
    const unsigned long long cb = __ballot(chosen);
    const int slot = nsel + __popcll(cb & below);
    nsel += __popcll(cb);
    long long out = id;
    if (chosen) {
      if (slot < g.P) {  // always: exactly n_pred <= P positions are chosen
        prow[slot] = j;
        lrow[slot] = id;
      }
      const uint32_t a = __umulhi(mlm_hash_tail(h3, (uint32_t)j, 1u), 10u);
      if (a < 8u) out = g.mask_id;
      else if (a == 9u) out = (long long)g.vocab_lo + (long long)__umulhi(mlm_hash_tail(h3, (uint32_t)j, 2u), g.vocab_range);
    }
    if (inb) {
      const long long o = row * S + j;
      ids[o] = out;
      tt[o] = (j >= alen && j < len) ? 1 : 0;
      am[o] = j < len ? 1 : 0;
    }
  }
  for (int p = n_pred + lane; p < g.P; p += kWave) {  // unused slots
    prow[p] = 0;
    lrow[p] = -1;
  }
}

}  // namespace

void mlm_mask(const int* input_ids, const int* a_len, const int* length, const long long* index, long long* ids,
              long long* token_types, long long* attention_mask, long long* positions, long long* labels, int B, int S,
              const MlmMaskArgs& args, hipStream_t st) {
  if (B <= 0) return;
  const int key_stride = (S + 3) & ~3;  // every wave's key row starts 16-byte aligned
  const int grid = (B + kMlmWaves - 1) / kMlmWaves;
  hipLaunchKernelGGL(mlm_mask_kernel, dim3(grid), dim3(kMlmWaves * kWave), (size_t)kMlmWaves * key_stride * 4, st,
                     input_ids, a_len, length, index, ids, token_types, attention_mask, positions, labels, B, S,
                     key_stride, args);
  DTG_LAUNCH_CHECK();
}

}  // namespace dtg
