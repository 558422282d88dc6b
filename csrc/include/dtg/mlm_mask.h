// Launcher of the BERT dynamic-masking kernel (csrc/kernels/mlm_mask.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dtg {

constexpr int kMlmMaxSeq = 2048;     // S <= this: a wave's key row is at most 8 KiB of LDS, a workgroup's 32 KiB
constexpr int kMlmMaxSpecial = 4;    // special ids that are never masked

struct MlmMaskArgs {
  uint32_t seed, epoch;              // the low 32 bits, as data/sampler.py::hash32 takes its words
  int P, mask_per_mille, mask_id, vocab_lo;
  uint32_t vocab_range;              // vocab_hi - vocab_lo, >= 1
  int special[kMlmMaxSpecial], n_special;
  int valid_rows;                    // rows >= this are the evaluation pass's padding rows: copied unmasked
  int key_shift;                     // 32 - key_bits, in [0, 31]
};

// input_ids i32 [B,S], a_len / length i32 [B], index i64 [B]  ->  ids, token_type_ids, attention_mask i64 [B,S],
// mlm_positions, mlm_labels i64 [B,P]; one launch, every output element written exactly once.
void mlm_mask(const int* input_ids, const int* a_len, const int* length, const long long* index, long long* ids,
              long long* token_types, long long* attention_mask, long long* positions, long long* labels, int B, int S,
              const MlmMaskArgs& args, hipStream_t st);

}  // namespace dtg
