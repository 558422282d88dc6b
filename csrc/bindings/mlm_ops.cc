// PyTorch binding of the BERT dynamic-masking kernel (mlm_mask.hip); registered into dtg._C by ops.cc.
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <vector>

#include "dtg/mlm_mask.h"

namespace {

using at::Tensor;

// input_ids i32 [B,S], a_len / length i32 [B], index i64 [B]; ids / token_types / attention_mask i64 [B,S] and
// positions / labels i64 [B,P] are destinations (contiguous; they may be views into larger buffers).
void mlm_mask(Tensor input_ids, Tensor a_len, Tensor length, Tensor index, Tensor ids, Tensor token_types,
              Tensor attention_mask, Tensor positions, Tensor labels, int64_t seed, int64_t epoch,
              int64_t mask_per_mille, int64_t mask_id, int64_t vocab_lo, int64_t vocab_hi,
              std::vector<int64_t> special_ids, int64_t valid_rows, int64_t key_bits) {
  TORCH_CHECK(input_ids.is_cuda() && input_ids.scalar_type() == at::kInt && input_ids.dim() == 2 &&
                  input_ids.is_contiguous(),
              "input_ids must be a contiguous int32 GPU tensor [B, S]");
  const int64_t B = input_ids.size(0), S = input_ids.size(1);
  TORCH_CHECK(S >= 1 && S <= dtg::kMlmMaxSeq, "1 <= S <= ", dtg::kMlmMaxSeq, " required, got ", S);
  TORCH_CHECK(B < (1LL << 31), "too many rows");
  for (const Tensor* t : {&a_len, &length})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->dim() == 1 && t->size(0) == B &&
                    t->is_contiguous(),
                "a_len and length must be contiguous int32 GPU tensors [B]");
  TORCH_CHECK(index.is_cuda() && index.scalar_type() == at::kLong && index.dim() == 1 && index.size(0) == B &&
                  index.is_contiguous(),
              "index must be a contiguous int64 GPU tensor [B]");
  TORCH_CHECK(positions.dim() == 2 && positions.size(1) >= 1 && positions.size(1) < (1LL << 20),
              "positions must be [B, P] with 1 <= P < 2^20");
  const int64_t P = positions.size(1);
  for (const Tensor* t : {&ids, &token_types, &attention_mask})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->dim() == 2 && t->size(0) == B &&
                    t->size(1) == S && t->is_contiguous(),
                "ids, token_types and attention_mask must be contiguous int64 GPU tensors [B, S]");
  for (const Tensor* t : {&positions, &labels})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->dim() == 2 && t->size(0) == B &&
                    t->size(1) == P && t->is_contiguous(),
                "positions and labels must be contiguous int64 GPU tensors [B, P]");
  for (const Tensor* t : {&a_len, &length, &index, &ids, &token_types, &attention_mask, &positions, &labels})
    TORCH_CHECK(t->device() == input_ids.device(), "all tensors must be on the same device");
  TORCH_CHECK(mask_per_mille >= 0 && mask_per_mille <= 1000, "0 <= mask_per_mille <= 1000 required");
  TORCH_CHECK(key_bits >= 1 && key_bits <= 32, "1 <= key_bits <= 32 required");
  TORCH_CHECK(vocab_lo >= 0 && vocab_lo < vocab_hi && vocab_hi < (1LL << 31), "0 <= vocab_lo < vocab_hi < 2^31 required");
  TORCH_CHECK(mask_id >= 0 && mask_id < (1LL << 31), "0 <= mask_id < 2^31 required");
  TORCH_CHECK((int64_t)special_ids.size() <= dtg::kMlmMaxSpecial, "at most ", dtg::kMlmMaxSpecial, " special ids");
  TORCH_CHECK(valid_rows >= 0 && valid_rows <= B, "0 <= valid_rows <= B required");
  dtg::MlmMaskArgs g;
  g.seed = (uint32_t)((uint64_t)seed & 0xFFFFFFFFull);
  g.epoch = (uint32_t)((uint64_t)epoch & 0xFFFFFFFFull);
  g.P = (int)P;
  g.mask_per_mille = (int)mask_per_mille;
  g.mask_id = (int)mask_id;
  g.vocab_lo = (int)vocab_lo;
  g.vocab_range = (uint32_t)(vocab_hi - vocab_lo);
  g.n_special = (int)special_ids.size();
  for (int t = 0; t < dtg::kMlmMaxSpecial; ++t) {
    g.special[t] = 0;
    if (t < g.n_special) {
      TORCH_CHECK(special_ids[t] >= -(1LL << 31) && special_ids[t] < (1LL << 31), "special ids must fit int32");
      g.special[t] = (int)special_ids[t];
    }
  }
  g.valid_rows = (int)valid_rows;
  g.key_shift = (int)(32 - key_bits);
  c10::DeviceGuard dg(input_ids.device());
  dtg::mlm_mask(input_ids.data_ptr<int>(), a_len.data_ptr<int>(), length.data_ptr<int>(),
                reinterpret_cast<const long long*>(index.data_ptr<int64_t>()),
                reinterpret_cast<long long*>(ids.data_ptr<int64_t>()),
                reinterpret_cast<long long*>(token_types.data_ptr<int64_t>()),
                reinterpret_cast<long long*>(attention_mask.data_ptr<int64_t>()),
                reinterpret_cast<long long*>(positions.data_ptr<int64_t>()),
                reinterpret_cast<long long*>(labels.data_ptr<int64_t>()), (int)B, (int)S, g,
                c10::hip::getCurrentHIPStream().stream());
}

}  // namespace

void register_mlm_ops(pybind11::module_& m) {
  m.def("mlm_mask", &mlm_mask, pybind11::arg("input_ids"), pybind11::arg("a_len"), pybind11::arg("length"),
        pybind11::arg("index"), pybind11::arg("ids"), pybind11::arg("token_types"), pybind11::arg("attention_mask"),
        pybind11::arg("positions"), pybind11::arg("labels"), pybind11::arg("seed"), pybind11::arg("epoch"),
        pybind11::arg("mask_per_mille"), pybind11::arg("mask_id"), pybind11::arg("vocab_lo"),
        pybind11::arg("vocab_hi"), pybind11::arg("special_ids"), pybind11::arg("valid_rows"),
        pybind11::arg("key_bits") = 32);
}
