// PyTorch bindings of the evaluation-metric kernels (eval_metrics.hip); registered into dtg._C by ops.cc.
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <tuple>
#include <vector>

#include "dtg/kernels.h"

namespace {

using at::Tensor;

// logits bf16 / fp32 [B, V] contiguous, labels int64 [B] -> (loss fp32 [B], rank int32 [B]); the outputs are
// allocated here unless the caller hands in both (contiguous [B] on the logits' device, e.g. views of a larger buffer)
std::tuple<Tensor, Tensor> xent_rank(Tensor logits, Tensor labels, c10::optional<Tensor> loss_out,
                                     c10::optional<Tensor> rank_out) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous(),
              "logits must be a contiguous GPU tensor [B, V]");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits bf16/fp32");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V < (1LL << 31) && B < (1LL << 31), "1 <= V < 2^31 and B < 2^31 required");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong && labels.dim() == 1 && labels.is_contiguous() &&
                  labels.size(0) == B,
              "labels must be a contiguous int64 GPU tensor [B]");
  TORCH_CHECK(labels.device() == logits.device(), "logits and labels must be on the same device");
  c10::DeviceGuard dg(logits.device());
  const bool given = loss_out.has_value() && loss_out->defined();
  TORCH_CHECK(given == (rank_out.has_value() && rank_out->defined()), "give both outputs or neither");
  Tensor loss = given ? *loss_out : at::empty({B}, logits.options().dtype(at::kFloat));
  Tensor rank = given ? *rank_out : at::empty({B}, logits.options().dtype(at::kInt));
  if (given) {
    TORCH_CHECK(loss.scalar_type() == at::kFloat && rank.scalar_type() == at::kInt && loss.dim() == 1 &&
                    rank.dim() == 1 && loss.size(0) == B && rank.size(0) == B && loss.is_contiguous() &&
                    rank.is_contiguous() && loss.device() == logits.device() && rank.device() == logits.device(),
                "outputs must be contiguous fp32 [B] and int32 [B] on the logits' device");
  }
  dtg::xent_rank(logits.data_ptr(), logits.scalar_type() == at::kBFloat16,
                 reinterpret_cast<const long long*>(labels.data_ptr<int64_t>()), B, (int)V, loss.data_ptr<float>(),
                 rank.data_ptr<int>(), c10::hip::getCurrentHIPStream().stream());
  return {loss, rank};
}

// acc fp64 [8] on the device of loss / rank (fp32 / int32 [B]); 1 <= len(ks) <= 4
void metric_accumulate(Tensor acc, Tensor loss, Tensor rank, std::vector<int64_t> ks, int64_t V) {
  TORCH_CHECK(loss.is_cuda() && loss.scalar_type() == at::kFloat && loss.dim() == 1 && loss.is_contiguous(),
              "loss must be a contiguous fp32 GPU tensor [B]");
  const int64_t B = loss.size(0);
  TORCH_CHECK(rank.is_cuda() && rank.scalar_type() == at::kInt && rank.dim() == 1 && rank.is_contiguous() &&
                  rank.size(0) == B,
              "rank must be a contiguous int32 GPU tensor [B]");
  TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == at::kDouble && acc.dim() == 1 && acc.is_contiguous() &&
                  acc.size(0) == 8,
              "acc must be a contiguous fp64 GPU tensor [8]");
  TORCH_CHECK(rank.device() == loss.device() && acc.device() == loss.device(),
              "acc, loss and rank must be on the same device");
  TORCH_CHECK(ks.size() >= 1 && ks.size() <= 4, "1 <= len(ks) <= 4 required");
  TORCH_CHECK(V >= 1 && V < (1LL << 31) && B < (1LL << 31), "1 <= V < 2^31 and B < 2^31 required");
  int k[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < ks.size(); ++i) {
    TORCH_CHECK(ks[i] >= 1 && ks[i] < (1LL << 31), "every k must be >= 1");
    k[i] = (int)ks[i];
  }
  c10::DeviceGuard dg(loss.device());
  dtg::metric_accumulate(loss.data_ptr<float>(), rank.data_ptr<int>(), B, (int)V, k, (int)ks.size(),
                         acc.data_ptr<double>(), c10::hip::getCurrentHIPStream().stream());
}

}  // namespace

void register_eval_ops(pybind11::module_& m) {
  m.def("xent_rank", &xent_rank, pybind11::arg("logits"), pybind11::arg("labels"),
        pybind11::arg("loss") = pybind11::none(), pybind11::arg("rank") = pybind11::none());
  m.def("metric_accumulate", &metric_accumulate, pybind11::arg("acc"), pybind11::arg("loss"), pybind11::arg("rank"),
        pybind11::arg("ks"), pybind11::arg("V"));
}
