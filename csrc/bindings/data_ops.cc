// PyTorch binding of the input-pipeline kernel (augment.hip); registered into dtg._C by ops.cc.
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include "dtg/augment.h"

namespace {

using at::Tensor;

// raw u8 [N,H,W,3], params i32 [N,5], out bf16 [N,S,S,3] (the NHWC view of a channels_last [N,3,S,S] tensor, or a
// contiguous view into a larger buffer), scale / shift fp32 [3]; everything on one GPU.  grid: 0 = heuristic.
void crop_resize_norm(Tensor raw, Tensor params, Tensor out, Tensor scale, Tensor shift, int64_t grid) {
  TORCH_CHECK(raw.is_cuda() && raw.scalar_type() == at::kByte && raw.dim() == 4 && raw.is_contiguous() &&
                  raw.size(3) == 3,
              "raw must be a contiguous uint8 GPU tensor [N, H, W, 3]");
  const int64_t N = raw.size(0), H = raw.size(1), W = raw.size(2);
  TORCH_CHECK(H >= 1 && W >= 1 && H <= dtg::kAugMaxSide && W <= dtg::kAugMaxSide, "raw: 1 <= H, W <= ",
              dtg::kAugMaxSide, " required (32-bit coordinate arithmetic)");
  TORCH_CHECK(params.is_cuda() && params.scalar_type() == at::kInt && params.dim() == 2 && params.is_contiguous() &&
                  params.size(0) == N && params.size(1) == 5,
              "params must be a contiguous int32 GPU tensor [N, 5]");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 && out.dim() == 4 && out.is_contiguous() &&
                  out.size(0) == N && out.size(1) == out.size(2) && out.size(3) == 3,
              "out must be a contiguous bf16 GPU tensor [N, S, S, 3]");
  const int64_t S = out.size(1);
  TORCH_CHECK(S >= 1 && S <= dtg::kAugMaxSide, "1 <= S <= ", dtg::kAugMaxSide, " required");
  TORCH_CHECK(N < (1LL << 31) / 5, "too many images");
  for (const Tensor* t : {&scale, &shift})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == 3,
                "scale and shift must be fp32 GPU tensors of 3 elements");
  TORCH_CHECK(params.device() == raw.device() && out.device() == raw.device() && scale.device() == raw.device() &&
                  shift.device() == raw.device(),
              "all tensors must be on the same device");
  TORCH_CHECK(grid >= 0 && grid < (1LL << 31), "bad grid");
  c10::DeviceGuard dg(raw.device());
  dtg::crop_resize_norm(raw.data_ptr<uint8_t>(), params.data_ptr<int>(),
                        reinterpret_cast<unsigned short*>(out.data_ptr()), scale.data_ptr<float>(),
                        shift.data_ptr<float>(), (int)N, (int)H, (int)W, (int)S, (int)grid,
                        c10::hip::getCurrentHIPStream().stream());
}

}  // namespace

void register_data_ops(pybind11::module_& m) {
  m.def("crop_resize_norm", &crop_resize_norm, pybind11::arg("raw"), pybind11::arg("params"), pybind11::arg("out"),
        pybind11::arg("scale"), pybind11::arg("shift"), pybind11::arg("grid") = 0);
}
