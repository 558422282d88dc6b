// PyTorch bindings of the packed-row kernels (seqpack.hip); registered into dtg._C by ops.cc.
//
// Operands the 16-byte path cannot take -- a row width that is no multiple of 8, a base address that is not 16-byte
// aligned, a non-contiguous view -- are REFUSED here with a message that names the operand; there is no scalar
// path.  Every packed tensor's row count is its T_alloc: the kernels never write a row at or beyond it, whatever
// the device offsets say.  ``out`` lets a caller name the destination (a contiguous, aligned view into a larger
// buffer is fine).
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <vector>

#include "dtg/kernels.h"

namespace {

using at::Tensor;
using dtg::bf16_t;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }
bf16_t* bfp(const Tensor& t) { return reinterpret_cast<bf16_t*>(t.data_ptr()); }
const bf16_t* cbfp(const Tensor& t) { return reinterpret_cast<const bf16_t*>(t.data_ptr()); }
bool has(const c10::optional<Tensor>& t) { return t.has_value() && t->defined(); }
const long long* i64p(const Tensor& t) { return reinterpret_cast<const long long*>(t.data_ptr<int64_t>()); }
long long* i64w(const Tensor& t) { return reinterpret_cast<long long*>(t.data_ptr<int64_t>()); }

#define CHECK_ROWS_BF16(x)                                                                                      \
  TORCH_CHECK((x).is_cuda() && (x).scalar_type() == at::kBFloat16 && (x).dim() == 2, #x " must be a 2-D bf16 GPU tensor"); \
  TORCH_CHECK((x).is_contiguous(), #x " must be contiguous");                                                   \
  TORCH_CHECK((x).size(1) % 8 == 0, #x ": the row width must be a multiple of 8, got ", (x).size(1));         \
  TORCH_CHECK(((uintptr_t)(x).data_ptr() % 16) == 0, #x " must be 16-byte aligned")

void check_cu(const Tensor& cu, int64_t B, int64_t S, const Tensor& like) {
  TORCH_CHECK(B >= 0 && S >= 1 && B * S < (1LL << 31), "B >= 0, S >= 1 and B * S < 2^31 required");
  TORCH_CHECK(cu.is_cuda() && cu.scalar_type() == at::kInt && cu.dim() == 1 && cu.is_contiguous() &&
                  cu.size(0) == B + 1,
              "cu must be a contiguous int32 GPU tensor [B + 1]");
  TORCH_CHECK(cu.device() == like.device(), "all tensors must be on the same device");
}

Tensor seq_offsets(Tensor length, int64_t S) {
  TORCH_CHECK(length.is_cuda() && length.scalar_type() == at::kInt && length.dim() == 1 && length.is_contiguous(),
              "length must be a contiguous int32 GPU tensor [B]");
  const int64_t B = length.size(0);
  TORCH_CHECK(S >= 1 && B * S < (1LL << 31), "S >= 1 and B * S < 2^31 required");
  c10::DeviceGuard dg(length.device());
  auto cu = at::empty({B + 1}, length.options());
  dtg::seq_offsets(length.data_ptr<int>(), cu.data_ptr<int>(), (int)B, (int)S, cur_stream());
  return cu;
}

Tensor seq_pad(Tensor src, Tensor cu, int64_t B, int64_t S, c10::optional<Tensor> out) {
  CHECK_ROWS_BF16(src);
  check_cu(cu, B, S, src);
  const int64_t W = src.size(1);
  c10::DeviceGuard dg(src.device());
  Tensor dst = has(out) ? *out : at::empty({B * S, W}, src.options());
  CHECK_ROWS_BF16(dst);
  TORCH_CHECK(dst.size(0) == B * S && dst.size(1) == W && dst.device() == src.device(), "out must be [B * S, W]");
  dtg::seq_pad(cbfp(src), cu.data_ptr<int>(), bfp(dst), (int)B, (int)S, (long long)src.size(0), (int)W, cur_stream());
  return dst;
}

Tensor seq_unpad(Tensor src, Tensor cu, int64_t B, int64_t S, int64_t T_alloc, c10::optional<Tensor> out) {
  CHECK_ROWS_BF16(src);
  check_cu(cu, B, S, src);
  const int64_t W = src.size(1);
  TORCH_CHECK(src.size(0) == B * S, "src must be [B * S, W]");
  TORCH_CHECK(T_alloc >= 0 && T_alloc < (1LL << 31), "0 <= T_alloc < 2^31 required");
  c10::DeviceGuard dg(src.device());
  Tensor dst = has(out) ? *out : at::empty({T_alloc, W}, src.options());
  CHECK_ROWS_BF16(dst);
  TORCH_CHECK(dst.size(0) == T_alloc && dst.size(1) == W && dst.device() == src.device(), "out must be [T_alloc, W]");
  dtg::seq_unpad(cbfp(src), cu.data_ptr<int>(), bfp(dst), (int)B, (int)S, (long long)T_alloc, (int)W, cur_stream());
  return dst;
}

// ids / token types int64 [B, S] (token types optional); word [V, H], pos [>= S, H], type [*, H]; ids and token
// types are not range-checked on the device: the caller guarantees them, as for emb_fwd
Tensor emb_fwd_packed(Tensor ids, c10::optional<Tensor> tt, Tensor word, Tensor pos, Tensor type, Tensor cu,
                      int64_t T_alloc, c10::optional<Tensor> out) {
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kLong && ids.dim() == 2 && ids.is_contiguous(),
              "ids must be a contiguous int64 GPU tensor [B, S]");
  const int64_t B = ids.size(0), S = ids.size(1);
  CHECK_ROWS_BF16(word);
  CHECK_ROWS_BF16(pos);
  CHECK_ROWS_BF16(type);
  check_cu(cu, B, S, word);
  const int64_t H = word.size(1);
  TORCH_CHECK(pos.size(1) == H && type.size(1) == H && S <= pos.size(0), "embedding widths / position table");
  if (has(tt))
    TORCH_CHECK(tt->is_cuda() && tt->scalar_type() == at::kLong && tt->is_contiguous() && tt->dim() == 2 &&
                    tt->size(0) == B && tt->size(1) == S,
                "token types must be a contiguous int64 GPU tensor [B, S]");
  TORCH_CHECK(T_alloc >= 0 && T_alloc < (1LL << 31), "0 <= T_alloc < 2^31 required");
  c10::DeviceGuard dg(ids.device());
  Tensor dst = has(out) ? *out : at::empty({T_alloc, H}, word.options());
  CHECK_ROWS_BF16(dst);
  TORCH_CHECK(dst.size(0) == T_alloc && dst.size(1) == H && dst.device() == word.device(), "out must be [T_alloc, H]");
  dtg::emb_fwd_packed(i64p(ids), has(tt) ? i64p(*tt) : nullptr, cbfp(word), cbfp(pos), cbfp(type), cu.data_ptr<int>(),
                      bfp(dst), (int)B, (int)S, (long long)T_alloc, (int)H, cur_stream());
  return dst;
}

// -> (ids [T_alloc], token types [T_alloc] or an undefined tensor)
std::vector<Tensor> seq_gather_ids(Tensor ids, c10::optional<Tensor> tt, Tensor cu, int64_t T_alloc) {
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kLong && ids.dim() == 2 && ids.is_contiguous(),
              "ids must be a contiguous int64 GPU tensor [B, S]");
  const int64_t B = ids.size(0), S = ids.size(1);
  check_cu(cu, B, S, ids);
  if (has(tt))
    TORCH_CHECK(tt->is_cuda() && tt->scalar_type() == at::kLong && tt->is_contiguous() && tt->dim() == 2 &&
                    tt->size(0) == B && tt->size(1) == S,
                "token types must be a contiguous int64 GPU tensor [B, S]");
  TORCH_CHECK(T_alloc >= 0 && T_alloc < (1LL << 31), "0 <= T_alloc < 2^31 required");
  c10::DeviceGuard dg(ids.device());
  Tensor io = at::empty({T_alloc}, ids.options());
  Tensor to = has(tt) ? at::empty({T_alloc}, ids.options()) : Tensor();
  dtg::seq_gather_ids(i64p(ids), has(tt) ? i64p(*tt) : nullptr, cu.data_ptr<int>(), i64w(io),
                      has(tt) ? i64w(to) : nullptr, (int)B, (int)S, (long long)T_alloc, cur_stream());
  return {io, to};
}

// gP[p] += sum over b with len[b] > p of ds[cu[b] + p]: adds into gP, like emb_pos_bwd
void emb_pos_bwd_packed(Tensor ds, Tensor cu, Tensor gP, int64_t B, int64_t S) {
  CHECK_ROWS_BF16(ds);
  CHECK_ROWS_BF16(gP);
  check_cu(cu, B, S, ds);
  TORCH_CHECK(gP.size(0) >= S && gP.size(1) == ds.size(1) && gP.device() == ds.device(), "shape mismatch");
  c10::DeviceGuard dg(ds.device());
  dtg::emb_pos_bwd_packed(cbfp(ds), cu.data_ptr<int>(), bfp(gP), (int)B, (int)S, (long long)ds.size(0),
                          (int)ds.size(1), cur_stream());
}

// ---- fused attention on packed rows (attention_packed.hip) ----------------------------------------------------
// qkv [T_alloc, 3 * nh * 64] ([Q | K | V], head h at columns h * 64 of each); T_alloc is qkv.size(0)
// long_: the entry points for 128 < S <= 512 (the dKV + dQ backward pair)
void check_attn_packed(const Tensor& qkv, const Tensor& cu, int64_t B, int64_t S, int64_t nh, double p,
                       bool long_ = false) {
  CHECK_ROWS_BF16(qkv);
  TORCH_CHECK(nh >= 1 && qkv.size(1) == 3 * nh * 64, "qkv: the row width must be 3 * nh * 64 = ", 3 * nh * 64,
              ", got ", qkv.size(1));
  if (long_) {
    TORCH_CHECK(dtg::attn_packed_long_supported((int)S, 64),
                "S: long packed attention takes a multiple of 64 with 128 < S <= 512, got ", S);
  } else {
    TORCH_CHECK(dtg::attn_packed_supported((int)S, 64), "S: packed attention takes S = 64 or S = 128, got ", S);
  }
  check_cu(cu, B, S, qkv);
  TORCH_CHECK(qkv.size(0) % 8 == 0 && qkv.size(0) < (1LL << 31),
              "qkv: T_alloc (the row count) must be a multiple of 8 below 2^31, got ", qkv.size(0));
  TORCH_CHECK(p >= 0 && p < 1, "p: dropout probability in [0, 1)");
}

// -> [ctx [T_alloc, H] (zeros on the rows cu[B] .. T_alloc - 1), lse fp32 [nh, T_alloc]]
std::vector<Tensor> attn_packed_fwd_any(bool long_, Tensor qkv, Tensor cu, int64_t B, int64_t S, int64_t nh, double p,
                                        int64_t seed, c10::optional<Tensor> out) {
  check_attn_packed(qkv, cu, B, S, nh, p, long_);
  const int64_t T_alloc = qkv.size(0), H = nh * 64;
  c10::DeviceGuard dg(qkv.device());
  Tensor ctx = has(out) ? *out : at::empty({T_alloc, H}, qkv.options());
  CHECK_ROWS_BF16(ctx);
  TORCH_CHECK(ctx.size(0) == T_alloc && ctx.size(1) == H && ctx.device() == qkv.device(), "out must be [T_alloc, H]");
  Tensor lse = at::empty({nh, T_alloc}, qkv.options().dtype(at::kFloat));
  (long_ ? dtg::attn_packed_long_fwd : dtg::attn_packed_fwd)(cbfp(qkv), cu.data_ptr<int>(), bfp(ctx),
                                                             lse.data_ptr<float>(), (int)B, (int)S, (int)nh,
                                                             (long long)T_alloc, (float)p, (uint32_t)seed,
                                                             cur_stream());
  return {ctx, lse};
}
std::vector<Tensor> attn_packed_fwd(Tensor qkv, Tensor cu, int64_t B, int64_t S, int64_t nh, double p, int64_t seed,
                                    c10::optional<Tensor> out) {
  return attn_packed_fwd_any(false, qkv, cu, B, S, nh, p, seed, out);
}
std::vector<Tensor> attn_packed_long_fwd(Tensor qkv, Tensor cu, int64_t B, int64_t S, int64_t nh, double p,
                                         int64_t seed, c10::optional<Tensor> out) {
  return attn_packed_fwd_any(true, qkv, cu, B, S, nh, p, seed, out);
}

// dbias (optional, fp32 [3 * nh * 64]): the QKV bias gradient is ADDED into it by the kernel's epilogue.
// -> dqkv [T_alloc, 3H] (zeros on the rows cu[B] .. T_alloc - 1)
Tensor attn_packed_bwd_any(bool long_, Tensor qkv, Tensor ctx, Tensor dout, Tensor lse, Tensor cu, int64_t B, int64_t S,
                           int64_t nh, double p, int64_t seed, c10::optional<Tensor> dbias,
                           c10::optional<Tensor> out) {
  check_attn_packed(qkv, cu, B, S, nh, p, long_);
  const int64_t T_alloc = qkv.size(0), H = nh * 64;
  CHECK_ROWS_BF16(ctx);
  CHECK_ROWS_BF16(dout);
  TORCH_CHECK(ctx.size(0) == T_alloc && ctx.size(1) == H && ctx.device() == qkv.device(), "ctx must be [T_alloc, H]");
  TORCH_CHECK(dout.size(0) == T_alloc && dout.size(1) == H && dout.device() == qkv.device(),
              "dout must be [T_alloc, H]");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat && lse.is_contiguous() && lse.numel() == nh * T_alloc &&
                  lse.device() == qkv.device(),
              "lse must be a contiguous fp32 GPU tensor [nh, T_alloc]");
  if (has(dbias))
    TORCH_CHECK(dbias->is_cuda() && dbias->scalar_type() == at::kFloat && dbias->is_contiguous() &&
                    dbias->numel() == 3 * H && dbias->device() == qkv.device(),
                "dbias must be a contiguous fp32 GPU tensor [3 * nh * 64]");
  c10::DeviceGuard dg(qkv.device());
  Tensor dqkv = has(out) ? *out : at::empty({T_alloc, 3 * H}, qkv.options());
  CHECK_ROWS_BF16(dqkv);
  TORCH_CHECK(dqkv.size(0) == T_alloc && dqkv.size(1) == 3 * H && dqkv.device() == qkv.device(),
              "out must be [T_alloc, 3 * nh * 64]");
  (long_ ? dtg::attn_packed_long_bwd : dtg::attn_packed_bwd)(
      cbfp(qkv), cbfp(ctx), cbfp(dout), lse.data_ptr<float>(), cu.data_ptr<int>(), bfp(dqkv), (int)B, (int)S, (int)nh,
      (long long)T_alloc, (float)p, (uint32_t)seed, has(dbias) ? dbias->data_ptr<float>() : nullptr, cur_stream());
  return dqkv;
}
Tensor attn_packed_bwd(Tensor qkv, Tensor ctx, Tensor dout, Tensor lse, Tensor cu, int64_t B, int64_t S, int64_t nh,
                       double p, int64_t seed, c10::optional<Tensor> dbias, c10::optional<Tensor> out) {
  return attn_packed_bwd_any(false, qkv, ctx, dout, lse, cu, B, S, nh, p, seed, dbias, out);
}
// the dKV launch, then the dQ launch, on the current stream
Tensor attn_packed_long_bwd(Tensor qkv, Tensor ctx, Tensor dout, Tensor lse, Tensor cu, int64_t B, int64_t S,
                            int64_t nh, double p, int64_t seed, c10::optional<Tensor> dbias,
                            c10::optional<Tensor> out) {
  return attn_packed_bwd_any(true, qkv, ctx, dout, lse, cu, B, S, nh, p, seed, dbias, out);
}

}  // namespace

void register_seqpack_ops(pybind11::module_& m) {
  namespace py = pybind11;
  m.def("seq_offsets", &seq_offsets, py::arg("length"), py::arg("S"));
  m.def("seq_pad", &seq_pad, py::arg("src"), py::arg("cu"), py::arg("B"), py::arg("S"), py::arg("out") = py::none());
  m.def("seq_unpad", &seq_unpad, py::arg("src"), py::arg("cu"), py::arg("B"), py::arg("S"), py::arg("T_alloc"),
        py::arg("out") = py::none());
  m.def("emb_fwd_packed", &emb_fwd_packed, py::arg("ids"), py::arg("token_types"), py::arg("word"), py::arg("pos"),
        py::arg("type"), py::arg("cu"), py::arg("T_alloc"), py::arg("out") = py::none());
  m.def("seq_gather_ids", &seq_gather_ids, py::arg("ids"), py::arg("token_types"), py::arg("cu"), py::arg("T_alloc"));
  m.def("emb_pos_bwd_packed", &emb_pos_bwd_packed);
  m.def("attn_packed_supported", [](int64_t S, int64_t dh) { return dtg::attn_packed_supported((int)S, (int)dh) != 0; });
  m.def("attn_packed_fwd", &attn_packed_fwd, py::arg("qkv"), py::arg("cu"), py::arg("B"), py::arg("S"), py::arg("nh"),
        py::arg("p"), py::arg("seed"), py::arg("out") = py::none());
  m.def("attn_packed_bwd", &attn_packed_bwd, py::arg("qkv"), py::arg("ctx"), py::arg("dout"), py::arg("lse"),
        py::arg("cu"), py::arg("B"), py::arg("S"), py::arg("nh"), py::arg("p"), py::arg("seed"),
        py::arg("dbias") = py::none(), py::arg("out") = py::none());
  m.def("attn_packed_long_supported",
        [](int64_t S, int64_t dh) { return dtg::attn_packed_long_supported((int)S, (int)dh) != 0; });
  m.def("attn_packed_long_fwd", &attn_packed_long_fwd, py::arg("qkv"), py::arg("cu"), py::arg("B"), py::arg("S"),
        py::arg("nh"), py::arg("p"), py::arg("seed"), py::arg("out") = py::none());
  m.def("attn_packed_long_bwd", &attn_packed_long_bwd, py::arg("qkv"), py::arg("ctx"), py::arg("dout"), py::arg("lse"),
        py::arg("cu"), py::arg("B"), py::arg("S"), py::arg("nh"), py::arg("p"), py::arg("seed"),
        py::arg("dbias") = py::none(), py::arg("out") = py::none());
}
