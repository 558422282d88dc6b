// PyTorch bindings for dtg's HIP kernels (module dtg._C).
// Each wrapper validates shapes/dtypes/devices on the host (a kernel never sees an operand whose
// shape disagrees with its grid), allocates outputs with the caching allocator and launches on the
// current HIP stream, so everything composes with torch streams and hipGraph capture.
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include "dtg/kernels.h"

namespace {

using at::Tensor;
using dtg::bf16_t;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// fp32 zeros on like's device, filled by a dtg kernel on the current stream
at::Tensor zeros_f32(long long n, const at::Tensor& like) {
  c10::DeviceGuard dg(like.device());  // the fill runs on like's device's current stream
  at::Tensor t = at::empty({n}, like.options().dtype(at::kFloat));
  dtg::fill_zero(t.data_ptr(), n * 4, cur_stream());
  return t;
}

#define CHECK_CUDA(x) TORCH_CHECK((x).is_cuda(), #x " must be a GPU tensor")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")
#define CHECK_DT(x, dt) TORCH_CHECK((x).scalar_type() == (dt), #x " must be " #dt)
#define CHECK_IN(x) \
  CHECK_CUDA(x);    \
  CHECK_CONTIG(x)

bf16_t* bfp(const Tensor& t) { return reinterpret_cast<bf16_t*>(t.data_ptr()); }
const bf16_t* cbfp(const Tensor& t) { return reinterpret_cast<const bf16_t*>(t.data_ptr()); }
template <class T>
T* opt_ptr(const c10::optional<Tensor>& t) {
  return (t.has_value() && t->defined()) ? reinterpret_cast<T*>(t->data_ptr()) : nullptr;
}

void check_flat(const Tensor& w, const Tensor& g, const c10::optional<Tensor>& mirror) {
  CHECK_IN(w);
  CHECK_IN(g);
  CHECK_DT(w, at::kFloat);
  TORCH_CHECK(g.scalar_type() == at::kFloat || g.scalar_type() == at::kBFloat16, "grad must be fp32 or bf16");
  TORCH_CHECK(g.numel() == w.numel(), "grad/param size mismatch");
  if (mirror.has_value() && mirror->defined()) {
    CHECK_IN(*mirror);
    CHECK_DT(*mirror, at::kBFloat16);
    TORCH_CHECK(mirror->numel() == w.numel(), "mirror size mismatch");
  }
}

void check_state(const Tensor& s, const Tensor& w) {
  CHECK_IN(s);
  CHECK_DT(s, at::kFloat);
  TORCH_CHECK(s.numel() == w.numel(), "optimizer state size mismatch");
}

void check_hyper(const Tensor& h) {
  CHECK_IN(h);
  CHECK_DT(h, at::kFloat);
  TORCH_CHECK(h.numel() >= 2, "hyper must hold {lr, step}");
}

// an optional device scalar (the clip factor) on w's device; null when absent
const float* clip_ptr(const c10::optional<Tensor>& clip, const Tensor& w) {
  if (!clip.has_value() || !clip->defined()) return nullptr;
  CHECK_IN(*clip);
  CHECK_DT(*clip, at::kFloat);
  TORCH_CHECK(clip->numel() >= 1 && clip->device() == w.device(), "clip must be a device scalar on the master's device");
  return clip->data_ptr<float>();
}

// ---- optimizers ----------------------------------------------------------------------------
void sgd_apply(Tensor w, c10::optional<Tensor> mirror, Tensor g, Tensor hyper, double wd, double gscale,
               bool zero_grad, c10::optional<Tensor> clip) {
  check_flat(w, g, mirror);
  check_hyper(hyper);
  c10::DeviceGuard dg(w.device());
  dtg::sgd_apply(w.data_ptr<float>(), opt_ptr<bf16_t>(mirror), g.data_ptr(), g.scalar_type() == at::kBFloat16,
                 w.numel(), hyper.data_ptr<float>(), (float)wd, (float)gscale, zero_grad, cur_stream(),
                 clip_ptr(clip, w));
}

void momentum_apply(Tensor w, c10::optional<Tensor> mirror, Tensor g, Tensor mom, Tensor hyper, double mu, double wd,
                    bool nesterov, double gscale, bool zero_grad, c10::optional<Tensor> clip) {
  check_flat(w, g, mirror);
  check_state(mom, w);
  check_hyper(hyper);
  c10::DeviceGuard dg(w.device());
  dtg::momentum_apply(w.data_ptr<float>(), opt_ptr<bf16_t>(mirror), g.data_ptr(), g.scalar_type() == at::kBFloat16,
                      mom.data_ptr<float>(), w.numel(), hyper.data_ptr<float>(), (float)mu, (float)wd, nesterov,
                      (float)gscale, zero_grad, cur_stream(), clip_ptr(clip, w));
}

void adagrad_apply(Tensor w, c10::optional<Tensor> mirror, Tensor g, Tensor acc, Tensor hyper, double eps,
                   double gscale, bool zero_grad, c10::optional<Tensor> clip) {
  check_flat(w, g, mirror);
  check_state(acc, w);
  check_hyper(hyper);
  c10::DeviceGuard dg(w.device());
  dtg::adagrad_apply(w.data_ptr<float>(), opt_ptr<bf16_t>(mirror), g.data_ptr(), g.scalar_type() == at::kBFloat16,
                     acc.data_ptr<float>(), w.numel(), hyper.data_ptr<float>(), (float)eps, (float)gscale, zero_grad,
                     cur_stream(), clip_ptr(clip, w));
}

void adam_apply(Tensor w, c10::optional<Tensor> mirror, Tensor g, Tensor m, Tensor v, Tensor hyper, double b1,
                double b2, double eps, double wd, double gscale, bool zero_grad, c10::optional<Tensor> clip) {
  check_flat(w, g, mirror);
  check_state(m, w);
  check_state(v, w);
  check_hyper(hyper);
  c10::DeviceGuard dg(w.device());
  dtg::adam_apply(w.data_ptr<float>(), opt_ptr<bf16_t>(mirror), g.data_ptr(), g.scalar_type() == at::kBFloat16,
                  m.data_ptr<float>(), v.data_ptr<float>(), w.numel(), hyper.data_ptr<float>(), (float)b1, (float)b2,
                  (float)eps, (float)wd, (float)gscale, zero_grad, cur_stream(), clip_ptr(clip, w));
}

void axpby(Tensor acc, Tensor g, double alpha, double beta) {
  CHECK_IN(acc);
  CHECK_IN(g);
  CHECK_DT(acc, at::kFloat);
  TORCH_CHECK(g.scalar_type() == at::kFloat || g.scalar_type() == at::kBFloat16, "g must be fp32 or bf16");
  TORCH_CHECK(acc.numel() == g.numel(), "size mismatch");
  c10::DeviceGuard dg(acc.device());
  dtg::axpby(acc.data_ptr<float>(), g.data_ptr(), g.scalar_type() == at::kBFloat16, acc.numel(), (float)alpha,
             (float)beta, cur_stream());
}

// ---- k-way sum-apply (sync PS) ----------------------------------------------------------------
// The kernels move 8 elements per lane with 16-byte accesses: a bf16 buffer must be 16-byte aligned, an fp32
// buffer 32-byte aligned (one lane iteration's footprint).  Everything is validated here, before any launch.
void check_align(const Tensor& t, const char* what) {
  const uintptr_t a = t.scalar_type() == at::kFloat ? 32 : 16;
  TORCH_CHECK(((uintptr_t)t.data_ptr() % a) == 0, what, " must be ", (int)a, "-byte aligned");
}

// validates the sources against the destination `w` (fp32, n elements); returns (pointers, k, bf16?)
std::tuple<dtg::GradSrcs, int, int> check_srcs(const std::vector<Tensor>& srcs, const Tensor& w) {
  TORCH_CHECK(!srcs.empty() && srcs.size() <= 8, "1..8 gradient sources, got ", srcs.size());
  const auto dt = srcs[0].scalar_type();
  TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16, "sources must be fp32 or bf16");
  dtg::GradSrcs gs;
  for (size_t j = 0; j < srcs.size(); ++j) {
    const Tensor& s = srcs[j];
    CHECK_IN(s);
    TORCH_CHECK(s.scalar_type() == dt, "all sources must have one dtype");
    TORCH_CHECK(s.numel() == w.numel(), "source ", j, " size mismatch: ", s.numel(), " vs ", w.numel());
    TORCH_CHECK(s.device() == w.device(), "source ", j, " is on another device");
    check_align(s, "source");
    gs.p[j] = s.data_ptr();
  }
  return {gs, (int)srcs.size(), dt == at::kBFloat16 ? 1 : 0};
}

void check_f32_like(const Tensor& t, const Tensor& w, const char* what) {
  CHECK_IN(t);
  TORCH_CHECK(t.scalar_type() == at::kFloat, what, " must be fp32");
  TORCH_CHECK(t.numel() == w.numel(), what, " size mismatch");
  TORCH_CHECK(t.device() == w.device(), what, " is on another device");
  check_align(t, what);
}

struct SumArgs {
  dtg::GradSrcs src;
  int k, bf16;
  bf16_t* mirror;
  const float* acc;
};

SumArgs check_sum(const Tensor& w, const c10::optional<Tensor>& mirror, const std::vector<Tensor>& srcs,
                  const Tensor& hyper, const c10::optional<Tensor>& acc, std::initializer_list<const Tensor*> slots) {
  CHECK_IN(w);
  CHECK_DT(w, at::kFloat);
  check_align(w, "master");
  SumArgs a;
  std::tie(a.src, a.k, a.bf16) = check_srcs(srcs, w);
  check_hyper(hyper);
  TORCH_CHECK(hyper.device() == w.device(), "hyper is on another device");
  a.mirror = nullptr;
  if (mirror.has_value() && mirror->defined()) {
    CHECK_IN(*mirror);
    CHECK_DT(*mirror, at::kBFloat16);
    TORCH_CHECK(mirror->numel() == w.numel(), "mirror size mismatch");
    TORCH_CHECK(mirror->device() == w.device(), "mirror is on another device");
    check_align(*mirror, "mirror");
    a.mirror = bfp(*mirror);
  }
  a.acc = nullptr;
  if (acc.has_value() && acc->defined()) {
    check_f32_like(*acc, w, "acc");
    a.acc = acc->data_ptr<float>();
  }
  for (const Tensor* s : slots) check_f32_like(*s, w, "optimizer state");
  return a;
}

void sgd_sum_apply(Tensor w, c10::optional<Tensor> mirror, std::vector<Tensor> srcs, Tensor hyper, double wd,
                   double gscale, c10::optional<Tensor> acc) {
  const SumArgs a = check_sum(w, mirror, srcs, hyper, acc, {});
  c10::DeviceGuard dg(w.device());
  dtg::sgd_sum_apply(w.data_ptr<float>(), a.mirror, a.acc, a.src, a.k, a.bf16, w.numel(), hyper.data_ptr<float>(),
                     (float)wd, (float)gscale, cur_stream());
}

void momentum_sum_apply(Tensor w, c10::optional<Tensor> mirror, std::vector<Tensor> srcs, Tensor mom, Tensor hyper,
                        double mu, double wd, bool nesterov, double gscale, c10::optional<Tensor> acc) {
  const SumArgs a = check_sum(w, mirror, srcs, hyper, acc, {&mom});
  c10::DeviceGuard dg(w.device());
  dtg::momentum_sum_apply(w.data_ptr<float>(), a.mirror, a.acc, a.src, a.k, a.bf16, mom.data_ptr<float>(), w.numel(),
                          hyper.data_ptr<float>(), (float)mu, (float)wd, nesterov, (float)gscale, cur_stream());
}

void adagrad_sum_apply(Tensor w, c10::optional<Tensor> mirror, std::vector<Tensor> srcs, Tensor slot, Tensor hyper,
                       double eps, double gscale, c10::optional<Tensor> acc) {
  const SumArgs a = check_sum(w, mirror, srcs, hyper, acc, {&slot});
  c10::DeviceGuard dg(w.device());
  dtg::adagrad_sum_apply(w.data_ptr<float>(), a.mirror, a.acc, a.src, a.k, a.bf16, slot.data_ptr<float>(), w.numel(),
                         hyper.data_ptr<float>(), (float)eps, (float)gscale, cur_stream());
}

void adam_sum_apply(Tensor w, c10::optional<Tensor> mirror, std::vector<Tensor> srcs, Tensor m, Tensor v, Tensor hyper,
                    double b1, double b2, double eps, double wd, double gscale, c10::optional<Tensor> acc) {
  const SumArgs a = check_sum(w, mirror, srcs, hyper, acc, {&m, &v});
  c10::DeviceGuard dg(w.device());
  dtg::adam_sum_apply(w.data_ptr<float>(), a.mirror, a.acc, a.src, a.k, a.bf16, m.data_ptr<float>(),
                      v.data_ptr<float>(), w.numel(), hyper.data_ptr<float>(), (float)b1, (float)b2, (float)eps,
                      (float)wd, (float)gscale, cur_stream());
}

void grad_sum(Tensor acc, std::vector<Tensor> srcs, bool first, double scale) {
  CHECK_IN(acc);
  CHECK_DT(acc, at::kFloat);
  check_align(acc, "acc");
  dtg::GradSrcs gs;
  int k, bf16;
  std::tie(gs, k, bf16) = check_srcs(srcs, acc);
  c10::DeviceGuard dg(acc.device());
  dtg::grad_sum(acc.data_ptr<float>(), gs, k, bf16, acc.numel(), first, (float)scale, cur_stream());
}

// ---- gradient accumulation over micro-batches (parallel/accum.py) ----------------------------------------------
// acc: fp32, g: fp32 or bf16 of the same length, any contiguous views (no alignment demand: the launcher picks the
// scalar kernels for operands that are not 16-byte aligned); the two must not overlap.
void check_fold(const Tensor& acc, const Tensor& g) {
  CHECK_IN(acc);
  CHECK_IN(g);
  CHECK_DT(acc, at::kFloat);
  TORCH_CHECK(g.scalar_type() == at::kFloat || g.scalar_type() == at::kBFloat16, "g must be fp32 or bf16");
  TORCH_CHECK(acc.numel() == g.numel(), "acc / g size mismatch: ", acc.numel(), " vs ", g.numel());
  TORCH_CHECK(acc.device() == g.device(), "acc and g are on different devices");
  const char* a = static_cast<const char*>(acc.data_ptr());
  const char* b = static_cast<const char*>(g.data_ptr());
  TORCH_CHECK(a + acc.numel() * 4 <= b || b + g.numel() * g.element_size() <= a, "acc and g overlap");
}

void grad_fold(Tensor acc, Tensor g, bool first) {
  check_fold(acc, g);
  c10::DeviceGuard dg(acc.device());
  dtg::grad_fold(acc.data_ptr<float>(), g.data_ptr(), g.scalar_type() == at::kBFloat16, acc.numel(), first,
                 cur_stream());
}

void grad_unfold(Tensor g, Tensor acc, int64_t lo, int64_t hi) {
  check_fold(acc, g);
  TORCH_CHECK(0 <= lo && lo <= hi && hi <= g.numel(), "range [", lo, ", ", hi, ") outside [0, ", g.numel(), ")");
  c10::DeviceGuard dg(acc.device());
  dtg::grad_unfold(g.data_ptr(), g.scalar_type() == at::kBFloat16, acc.data_ptr<float>(), lo, hi, cur_stream());
}

// ---- checkpoint snapshot (snapshot.hip) ----------------------------------------------------------------------
// rows: HOST int64 [P, 4] = (offset, numel, I, RS), ascending and disjoint inside [0, n).  Returns the number of
// kStateChunk chunks.  Everything a kernel will index with is checked here, before any launch.
long long check_state_rows(const Tensor& rows, long long n) {
  TORCH_CHECK(rows.device().is_cpu() && rows.scalar_type() == at::kLong && rows.dim() == 2 && rows.size(1) == 4 &&
                  rows.is_contiguous(),
              "rows must be a contiguous host int64 [P, 4] table");
  const int64_t* r = rows.data_ptr<int64_t>();
  long long end = 0, chunks = 0;
  for (int64_t p = 0; p < rows.size(0); ++p) {
    const int64_t off = r[4 * p], numel = r[4 * p + 1], I = r[4 * p + 2], RS = r[4 * p + 3];
    TORCH_CHECK(numel >= 0 && numel < (1ll << 31) - 2 * dtg::kStateChunk, "row ", p, ": numel ", numel,
                " out of range");
    TORCH_CHECK(off >= end && off <= n && numel <= n - off, "row ", p, ": [", off, ", ", off + numel,
                ") is outside the buffer of ", n, " elements or overlaps the previous row");
    TORCH_CHECK(off % 4 == 0, "row ", p, ": offset ", off, " is not 16-byte aligned");
    TORCH_CHECK(I >= 1 && RS >= 1, "row ", p, ": I and RS must be positive");
    TORCH_CHECK(RS == 1 || numel % (I * RS) == 0, "row ", p, ": numel is no multiple of I * RS");
    end = off + numel;
    chunks += (numel + dtg::kStateChunk - 1) / dtg::kStateChunk;
  }
  TORCH_CHECK(chunks < (1ll << 31), "too many chunks");
  return chunks;
}

// the host-built chunk table of `rows`: int32 [C, 2] = (row, chunk within the row)
Tensor state_chunk_table(Tensor rows, int64_t n) {
  const long long C = check_state_rows(rows, n);
  Tensor out = at::empty({C, 2}, at::TensorOptions().dtype(at::kInt));
  int* o = out.data_ptr<int>();
  const int64_t* r = rows.data_ptr<int64_t>();
  for (int64_t p = 0; p < rows.size(0); ++p) {
    const int64_t nc = (r[4 * p + 1] + dtg::kStateChunk - 1) / dtg::kStateChunk;
    for (int64_t c = 0; c < nc; ++c) {
      *o++ = (int)p;
      *o++ = (int)c;
    }
  }
  return out;
}

struct StateArgs {
  dtg::StatePtrs ptrs;
  int k;
  long long n;
  int n_chunks;
};

StateArgs check_state(const std::vector<Tensor>& bufs, const Tensor& image, const Tensor& rows, const Tensor& rows_dev,
                      const Tensor& chunks_dev) {
  TORCH_CHECK(!bufs.empty() && bufs.size() <= (size_t)dtg::kMaxStateSrcs, "1..4 state buffers, got ", bufs.size());
  StateArgs a;
  a.k = (int)bufs.size();
  a.n = bufs[0].numel();
  const auto dev = bufs[0].device();
  for (size_t j = 0; j < bufs.size(); ++j) {
    const Tensor& s = bufs[j];
    CHECK_IN(s);
    TORCH_CHECK(s.scalar_type() == at::kFloat, "state buffer ", j, " must be fp32");
    TORCH_CHECK(s.numel() == a.n, "state buffer ", j, " size mismatch: ", s.numel(), " vs ", a.n);
    TORCH_CHECK(s.device() == dev, "state buffer ", j, " is on another device");
    TORCH_CHECK(((uintptr_t)s.data_ptr() % 16) == 0, "state buffer ", j, " must be 16-byte aligned");
    a.ptrs.p[j] = s.data_ptr<float>();
  }
  CHECK_IN(image);
  CHECK_DT(image, at::kFloat);
  TORCH_CHECK(image.device() == dev, "image is on another device");
  TORCH_CHECK(image.numel() == a.k * a.n, "image must hold ", a.k, " x ", a.n, " elements, got ", image.numel());
  TORCH_CHECK(((uintptr_t)image.data_ptr() % 16) == 0 && (a.k == 1 || a.n % 4 == 0), "image must be 16-byte aligned");
  const long long C = check_state_rows(rows, a.n);
  TORCH_CHECK(rows_dev.is_cuda() && rows_dev.device() == dev && rows_dev.scalar_type() == at::kLong &&
                  rows_dev.is_contiguous() && rows_dev.sizes() == rows.sizes(),
              "rows_dev must be the device copy of rows");
  TORCH_CHECK(chunks_dev.is_cuda() && chunks_dev.device() == dev && chunks_dev.scalar_type() == at::kInt &&
                  chunks_dev.is_contiguous() && chunks_dev.dim() == 2 && chunks_dev.size(0) == C &&
                  chunks_dev.size(1) == 2,
              "chunks_dev must be the device copy of the [", C, ", 2] chunk table of rows");
  a.n_chunks = (int)C;
  return a;
}

void state_pack(std::vector<Tensor> srcs, Tensor image, Tensor rows, Tensor rows_dev, Tensor chunks_dev) {
  const StateArgs a = check_state(srcs, image, rows, rows_dev, chunks_dev);
  c10::DeviceGuard dg(image.device());
  dtg::state_pack(a.ptrs, a.k, image.data_ptr<float>(), a.n, (const long long*)rows_dev.data_ptr<int64_t>(),
                  chunks_dev.data_ptr<int>(), a.n_chunks, cur_stream());
}

void state_unpack(std::vector<Tensor> dsts, Tensor image, Tensor rows, Tensor rows_dev, Tensor chunks_dev) {
  const StateArgs a = check_state(dsts, image, rows, rows_dev, chunks_dev);
  c10::DeviceGuard dg(image.device());
  dtg::state_unpack(a.ptrs, a.k, image.data_ptr<float>(), a.n, (const long long*)rows_dev.data_ptr<int64_t>(),
                    chunks_dev.data_ptr<int>(), a.n_chunks, cur_stream());
}

// ---- layer-wise adaptive optimizers and global-norm clipping (layerwise.hip) -----------------------------------
// rows: HOST int64 [P, 3] = (offset in the row's group, numel, first chunk) over every flat group of an optimizer.
// Returns the number of kLwChunk chunks; the first-chunk column must be the running chunk count.
long long check_lw_rows(const Tensor& rows) {
  TORCH_CHECK(rows.device().is_cpu() && rows.scalar_type() == at::kLong && rows.dim() == 2 && rows.size(1) == 3 &&
                  rows.is_contiguous(),
              "rows must be a contiguous host int64 [P, 3] table");
  const int64_t* r = rows.data_ptr<int64_t>();
  long long chunks = 0;
  for (int64_t p = 0; p < rows.size(0); ++p) {
    const int64_t off = r[3 * p], numel = r[3 * p + 1];
    TORCH_CHECK(numel >= 0 && numel < (1ll << 31) - 2 * dtg::kLwChunk, "row ", p, ": numel ", numel, " out of range");
    TORCH_CHECK(off >= 0 && off % 8 == 0, "row ", p, ": offset ", off, " is not a multiple of 8 elements");
    TORCH_CHECK(r[3 * p + 2] == chunks, "row ", p, ": first chunk ", r[3 * p + 2], ", expected ", chunks);
    chunks += (numel + dtg::kLwChunk - 1) / dtg::kLwChunk;
    TORCH_CHECK(chunks < (1ll << 30), "too many chunks");
  }
  return chunks;
}

// the host-built chunk table of `rows`: int32 [C, 2] = (row, chunk within the row)
Tensor lw_chunk_table(Tensor rows) {
  const long long C = check_lw_rows(rows);
  Tensor out = at::empty({C, 2}, at::TensorOptions().dtype(at::kInt));
  int* o = out.data_ptr<int>();
  const int64_t* r = rows.data_ptr<int64_t>();
  for (int64_t p = 0; p < rows.size(0); ++p) {
    const int64_t nc = (r[3 * p + 1] + dtg::kLwChunk - 1) / dtg::kLwChunk;
    for (int64_t c = 0; c < nc; ++c) {
      *o++ = (int)p;
      *o++ = (int)c;
    }
  }
  return out;
}

struct LwTab {
  const long long* rows;
  const int* chunks;
  int P, C;
};

LwTab check_lw_tab(const Tensor& rows, const Tensor& rows_dev, const Tensor& chunks_dev, const c10::Device& dev) {
  LwTab t;
  t.C = (int)check_lw_rows(rows);
  t.P = (int)rows.size(0);
  TORCH_CHECK(rows_dev.is_cuda() && rows_dev.device() == dev && rows_dev.scalar_type() == at::kLong &&
                  rows_dev.is_contiguous() && rows_dev.sizes() == rows.sizes(),
              "rows_dev must be the device copy of rows");
  TORCH_CHECK(chunks_dev.is_cuda() && chunks_dev.device() == dev && chunks_dev.scalar_type() == at::kInt &&
                  chunks_dev.is_contiguous() && chunks_dev.dim() == 2 && chunks_dev.size(0) == t.C &&
                  chunks_dev.size(1) == 2,
              "chunks_dev must be the device copy of the [", t.C, ", 2] chunk table of rows");
  t.rows = (const long long*)rows_dev.data_ptr<int64_t>();
  t.chunks = chunks_dev.data_ptr<int>();
  return t;
}

// A launch over the chunks [c_lo, c_hi) of one group, which owns the rows [row_lo, row_hi) and buffers of n
// elements: the interval lies inside the group's chunks and every row of the group inside the buffers.
void check_lw_span(const Tensor& rows, const LwTab& t, long long n, int64_t row_lo, int64_t row_hi, int64_t c_lo,
                   int64_t c_hi) {
  TORCH_CHECK(0 <= row_lo && row_lo <= row_hi && row_hi <= t.P, "rows [", row_lo, ", ", row_hi, ") out of range");
  const int64_t* r = rows.data_ptr<int64_t>();
  long long end = 0;
  for (int64_t p = row_lo; p < row_hi; ++p) {
    const int64_t off = r[3 * p], numel = r[3 * p + 1];
    TORCH_CHECK(off >= end && off <= n && numel <= n - off, "row ", p, ": [", off, ", ", off + numel,
                ") is outside the buffer of ", n, " elements or overlaps the previous row");
    end = off + numel;
  }
  const int64_t g_lo = row_lo < t.P ? r[3 * row_lo + 2] : t.C, g_hi = row_hi < t.P ? r[3 * row_hi + 2] : t.C;
  TORCH_CHECK(g_lo <= c_lo && c_lo <= c_hi && c_hi <= g_hi, "chunks [", c_lo, ", ", c_hi,
              ") are outside the group's [", g_lo, ", ", g_hi, ")");
}

void check_lw_buf(const Tensor& t, long long n, const c10::Device& dev, const char* what, bool f32_only = true) {
  CHECK_IN(t);
  TORCH_CHECK(t.scalar_type() == at::kFloat || (!f32_only && t.scalar_type() == at::kBFloat16), what,
              f32_only ? " must be fp32" : " must be fp32 or bf16");
  TORCH_CHECK(t.numel() == n, what, " size mismatch: ", t.numel(), " vs ", n);
  TORCH_CHECK(t.device() == dev, what, " is on another device");
  check_align(t, what);
}

float* check_lw_scratch(const Tensor& t, long long n, const c10::Device& dev, const char* what) {
  CHECK_IN(t);
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.numel() == n && t.device() == dev, what, " must hold ", n,
              " fp32 elements on the group's device");
  return t.data_ptr<float>();
}

void seg_sqnorm(c10::optional<Tensor> w, c10::optional<Tensor> g, Tensor partials, Tensor rows, Tensor rows_dev,
                Tensor chunks_dev, int64_t row_lo, int64_t row_hi, int64_t c_lo, int64_t c_hi) {
  const bool hw = w.has_value() && w->defined(), hg = g.has_value() && g->defined();
  TORCH_CHECK(hw || hg, "seg_sqnorm needs the master, the gradient or both");
  const Tensor& any = hw ? *w : *g;
  const long long n = any.numel();
  const auto dev = any.device();
  if (hw) check_lw_buf(*w, n, dev, "master");
  if (hg) check_lw_buf(*g, n, dev, "grad", false);
  const LwTab t = check_lw_tab(rows, rows_dev, chunks_dev, dev);
  check_lw_span(rows, t, n, row_lo, row_hi, c_lo, c_hi);
  float* part = check_lw_scratch(partials, 2ll * t.C, dev, "partials");
  c10::DeviceGuard dg(dev);
  dtg::seg_sqnorm(hw ? w->data_ptr<float>() : nullptr, hg ? g->data_ptr() : nullptr,
                  hg && g->scalar_type() == at::kBFloat16, t.rows, t.chunks, (int)c_lo, (int)(c_hi - c_lo), part, t.C,
                  cur_stream());
}

void lamb_moments(Tensor w, Tensor g, Tensor m, Tensor v, Tensor hyper, Tensor partials, Tensor rows, Tensor rows_dev,
                  Tensor chunks_dev, int64_t row_lo, int64_t row_hi, int64_t c_lo, int64_t c_hi, double b1, double b2,
                  double eps, double wd, double gscale, c10::optional<Tensor> clip, bool zero_grad) {
  const long long n = w.numel();
  const auto dev = w.device();
  check_lw_buf(w, n, dev, "master");
  check_lw_buf(g, n, dev, "grad", false);
  check_lw_buf(m, n, dev, "m");
  check_lw_buf(v, n, dev, "v");
  check_hyper(hyper);
  TORCH_CHECK(hyper.device() == dev, "hyper is on another device");
  const LwTab t = check_lw_tab(rows, rows_dev, chunks_dev, dev);
  check_lw_span(rows, t, n, row_lo, row_hi, c_lo, c_hi);
  float* part = check_lw_scratch(partials, 2ll * t.C, dev, "partials");
  c10::DeviceGuard dg(dev);
  dtg::lamb_moments(w.data_ptr<float>(), g.data_ptr(), g.scalar_type() == at::kBFloat16, m.data_ptr<float>(),
                    v.data_ptr<float>(), t.rows, t.chunks, (int)c_lo, (int)(c_hi - c_lo), part, t.C,
                    hyper.data_ptr<float>(), b1, b2, (float)eps, (float)wd, (float)gscale, clip_ptr(clip, w),
                    zero_grad, cur_stream());
}

void lamb_apply(Tensor w, c10::optional<Tensor> mirror, Tensor m, Tensor v, Tensor hyper, Tensor ratio, Tensor rows,
                Tensor rows_dev, Tensor chunks_dev, int64_t row_lo, int64_t row_hi, int64_t c_lo, int64_t c_hi,
                double b1, double b2, double eps, double wd) {
  const long long n = w.numel();
  const auto dev = w.device();
  check_lw_buf(w, n, dev, "master");
  check_lw_buf(m, n, dev, "m");
  check_lw_buf(v, n, dev, "v");
  const bool hm = mirror.has_value() && mirror->defined();
  if (hm) {
    check_lw_buf(*mirror, n, dev, "mirror", false);
    CHECK_DT(*mirror, at::kBFloat16);
  }
  check_hyper(hyper);
  TORCH_CHECK(hyper.device() == dev, "hyper is on another device");
  const LwTab t = check_lw_tab(rows, rows_dev, chunks_dev, dev);
  check_lw_span(rows, t, n, row_lo, row_hi, c_lo, c_hi);
  const float* rt = check_lw_scratch(ratio, t.P, dev, "ratio");
  c10::DeviceGuard dg(dev);
  dtg::lamb_apply(w.data_ptr<float>(), hm ? bfp(*mirror) : nullptr, m.data_ptr<float>(), v.data_ptr<float>(), t.rows,
                  t.chunks, (int)c_lo, (int)(c_hi - c_lo), hyper.data_ptr<float>(), b1, b2, (float)eps, (float)wd, rt,
                  cur_stream());
}

void lars_apply(Tensor w, c10::optional<Tensor> mirror, Tensor g, Tensor mom, Tensor hyper, Tensor ratio, Tensor rows,
                Tensor rows_dev, Tensor chunks_dev, int64_t row_lo, int64_t row_hi, int64_t c_lo, int64_t c_hi,
                double mu, double wd, double gscale, c10::optional<Tensor> clip, bool zero_grad) {
  const long long n = w.numel();
  const auto dev = w.device();
  check_lw_buf(w, n, dev, "master");
  check_lw_buf(g, n, dev, "grad", false);
  check_lw_buf(mom, n, dev, "momentum");
  const bool hm = mirror.has_value() && mirror->defined();
  if (hm) {
    check_lw_buf(*mirror, n, dev, "mirror", false);
    CHECK_DT(*mirror, at::kBFloat16);
  }
  check_hyper(hyper);
  TORCH_CHECK(hyper.device() == dev, "hyper is on another device");
  const LwTab t = check_lw_tab(rows, rows_dev, chunks_dev, dev);
  check_lw_span(rows, t, n, row_lo, row_hi, c_lo, c_hi);
  const float* rt = check_lw_scratch(ratio, t.P, dev, "ratio");
  c10::DeviceGuard dg(dev);
  dtg::lars_apply(w.data_ptr<float>(), hm ? bfp(*mirror) : nullptr, g.data_ptr(), g.scalar_type() == at::kBFloat16,
                  mom.data_ptr<float>(), t.rows, t.chunks, (int)c_lo, (int)(c_hi - c_lo), hyper.data_ptr<float>(),
                  (float)mu, (float)wd, (float)gscale, clip_ptr(clip, w), rt, zero_grad, cur_stream());
}

// group_rows: the first row past each group (ascending, the last one == P); adapt / wd per group
void seg_finalize(Tensor partials, Tensor rows, Tensor rows_dev, Tensor chunks_dev, std::vector<int64_t> group_rows,
                  std::vector<int64_t> adapt, std::vector<double> wd, int64_t rule, double clip_norm, double gscale,
                  double eta, double eps, Tensor norms, Tensor ratio, Tensor cfac) {
  const auto dev = partials.device();
  CHECK_CUDA(partials);
  const LwTab t = check_lw_tab(rows, rows_dev, chunks_dev, dev);
  const float* part = check_lw_scratch(partials, 2ll * t.C, dev, "partials");
  TORCH_CHECK(rule == dtg::kLwNone || rule == dtg::kLwLars || rule == dtg::kLwLamb, "rule in {0, 1, 2}");
  const size_t G = group_rows.size();
  TORCH_CHECK(G >= 1 && G <= (size_t)dtg::kMaxLwGroups && adapt.size() == G && wd.size() == G, "1..4 groups");
  dtg::LwGroups grp;
  int64_t prev = 0;
  for (size_t i = 0; i < G; ++i) {
    TORCH_CHECK(group_rows[i] >= prev && group_rows[i] <= t.P, "group_rows must ascend within [0, P]");
    prev = group_rows[i];
    grp.row_end[i] = (int)group_rows[i];
    grp.adapt[i] = adapt[i] ? 1 : 0;
    grp.wd[i] = (float)wd[i];
  }
  TORCH_CHECK(prev == t.P, "the last group must end at row P");
  float* nm = check_lw_scratch(norms, 2ll * t.P, dev, "norms");
  float* rt = check_lw_scratch(ratio, t.P, dev, "ratio");
  float* cf = check_lw_scratch(cfac, 1, dev, "cfac");
  c10::DeviceGuard dg(dev);
  dtg::seg_finalize(part, t.C, t.rows, t.P, grp, (int)rule, (float)clip_norm, (float)gscale, (float)eta, (float)eps, nm,
                    rt, cf, cur_stream());
}

void f32_to_bf16(Tensor x, Tensor y) {
  CHECK_IN(x);
  CHECK_IN(y);
  CHECK_DT(x, at::kFloat);
  CHECK_DT(y, at::kBFloat16);
  TORCH_CHECK(x.numel() == y.numel(), "size mismatch");
  c10::DeviceGuard dg(x.device());
  dtg::f32_to_bf16(x.data_ptr<float>(), bfp(y), x.numel(), cur_stream());
}

// ---- batchnorm -------------------------------------------------------------------------------
// x: NHWC-contiguous bf16 viewed as [M, C] (the caller passes channels_last tensors flattened).
std::tuple<Tensor, Tensor, Tensor> bn_fwd_train(Tensor x, c10::optional<Tensor> res, Tensor gamma, Tensor beta,
                                                Tensor rmean, Tensor rvar, double momentum, double eps, bool relu) {
  CHECK_IN(x);
  CHECK_DT(x, at::kBFloat16);
  TORCH_CHECK(x.dim() == 2, "x must be [M, C]");
  const long long M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
  for (const Tensor* t : {&gamma, &beta, &rmean, &rvar}) {
    CHECK_IN(*t);
    CHECK_DT(*t, at::kFloat);
    TORCH_CHECK(t->numel() == C, "per-channel tensor size mismatch");
  }
  if (res.has_value() && res->defined()) {
    CHECK_IN(*res);
    CHECK_DT(*res, at::kBFloat16);
    TORCH_CHECK(res->sizes() == x.sizes(), "residual shape mismatch");
  }
  c10::DeviceGuard dg(x.device());
  auto y = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto smean = at::empty({C}, fopt), sinv = at::empty({C}, fopt);
  auto ws = at::empty({dtg::bn_workspace_floats(M, C)}, fopt);
  dtg::bn_fwd_train(cbfp(x), res.has_value() && res->defined() ? cbfp(*res) : nullptr, bfp(y),
                    gamma.data_ptr<float>(), beta.data_ptr<float>(), rmean.data_ptr<float>(), rvar.data_ptr<float>(),
                    smean.data_ptr<float>(), sinv.data_ptr<float>(), ws.data_ptr<float>(), M, C, (float)momentum,
                    (float)eps, relu, cur_stream());
  return {y, smean, sinv};
}

Tensor bn_fwd_infer(Tensor x, c10::optional<Tensor> res, Tensor gamma, Tensor beta, Tensor rmean, Tensor rvar,
                    double eps, bool relu) {
  CHECK_IN(x);
  CHECK_DT(x, at::kBFloat16);
  TORCH_CHECK(x.dim() == 2, "x must be [M, C]");
  const long long M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
  for (const Tensor* t : {&gamma, &beta, &rmean, &rvar}) {
    CHECK_IN(*t);
    CHECK_DT(*t, at::kFloat);
    TORCH_CHECK(t->numel() == C, "per-channel tensor size mismatch");
  }
  if (res.has_value() && res->defined()) {
    CHECK_IN(*res);
    TORCH_CHECK(res->sizes() == x.sizes(), "residual shape mismatch");
  }
  c10::DeviceGuard dg(x.device());
  auto y = at::empty_like(x);
  auto ws = at::empty({2LL * C}, x.options().dtype(at::kFloat));
  dtg::bn_fwd_infer(cbfp(x), res.has_value() && res->defined() ? cbfp(*res) : nullptr, bfp(y),
                    gamma.data_ptr<float>(), beta.data_ptr<float>(), rmean.data_ptr<float>(), rvar.data_ptr<float>(),
                    ws.data_ptr<float>(), M, C, (float)eps, relu, cur_stream());
  return y;
}

// dgamma_acc / dbeta_acc given: the parameter gradients are ACCUMULATED into them (flat grads)
std::tuple<Tensor, c10::optional<Tensor>, Tensor, Tensor> bn_bwd(Tensor dy, c10::optional<Tensor> y, Tensor x,
                                                                  Tensor gamma, Tensor smean, Tensor sinv, bool relu,
                                                                  bool want_dres, c10::optional<Tensor> dgamma_acc,
                                                                  c10::optional<Tensor> dbeta_acc) {
  CHECK_IN(dy);
  CHECK_IN(x);
  CHECK_DT(dy, at::kBFloat16);
  CHECK_DT(x, at::kBFloat16);
  TORCH_CHECK(dy.sizes() == x.sizes() && x.dim() == 2, "dy/x must be [M, C]");
  const long long M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
  if (relu) {
    TORCH_CHECK(y.has_value() && y->defined(), "relu backward needs the saved output");
    CHECK_IN(*y);
    TORCH_CHECK(y->sizes() == x.sizes(), "y shape mismatch");
  }
  for (const Tensor* t : {&gamma, &smean, &sinv}) {
    CHECK_IN(*t);
    CHECK_DT(*t, at::kFloat);
    TORCH_CHECK(t->numel() == C, "per-channel tensor size mismatch");
  }
  c10::DeviceGuard dg(x.device());
  auto dx = at::empty_like(x);
  c10::optional<Tensor> dres;
  if (want_dres) dres = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  const bool acc = dgamma_acc.has_value() && dgamma_acc->defined() && dbeta_acc.has_value() && dbeta_acc->defined();
  Tensor dgamma, dbeta;
  if (acc) {
    dgamma = *dgamma_acc;
    dbeta = *dbeta_acc;
    for (const Tensor* t : {&dgamma, &dbeta}) {
      CHECK_IN(*t);
      CHECK_DT(*t, at::kFloat);
      TORCH_CHECK(t->numel() == C, "gradient accumulator size mismatch");
    }
  } else {
    dgamma = at::empty({C}, fopt);
    dbeta = at::empty({C}, fopt);
  }
  auto ws = at::empty({dtg::bn_workspace_floats(M, C) + C}, fopt);
  dtg::bn_bwd(cbfp(dy), relu ? cbfp(*y) : nullptr, cbfp(x), gamma.data_ptr<float>(), smean.data_ptr<float>(),
              sinv.data_ptr<float>(), bfp(dx), want_dres ? bfp(*dres) : nullptr, dgamma.data_ptr<float>(),
              dbeta.data_ptr<float>(), ws.data_ptr<float>(), M, C, relu, acc, cur_stream());
  return {dx, dres, dgamma, dbeta};
}

// ---- softmax cross entropy -----------------------------------------------------------------
std::tuple<Tensor, c10::optional<Tensor>, Tensor> softmax_xent(Tensor logits, Tensor labels, double scale,
                                                                bool want_grad) {
  CHECK_IN(logits);
  CHECK_IN(labels);
  TORCH_CHECK(logits.dim() == 2, "logits must be [B, V]");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits bf16/fp32");
  CHECK_DT(labels, at::kLong);
  TORCH_CHECK(labels.numel() == logits.size(0), "labels size mismatch");
  c10::DeviceGuard dg(logits.device());
  const long long B = logits.size(0);
  const int V = (int)logits.size(1);
  auto fopt = logits.options().dtype(at::kFloat);
  auto loss = at::empty({B}, fopt), lse = at::empty({B}, fopt);
  c10::optional<Tensor> dx;
  if (want_grad) dx = at::empty_like(logits);
  if (B > 0)
    dtg::softmax_xent(logits.data_ptr(), logits.scalar_type() == at::kBFloat16, reinterpret_cast<const long long*>(labels.data_ptr<int64_t>()), B, V,
                      (float)scale, loss.data_ptr<float>(), want_grad ? dx->data_ptr() : nullptr,
                      lse.data_ptr<float>(), cur_stream());
  return {loss, dx, lse};
}

// dlogits = (softmax(logits) - onehot(labels)) * scale * g, g a 0-d/1-element fp32 GPU tensor (the
// upstream gradient, read on the device: no host sync, no separate rescale pass)
Tensor softmax_xent_bwd(Tensor logits, Tensor labels, Tensor lse, Tensor g, double scale) {
  CHECK_IN(logits);
  CHECK_IN(labels);
  CHECK_IN(lse);
  TORCH_CHECK(logits.dim() == 2, "logits must be [B, V]");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits bf16/fp32");
  CHECK_DT(labels, at::kLong);
  CHECK_DT(lse, at::kFloat);
  const long long B = logits.size(0);
  const int V = (int)logits.size(1);
  TORCH_CHECK(labels.numel() == B && lse.numel() == B, "labels / lse size mismatch");
  CHECK_CUDA(g);
  TORCH_CHECK(g.numel() == 1, "g must hold one element");
  Tensor gf = g.scalar_type() == at::kFloat ? g.contiguous() : g.to(at::kFloat);
  c10::DeviceGuard dg(logits.device());
  auto dx = at::empty_like(logits);
  if (B > 0)
    dtg::softmax_xent_bwd(logits.data_ptr(), logits.scalar_type() == at::kBFloat16,
                          reinterpret_cast<const long long*>(labels.data_ptr<int64_t>()), lse.data_ptr<float>(), B, V,
                          (float)scale, gf.data_ptr<float>(), dx.data_ptr(), cur_stream());
  return dx;
}

// ---- GEMM ----------------------------------------------------------------------------------
// out[M,N] = act(alpha * op(A) op(B) + beta*out + bias).  a_kc: A stored [M,K] (else [K,M]);
// b_kc: B stored [N,K] (else [K,N]).  Row strides are taken from the 2-D tensors.
void gemm(Tensor A, bool a_kc, Tensor B, bool b_kc, Tensor out, double alpha, double beta,
          c10::optional<Tensor> bias, int64_t act, int64_t split_k, c10::optional<Tensor> aux, int64_t aux_mode,
          c10::optional<Tensor> colsum) {
  CHECK_CUDA(A);
  CHECK_CUDA(B);
  CHECK_CUDA(out);
  CHECK_DT(A, at::kBFloat16);
  CHECK_DT(B, at::kBFloat16);
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && out.dim() == 2, "gemm operands must be 2-D");
  TORCH_CHECK(A.stride(1) == 1 && B.stride(1) == 1 && out.stride(1) == 1, "inner dim must be contiguous");
  TORCH_CHECK(out.scalar_type() == at::kFloat || out.scalar_type() == at::kBFloat16, "out fp32/bf16");
  const int M = (int)(a_kc ? A.size(0) : A.size(1));
  const int K = (int)(a_kc ? A.size(1) : A.size(0));
  const int N = (int)(b_kc ? B.size(0) : B.size(1));
  const int Kb = (int)(b_kc ? B.size(1) : B.size(0));
  TORCH_CHECK(K == Kb, "gemm K mismatch: ", K, " vs ", Kb);
  TORCH_CHECK(out.size(0) == M && out.size(1) == N, "gemm out shape mismatch");
  TORCH_CHECK(K % 8 == 0 || (!a_kc && !b_kc), "K-contiguous operands need K % 8 == 0 (pad the reduction dim)");
  TORCH_CHECK(a_kc || M % 8 == 0, "K-major A needs M % 8 == 0");
  TORCH_CHECK(b_kc || N % 8 == 0, "K-major B needs N % 8 == 0");
  TORCH_CHECK(A.stride(0) % 8 == 0 && B.stride(0) % 8 == 0, "row strides must be 16-byte multiples");
  TORCH_CHECK(((uintptr_t)A.data_ptr() % 16) == 0 && ((uintptr_t)B.data_ptr() % 16) == 0, "16-byte alignment");
  const float* bptr = nullptr;
  if (bias.has_value() && bias->defined()) {
    CHECK_IN(*bias);
    CHECK_DT(*bias, at::kFloat);
    TORCH_CHECK(bias->numel() == N, "bias size mismatch");
    bptr = bias->data_ptr<float>();
  }
  void* auxp = nullptr;
  if (aux_mode != 0) {
    TORCH_CHECK(aux_mode >= 1 && aux_mode <= 4, "aux_mode in {0, 1, 2, 3, 4}");
    TORCH_CHECK(aux_mode != 3 || act != 0, "aux_mode 3 stores act'(pre): needs an activation");
    TORCH_CHECK(aux.has_value() && aux->defined(), "aux_mode needs an aux tensor");
    TORCH_CHECK(aux->is_cuda() && aux->scalar_type() == at::kBFloat16 && aux->dim() == 2, "aux must be bf16 2-D");
    TORCH_CHECK(aux->size(0) == M && aux->size(1) == N && aux->stride(0) == out.stride(0) && aux->stride(1) == 1,
                "aux must match out's shape and row stride");
    auxp = aux->data_ptr();
  }
  c10::DeviceGuard dg(A.device());
  if (colsum.has_value() && colsum->defined()) {
    // fused bias gradient: colsum[n] += sum_m out[m, n] (dgrad layout, bf16 out, plain alpha/beta)
    CHECK_IN(*colsum);
    CHECK_DT(*colsum, at::kFloat);
    TORCH_CHECK(colsum->numel() == N, "colsum must hold N floats");
    TORCH_CHECK(a_kc && !b_kc && out.scalar_type() == at::kBFloat16 && alpha == 1.0 && beta == 0.0,
                "colsum epilogue: A [M,K], B [K,N], bf16 out, alpha 1, beta 0");
    TORCH_CHECK(out.stride(0) % 8 == 0 && N % 8 == 0 && ((uintptr_t)out.data_ptr() % 16) == 0 &&
                    (bptr == nullptr || ((uintptr_t)bptr % 16) == 0) && (auxp == nullptr || ((uintptr_t)auxp % 16) == 0),
                "colsum epilogue needs 16-byte aligned rows");
    dtg::gemm_bf16_colsum(cbfp(A), A.stride(0), cbfp(B), B.stride(0), bfp(out), out.stride(0), M, N, K, bptr, (int)act,
                          auxp, (int)aux_mode, colsum->data_ptr<float>(), cur_stream());
    return;
  }
  int sk = split_k > 0 ? (int)split_k : dtg::gemm_pick_split(M, N, K, a_kc ? 1 : 0);
  Tensor ws;
  float* wsp = nullptr;
  if (sk > 1) {
    ws = at::empty({dtg::gemm_workspace_floats(M, N, K, sk)}, A.options().dtype(at::kFloat));
    wsp = ws.data_ptr<float>();
  }
  dtg::gemm_bf16(cbfp(A), A.stride(0), a_kc, cbfp(B), B.stride(0), b_kc, out.data_ptr(), out.stride(0),
                 out.scalar_type() == at::kBFloat16, M, N, K, (float)alpha, (float)beta, bptr, (int)act, sk, wsp,
                 cur_stream(), dtg::GemmBatch(), auxp, (int)aux_mode);
}

// ---- implicit-GEMM convolution -----------------------------------------------------------------
// Activations are NHWC-contiguous ("channels_last") bf16 tensors given as [N, H, W, C] views;
// the weight is [K, R, S, C] contiguous (a channels_last [K, C, R, S] parameter viewed as such).
void check_nhwc(const Tensor& t, const char* what) {
  CHECK_CUDA(t);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, what, " must be bf16");
  TORCH_CHECK(t.dim() == 4 && t.is_contiguous(), what, " must be a contiguous [N,H,W,C] tensor");
  TORCH_CHECK(((uintptr_t)t.data_ptr() % 16) == 0, what, " must be 16-byte aligned");
}

bool conv_supported(int64_t C, int64_t K, int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t which) {
  return dtg::conv_supported((int)C, (int)K, (int)R, (int)S, (int)stride, (int)pad, (int)which) != 0;
}

Tensor conv_fwd(Tensor x, Tensor w, int64_t stride, int64_t pad) {
  check_nhwc(x, "x");
  check_nhwc(w, "w");
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int K = w.size(0), R = w.size(1), S = w.size(2);
  TORCH_CHECK(w.size(3) == C, "weight channels mismatch");
  TORCH_CHECK(dtg::conv_supported(C, K, R, S, stride, pad, 0), "conv shape not supported by the HIP kernel");
  const int P = (H + 2 * pad - R) / stride + 1, Q = (W + 2 * pad - S) / stride + 1;
  TORCH_CHECK(P > 0 && Q > 0, "empty output");
  TORCH_CHECK((long long)N * H * W * C < (1LL << 31) && (long long)N * P * Q * K < (1LL << 31), "tensor too large");
  c10::DeviceGuard dg(x.device());
  auto y = at::empty({N, P, Q, K}, x.options());
  dtg::conv_fwd(cbfp(x), cbfp(w), bfp(y), N, H, W, C, K, R, S, stride, pad, cur_stream());
  return y;
}

// (a stride-1 dgrad that read the weight transposed to [C][(r,s,k)] measured equal within +-5 % on the
// ResNet-50 3x3 layers and was retired; conv_dgrad's wT argument stays for the kernel's K-contiguous form)

// dx (= or +=, beta) dgrad; `out` (optional, [N,H,W,C] bf16) receives it in place.  zero_rest=False: a
// strided dgrad leaves the rows no filter tap reaches unwritten (see gemm_bn's sub2_hw)
Tensor conv_dgrad(Tensor dy, Tensor w, int64_t H, int64_t W, int64_t stride, int64_t pad, c10::optional<Tensor> out,
                  double beta, bool zero_rest) {
  check_nhwc(dy, "dy");
  check_nhwc(w, "w");
  const int N = dy.size(0), P = dy.size(1), Q = dy.size(2), K = dy.size(3);
  const int R = w.size(1), S = w.size(2), C = w.size(3);
  TORCH_CHECK(w.size(0) == K, "weight/dy channel mismatch");
  TORCH_CHECK(dtg::conv_supported(C, K, R, S, stride, pad, 1), "dgrad shape not supported by the HIP kernel");
  TORCH_CHECK((H + 2 * pad - R) / stride + 1 == P && (W + 2 * pad - S) / stride + 1 == Q, "dgrad geometry mismatch");
  c10::DeviceGuard dg(dy.device());
  Tensor dx;
  if (out.has_value()) {
    dx = *out;
    check_nhwc(dx, "out");
    TORCH_CHECK(dx.size(0) == N && dx.size(1) == H && dx.size(2) == W && dx.size(3) == C, "out shape mismatch");
  } else {
    TORCH_CHECK(beta == 0.0, "beta != 0 needs out");
    dx = at::empty({N, H, W, C}, dy.options());
  }
  Tensor wT;
  TORCH_CHECK(zero_rest || (stride == 2 && R == 1 && S == 1 && pad == 0 && beta == 0.0),
              "zero_rest=False is for a stride-2 1x1 dgrad (beta 0)");
  dtg::conv_dgrad(cbfp(dy), cbfp(w), bfp(dx), N, H, W, C, K, R, S, stride, pad, (float)beta, cur_stream(),
                  dtg::BnEpi(), wT.defined() ? cbfp(wT) : nullptr, zero_rest ? 1 : 0);
  return dx;
}

// 8-channel input conv (the stem): x [N,H,W,8] NHWC, w [K, Kp] with Kp = ceil64(R*S*8), (r,s,c) columns.
// with_stats: also the forward BN statistics of y (returned partials, else an empty tensor).
// stride_w (0 = stride): a separate W stride -- the stem's pixel-pair form is a stride (2, 1) conv.
std::tuple<Tensor, Tensor> conv_fwd_c8(Tensor x, Tensor w, int64_t R, int64_t S, int64_t stride, int64_t pad,
                                       bool with_stats, int64_t stride_w) {
  check_nhwc(x, "x");
  CHECK_IN(w);
  CHECK_DT(w, at::kBFloat16);
  const int sw = stride_w > 0 ? (int)stride_w : (int)stride;
  const int N = x.size(0), H = x.size(1), W = x.size(2), K = w.size(0);
  TORCH_CHECK(x.size(3) == 8, "conv_fwd_c8 needs 8 input channels");
  TORCH_CHECK(w.dim() == 2 && w.size(1) == (R * S * 8 + 63) / 64 * 64, "w must be [K, ceil64(R*S*8)]");
  TORCH_CHECK(K % 64 == 0, "K % 64");
  TORCH_CHECK(stride > 0 && sw > 0 && pad >= 0, "bad stride / pad");
  const int P = (H + 2 * pad - R) / stride + 1, Q = (W + 2 * pad - S) / sw + 1;
  TORCH_CHECK(P > 0 && Q > 0 && (long long)N * P * Q * K < (1LL << 31), "bad geometry");
  c10::DeviceGuard dg(x.device());
  auto y = at::empty({N, P, Q, K}, x.options());
  Tensor part;
  dtg::BnEpi bn;
  if (with_stats) {
    part = zeros_f32((long long)dtg::kBnStatSlots * 2 * K, x);
    bn.part = part.data_ptr<float>();
    bn.mode = 1;
  } else {
    part = at::empty({0}, x.options().dtype(at::kFloat));
  }
  dtg::conv_fwd_c8(cbfp(x), cbfp(w), bfp(y), N, H, W, K, (int)R, (int)S, (int)stride, (int)pad, cur_stream(), bn, sw);
  return {y, part};
}

// ---- BN statistics fused into the producing GEMM / conv (dtg/bn_epi.cuh) ----------------------
// Statistics slots.  pooled: a buffer from a per-device ring of zeroed buffers which the consuming
// finalize (bn_*_part) zeroes again after reading -- no fill kernel per BN.  The caller must consume
// (or zero) every pooled buffer before kPartRing more are handed out; the fused ResNet bottleneck
// does (its producer -> consumer distance is at most 2).  Unpooled: a fresh zeroed tensor.
constexpr int kPartRing = 16;
constexpr long long kPartCap = (long long)dtg::kBnStatSlots * 2 * 2048;
Tensor bn_part(const Tensor& like, int64_t C, bool pooled = false) {
  if (!pooled || C > 2048) return zeros_f32((long long)dtg::kBnStatSlots * 2 * C, like);
  static Tensor* ring = new Tensor[64];  // per device; leaked on purpose (no teardown-order issues)
  static int next[64] = {0};
  const int dev = like.get_device();
  TORCH_CHECK(dev >= 0 && dev < 64, "device index");
  if (!ring[dev].defined()) ring[dev] = zeros_f32((long long)kPartRing * kPartCap, like);
  const int i = next[dev]++ % kPartRing;
  return ring[dev].narrow(0, i * kPartCap, (long long)dtg::kBnStatSlots * 2 * C);
}

dtg::BnEpi bn_bwd_epi(Tensor& part, const Tensor& x, const Tensor& mean, const Tensor& invstd, const Tensor& gamma,
                      const Tensor& beta, long long M, int C) {
  CHECK_IN(x);
  CHECK_DT(x, at::kBFloat16);
  TORCH_CHECK(x.numel() == M * C, "BN input shape mismatch");
  for (const Tensor* t : {&mean, &invstd, &gamma, &beta}) {
    CHECK_IN(*t);
    CHECK_DT(*t, at::kFloat);
    TORCH_CHECK(t->numel() == C, "per-channel tensor size mismatch");
  }
  dtg::BnEpi bn;
  bn.part = part.data_ptr<float>();
  bn.mode = 2;
  bn.x = cbfp(x);
  bn.mean = mean.data_ptr<float>();
  bn.invstd = invstd.data_ptr<float>();
  bn.gamma = gamma.data_ptr<float>();
  bn.beta = beta.data_ptr<float>();
  return bn;
}

// mode 1: out = A W^T (W [N,K]) + forward BN statistics of out.
// mode 2: dp = (dY W) * relu'(bn(x)) (W [K,N]) + backward BN partials (x, mean, invstd, gamma, beta given).
// mode 3: dp = [mask > 0] * (dY W + beta*out) written into `out` (beta = 1 when out is given), partials
//         with xhat from x (the BN input of the layer whose relu output `mask` is).
std::tuple<Tensor, Tensor> gemm_bn(Tensor A, Tensor B, int64_t mode, c10::optional<Tensor> x,
                                   c10::optional<Tensor> mean, c10::optional<Tensor> invstd,
                                   c10::optional<Tensor> gamma, c10::optional<Tensor> beta,
                                   c10::optional<Tensor> mask, c10::optional<Tensor> out, bool pooled,
                                   c10::optional<Tensor> x2, c10::optional<Tensor> mean2,
                                   c10::optional<Tensor> invstd2, c10::optional<Tensor> part2,
                                   c10::optional<std::tuple<int64_t, int64_t>> sub2_hw) {
  CHECK_IN(A);
  CHECK_DT(A, at::kBFloat16);
  CHECK_CUDA(B);
  CHECK_DT(B, at::kBFloat16);
  TORCH_CHECK(mode >= 1 && mode <= 3, "mode in {1, 2, 3}");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && B.stride(1) == 1, "2-D operands, contiguous rows");
  const int M = (int)A.size(0), K = (int)A.size(1);
  const int N = (int)(mode == 1 ? B.size(0) : B.size(1));
  TORCH_CHECK((mode == 1 ? B.size(1) : B.size(0)) == K, "gemm_bn K mismatch");
  TORCH_CHECK(K % 8 == 0 && N % 8 == 0 && B.stride(0) % 8 == 0, "K, N and row strides must be multiples of 8");
  TORCH_CHECK(((uintptr_t)A.data_ptr() % 16) == 0 && ((uintptr_t)B.data_ptr() % 16) == 0, "16-byte alignment");
  c10::DeviceGuard dg(A.device());
  Tensor o;
  float bt = 0.f;
  if (out.has_value() && out->defined()) {
    TORCH_CHECK(mode == 3, "accumulating into `out` is mode 3 only");
    o = *out;
    CHECK_IN(o);
    CHECK_DT(o, at::kBFloat16);
    TORCH_CHECK(o.numel() == (long long)M * N, "out shape mismatch");
    bt = 1.f;
  } else {
    o = at::empty({M, N}, A.options());
  }
  auto part = bn_part(A, N, pooled);
  dtg::BnEpi bn;
  if (mode >= 2) {
    TORCH_CHECK(x && mean && invstd && gamma && beta, "modes 2/3 need x, mean, invstd, gamma, beta");
    bn = bn_bwd_epi(part, *x, *mean, *invstd, *gamma, *beta, M, N);
    if (mode == 3) {
      TORCH_CHECK(mask.has_value() && mask->defined(), "mode 3 needs the mask tensor");
      CHECK_IN(*mask);
      bn.mode = 3;
      if (x2.has_value() && x2->defined()) {  // second BN on the same gradient (projection shortcut)
        TORCH_CHECK(mean2 && invstd2 && part2, "x2 needs mean2, invstd2 and part2");
        CHECK_IN(*x2);
        CHECK_DT(*x2, at::kBFloat16);
        TORCH_CHECK(x2->numel() == (long long)M * N, "x2 shape mismatch");
        for (const Tensor* t : {&*mean2, &*invstd2}) {
          CHECK_IN(*t);
          CHECK_DT(*t, at::kFloat);
          TORCH_CHECK(t->numel() == N, "per-channel tensor size mismatch");
        }
        CHECK_IN(*part2);
        CHECK_DT(*part2, at::kFloat);
        TORCH_CHECK(part2->numel() == (long long)dtg::kBnStatSlots * 2 * N, "part2 size mismatch");
        bn.x2 = cbfp(*x2);
        bn.mean2 = mean2->data_ptr<float>();
        bn.invstd2 = invstd2->data_ptr<float>();
        bn.part2 = part2->data_ptr<float>();
      }
      if (sub2_hw.has_value()) {  // `out` holds a stride-2 projection dgrad: only its even (h, w) rows are valid
        const auto [sh, sw] = *sub2_hw;
        TORCH_CHECK(bt != 0.f && sh > 0 && sw > 0 && (long long)M % (sh * sw) == 0, "sub2_hw needs out and M = N*H*W");
        dtg::bn_sub2_rows(bn, (int)sh, (int)sw);
      }
      if (mask->scalar_type() == at::kByte) {  // packed bits [M, N/8]
        TORCH_CHECK(mask->numel() == (long long)M * (N / 8), "mask bits shape mismatch");
        bn.maskbits = mask->data_ptr<uint8_t>();
      } else {
        CHECK_DT(*mask, at::kBFloat16);
        TORCH_CHECK(mask->numel() == (long long)M * N, "mask shape mismatch");
        bn.mask = cbfp(*mask);
      }
    }
  } else {
    bn.part = part.data_ptr<float>();
    bn.mode = 1;
  }
  dtg::gemm_bf16_bn(cbfp(A), A.stride(0), cbfp(B), B.stride(0), bfp(o), N, M, N, K, bt, bn, cur_stream());
  return {o, part};
}

std::tuple<Tensor, Tensor> conv_fwd_bn(Tensor x, Tensor w, int64_t stride, int64_t pad, bool pooled) {
  check_nhwc(x, "x");
  check_nhwc(w, "w");
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int K = w.size(0), R = w.size(1), S = w.size(2);
  TORCH_CHECK(w.size(3) == C, "weight channels mismatch");
  TORCH_CHECK(dtg::conv_supported(C, K, R, S, stride, pad, 0), "conv shape not supported by the HIP kernel");
  const int P = (H + 2 * pad - R) / stride + 1, Q = (W + 2 * pad - S) / stride + 1;
  TORCH_CHECK(P > 0 && Q > 0, "empty output");
  TORCH_CHECK((long long)N * H * W * C < (1LL << 31) && (long long)N * P * Q * K < (1LL << 31), "tensor too large");
  c10::DeviceGuard dg(x.device());
  auto y = at::empty({N, P, Q, K}, x.options());
  auto part = bn_part(x, K, pooled);
  // (3x3 / s1 / p1, 64 -> 64: conv_fwd takes the direct halo-tile conv, csrc/kernels/conv_halo.hip)
  dtg::BnEpi bn;
  bn.part = part.data_ptr<float>();
  bn.mode = 1;
  dtg::conv_fwd(cbfp(x), cbfp(w), bfp(y), N, H, W, C, K, R, S, stride, pad, cur_stream(), bn);
  return {y, part};
}

// dp = dgrad(dy, w) * relu'(bn(x)) with backward BN partials; x is the BN input [N,H,W,C]
uint8_t* bits_ptr(const c10::optional<Tensor>& bits, long long M, int C) {
  if (!bits.has_value() || !bits->defined()) return nullptr;
  CHECK_IN(*bits);
  TORCH_CHECK(bits->scalar_type() == at::kByte && bits->numel() == M * (C / 8), "bits must be uint8 [M, C/8]");
  return bits->data_ptr<uint8_t>();
}

std::tuple<Tensor, Tensor> conv_dgrad_bn(Tensor dy, Tensor w, int64_t H, int64_t W, int64_t stride, int64_t pad,
                                         Tensor x, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta,
                                         bool pooled, c10::optional<Tensor> bits) {
  check_nhwc(dy, "dy");
  check_nhwc(w, "w");
  const int N = dy.size(0), P = dy.size(1), Q = dy.size(2), K = dy.size(3);
  const int R = w.size(1), S = w.size(2), C = w.size(3);
  TORCH_CHECK(w.size(0) == K, "weight/dy channel mismatch");
  TORCH_CHECK(dtg::conv_supported(C, K, R, S, stride, pad, 1), "dgrad shape not supported by the HIP kernel");
  TORCH_CHECK((H + 2 * pad - R) / stride + 1 == P && (W + 2 * pad - S) / stride + 1 == Q, "dgrad geometry mismatch");
  c10::DeviceGuard dg(dy.device());
  auto dx = at::empty({N, H, W, C}, dy.options());
  auto part = bn_part(dy, C, pooled);
  dtg::BnEpi bn = bn_bwd_epi(part, x, mean, invstd, gamma, beta, (long long)N * H * W, C);
  if (uint8_t* mb = bits_ptr(bits, (long long)N * H * W, C)) {  // the forward's packed relu mask: mode 3, beta 0
    bn.mode = 3;
    bn.maskbits = mb;
  }
  // stride 1: the kernel reads the weight transposed to [C][(r,s,k)] (K-contiguous; ~1 MB, one small copy)
  Tensor wT;
  TORCH_CHECK(dtg::conv_dgrad(cbfp(dy), cbfp(w), bfp(dx), N, H, W, C, K, R, S, stride, pad, 0.f, cur_stream(), bn,
                              wT.defined() ? cbfp(wT) : nullptr),
              "conv_dgrad_bn: geometry leaves rows unwritten (use conv_dgrad + bn_bwd)");
  return {dx, part};
}

// the BN-part bindings' repeated checks: fp32, contiguous on the device, n elements ...
static void check_f32(std::initializer_list<const Tensor*> ts, long long n, const char* what) {
  for (const Tensor* t : ts) {
    CHECK_IN(*t);
    CHECK_DT(*t, at::kFloat);
    TORCH_CHECK(t->numel() == n, what, " size mismatch");
  }
}
// ... per-channel parameters, statistics and gradient accumulators [C]; epilogue partials [kBnStatSlots][2][C]
static void check_per_channel(std::initializer_list<const Tensor*> ts, int C) {
  check_f32(ts, C, "per-channel tensor");
}
static void check_partials(std::initializer_list<const Tensor*> ts, int C) {
  check_f32(ts, (long long)dtg::kBnStatSlots * 2 * C, "partials");
}

// The next block's conv1 inside the apply pass (dtg::BnNextConv; check bn_apply_gemm_ok first): nw [N, C] is its
// weight, npart a zeroed partial slot for the statistics of y1n = out nw^T, which the op then returns last
static bool next_conv(const c10::optional<Tensor>& nw, const c10::optional<Tensor>& npart, const Tensor& x, bool form_ok,
                      bool two, dtg::BnNextConv& nx, Tensor& y1n) {
  if (!nw.has_value() || !nw->defined()) return false;
  const long long M = x.size(0);
  const int C = (int)x.size(1);
  CHECK_CUDA(*nw);
  CHECK_DT(*nw, at::kBFloat16);
  TORCH_CHECK(nw->dim() == 2 && nw->size(1) == C && nw->stride(1) == 1 && nw->stride(0) % 8 == 0 &&
                  ((uintptr_t)nw->data_ptr() % 16) == 0,
              "next weight must be [N, C] with 16-byte aligned rows");
  const int N = (int)nw->size(0);
  TORCH_CHECK(form_ok && dtg::bn_apply_gemm_ok(M, C, N) && !(two && C == 256 && N != 64),
              "bn_apply_gemm: unsupported shape or form (bn_apply_gemm_ok)");
  TORCH_CHECK(npart.has_value() && npart->defined(), "next weight needs next_part");
  check_f32({&*npart}, (long long)dtg::kBnStatSlots * 2 * N, "next_part");
  y1n = at::empty({M, N}, x.options());
  nx.w = cbfp(*nw);
  nx.ldw = nw->stride(0);
  nx.N = N;
  nx.y = bfp(y1n);
  nx.part = npart->data_ptr<float>();
  return true;
}

// bits (optional uint8 [M, C/8]) receives the packed (out > 0) relu mask
pybind11::tuple bn_fwd_part(Tensor x, Tensor part, c10::optional<Tensor> res, Tensor gamma, Tensor beta, Tensor rmean,
                            Tensor rvar, double momentum, double eps, bool relu, c10::optional<Tensor> bits,
                            c10::optional<Tensor> next_w, c10::optional<Tensor> next_part) {
  CHECK_IN(x);
  CHECK_DT(x, at::kBFloat16);
  TORCH_CHECK(x.dim() == 2, "x must be [M, C]");
  const long long M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
  check_partials({&part}, C);
  check_per_channel({&gamma, &beta, &rmean, &rvar}, C);
  const bool has_res = res.has_value() && res->defined();
  if (has_res) {
    CHECK_IN(*res);
    CHECK_DT(*res, at::kBFloat16);
    TORCH_CHECK(res->sizes() == x.sizes(), "residual shape mismatch");
  }
  c10::DeviceGuard dg(x.device());
  dtg::BnNextConv nx;
  Tensor y1n;
  const bool fuse = next_conv(next_w, next_part, x, has_res && relu, false, nx, y1n);
  auto y = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto smean = at::empty({C}, fopt), sinv = at::empty({C}, fopt), ws = at::empty({2LL * C}, fopt);
  dtg::bn_fwd_from_part(cbfp(x), has_res ? cbfp(*res) : nullptr, bfp(y), gamma.data_ptr<float>(),
                        beta.data_ptr<float>(), rmean.data_ptr<float>(), rvar.data_ptr<float>(),
                        smean.data_ptr<float>(), sinv.data_ptr<float>(), part.data_ptr<float>(), ws.data_ptr<float>(),
                        M, C, (float)momentum, (float)eps, relu, cur_stream(), bits_ptr(bits, M, C),
                        fuse ? &nx : nullptr);
  if (fuse) return pybind11::make_tuple(y, smean, sinv, y1n);
  return pybind11::make_tuple(y, smean, sinv);
}

// out = relu(bn(x) + bn2(r)), both from epilogue partials -> (out, mean, invstd, mean2, invstd2)
pybind11::tuple bn_fwd2_part(Tensor x, Tensor part, Tensor gamma, Tensor beta, Tensor rmean, Tensor rvar, Tensor r,
                             Tensor part2, Tensor gamma2, Tensor beta2, Tensor rmean2, Tensor rvar2, double momentum,
                             double eps, c10::optional<Tensor> bits, c10::optional<Tensor> next_w,
                             c10::optional<Tensor> next_part) {
  CHECK_IN(x);
  CHECK_IN(r);
  CHECK_DT(x, at::kBFloat16);
  CHECK_DT(r, at::kBFloat16);
  TORCH_CHECK(x.dim() == 2 && r.sizes() == x.sizes(), "x/r must be [M, C]");
  const long long M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
  check_partials({&part, &part2}, C);
  check_per_channel({&gamma, &beta, &rmean, &rvar, &gamma2, &beta2, &rmean2, &rvar2}, C);
  c10::DeviceGuard dg(x.device());
  dtg::BnNextConv nx;
  Tensor y1n;
  const bool fuse = next_conv(next_w, next_part, x, true, true, nx, y1n);
  auto y = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto m1 = at::empty({C}, fopt), i1 = at::empty({C}, fopt), m2 = at::empty({C}, fopt), i2 = at::empty({C}, fopt);
  auto ws = at::empty({4LL * C}, fopt);
  dtg::bn_fwd2_from_part(cbfp(x), cbfp(r), bfp(y), part.data_ptr<float>(), part2.data_ptr<float>(),
                         gamma.data_ptr<float>(), beta.data_ptr<float>(), rmean.data_ptr<float>(),
                         rvar.data_ptr<float>(), m1.data_ptr<float>(), i1.data_ptr<float>(), gamma2.data_ptr<float>(),
                         beta2.data_ptr<float>(), rmean2.data_ptr<float>(), rvar2.data_ptr<float>(),
                         m2.data_ptr<float>(), i2.data_ptr<float>(), ws.data_ptr<float>(), M, C, (float)momentum,
                         (float)eps, cur_stream(), bits_ptr(bits, M, C), fuse ? &nx : nullptr);
  if (fuse) return pybind11::make_tuple(y, m1, i1, m2, i2, y1n);
  return pybind11::make_tuple(y, m1, i1, m2, i2);
}

// dx, dx2 of two BNs fed by the same masked gradient dp (BN3 + projection BN), parameter gradients
// accumulated into the given fp32 accumulators
// fused weight gradient (both bn_bwd*_part): with `wact` [M, CI] (the input of the conv whose output is x) and
// `wgrad` [C, CI] fp32, wgrad += dx^T wact inside the dx pass (bn_dx_wgrad.hip) -- check bn_dx_wgrad_ok first
static void check_wgrad_fuse(const Tensor& x, const c10::optional<Tensor>& wact, const c10::optional<Tensor>& wgrad) {
  TORCH_CHECK(wact.has_value() && wgrad.has_value() && wact->defined() && wgrad->defined(), "wact needs wgrad");
  CHECK_CUDA(*wact);
  CHECK_DT(*wact, at::kBFloat16);
  CHECK_IN(*wgrad);
  TORCH_CHECK(wgrad->scalar_type() == at::kFloat || wgrad->scalar_type() == at::kBFloat16, "wgrad fp32/bf16");
  const long long M = x.size(0);
  const int C = (int)x.size(1), CI = (int)wact->size(1);
  TORCH_CHECK(wact->dim() == 2 && wact->size(0) == M && wact->stride(1) == 1 && wact->stride(0) % 8 == 0 &&
                  ((uintptr_t)wact->data_ptr() % 16) == 0,
              "wact must be [M, CI] with 16-byte aligned rows");
  TORCH_CHECK(wgrad->numel() == (long long)C * CI, "wgrad must be [C, CI]");
  TORCH_CHECK(dtg::bn_dx_wgrad_ok(M, C, CI), "fused dx + wgrad: unsupported shape (see bn_dx_wgrad_ok)");
}

// fused data gradient (both bn_bwd*_part, with wact; 256 x 64 -- check bn_dx_dgrad_ok first): with `dgw` [C, CI]
// (that conv's weight as its dgrad GEMM reads it), the BN below it (`dgy` [M, CI] its input, `dgmean` / `dginv` its
// saved statistics, `dgbits` [M, CI / 8] the packed relu mask of its output) and `dgpart` (its zeroed partial
// slots, bn_part_alloc), the pass also computes what gemm_bn(dx, dgw, 3, ..., mask=dgbits) would: the calls then
// return dp [M, CI] and dgpart after their usual results, and dx is neither written nor allocated (None).
// `dgfull` asks for the full-width form instead (512 x 128 -- check bn_dx_dgrad_full_ok first; bn_bwd_part only:
// the dual form of that width is not built).
// `dgx` = True is the caller's word that x is bf16(wact dgw^T) -- the forward output of that conv, with both operands
// unmodified since: the pass then forms x again from wact and dgw, which it holds anyway, and does not read it (256 x 64
// -- check bn_dx_recompute_ok first).  x is still passed and shape-checked.
struct DgradFuse {
  c10::optional<Tensor> w, y, mean, invstd, bits, part;
  bool full = false;
  bool rx = false;
  bool on() const { return w.has_value() && w->defined(); }
};

// dgx rides on the fused dgrad: refused by name without its operands or outside the forms that have it
static void check_dgx(const DgradFuse& f, const Tensor& x, const c10::optional<Tensor>& wact, bool dual) {
  if (!f.rx) return;
  TORCH_CHECK(f.on(), "dgx needs dgw (x is recomputed from the fused dgrad's weight)");
  TORCH_CHECK(wact.has_value() && wact->defined(), "dgx needs wact (x is recomputed from the conv's input)");
  TORCH_CHECK(!f.full && wact->dim() == 2 && dtg::bn_dx_recompute_ok(x.size(0), (int)x.size(1), (int)wact->size(1), dual),
              "dgx: unsupported shape or form (see bn_dx_recompute_ok)");
}

static dtg::DxDgrad check_dgrad_fuse(const Tensor& x, const c10::optional<Tensor>& wact, const DgradFuse& f,
                                     const Tensor& dpo) {
  TORCH_CHECK(wact.has_value() && wact->defined(), "the fused dgrad rides on the fused weight gradient (wact)");
  for (const c10::optional<Tensor>* t : {&f.y, &f.mean, &f.invstd, &f.bits, &f.part})
    TORCH_CHECK(t->has_value() && (*t)->defined(), "dgw needs dgy, dgmean, dginv, dgbits and dgpart");
  const long long M = x.size(0);
  const int C = (int)x.size(1), CI = (int)wact->size(1);
  TORCH_CHECK(f.full || dtg::bn_dx_dgrad_ok(M, C, CI), "fused dx + dgrad: unsupported shape (see bn_dx_dgrad_ok)");
  TORCH_CHECK(!f.full || dtg::bn_dx_dgrad_full_ok(M, C, CI),
              "fused dx + dgrad: unsupported shape (see bn_dx_dgrad_full_ok)");
  CHECK_CUDA(*f.w);
  CHECK_DT(*f.w, at::kBFloat16);
  TORCH_CHECK(f.w->dim() == 2 && f.w->size(0) == C && f.w->size(1) == CI && f.w->stride(1) == 1 &&
                  f.w->stride(0) % 8 == 0 && ((uintptr_t)f.w->data_ptr() % 16) == 0,
              "dgw must be [C, CI] with 16-byte aligned rows");
  CHECK_IN(*f.y);
  CHECK_DT(*f.y, at::kBFloat16);
  TORCH_CHECK(f.y->dim() == 2 && f.y->size(0) == M && f.y->size(1) == CI && ((uintptr_t)f.y->data_ptr() % 16) == 0,
              "dgy must be [M, CI], 16-byte aligned");
  check_per_channel({&*f.mean, &*f.invstd}, CI);
  check_partials({&*f.part}, CI);
  dtg::DxDgrad d;
  d.w = cbfp(*f.w);
  d.ldw = f.w->stride(0);
  d.y = cbfp(*f.y);
  d.mean = f.mean->data_ptr<float>();
  d.invstd = f.invstd->data_ptr<float>();
  d.bits = bits_ptr(f.bits, M, CI);
  d.dp = bfp(dpo);
  d.part = f.part->data_ptr<float>();
  d.recompute_x = f.rx;
  return d;
}

// the fused branch of both bn_bwd*_part (bn_dx_wgrad.hip): one side per BN fed by dp -- BN3 with conv3's weight
// gradient, and in bn_bwd2_part the projection BN, with the shortcut conv's where wact2 is given
struct DxFuseSide {
  const Tensor &x, &part, &gamma, &smean, &sinv, &dgamma, &dbeta;
  const Tensor& dx;  // undefined: not written (BN3's with dgw)
  const c10::optional<Tensor> &wact, &wgrad;
};

// the parameter gradients and dx coefficients of each side (ws: 3C floats per side), then the pass; returns the fused
// dgrad's dp [M, CI] (undefined without dgw)
static Tensor bn_dx_wgrad_fused(const Tensor& dp, const DxFuseSide& a, const DxFuseSide* b, const Tensor& ws, int accum,
                                const DgradFuse& dgf) {
  const long long M = a.x.size(0);
  const int C = (int)a.x.size(1);
  check_wgrad_fuse(a.x, a.wact, a.wgrad);
  const int CI = (int)a.wact->size(1);
  const bool w2 = b && b->wact.has_value() && b->wact->defined();
  if (w2) {  // the projection shortcut's weight gradient too: dW2 += dx2^T wact2 (256 x 64 only)
    check_wgrad_fuse(b->x, b->wact, b->wgrad);
    TORCH_CHECK(C == 256 && CI == 64 && b->wact->size(1) == CI && b->wgrad->scalar_type() == a.wgrad->scalar_type(),
                "wact2: 256 x 64 only, wgrad2 of wgrad's dtype");
  }
  Tensor dpo;
  dtg::DxDgrad dgd;
  if (dgf.on()) {  // conv3's data gradient too (the dual form has it with both weight gradients only)
    TORCH_CHECK(!b || w2, "dgw in the dual form needs wact2");
    dpo = at::empty({M, (long long)CI}, a.x.options());
    dgd = check_dgrad_fuse(a.x, a.wact, dgf, dpo);
  }
  const long long ns = (long long)dtg::bn_dx_wgrad_slabs(C, CI, w2, dgf.on()) * C * CI;
  auto slabs = at::empty({w2 ? 2 * ns : ns}, a.x.options().dtype(at::kFloat));
  auto side = [&](const DxFuseSide& s, int k) {
    dtg::DxSide d;
    d.x = cbfp(s.x);
    float* coef = ws.data_ptr<float>() + k * 3LL * C;
    dtg::bn_bwd_coef_from_part(s.part.data_ptr<float>(), s.gamma.data_ptr<float>(), s.smean.data_ptr<float>(),
                               s.sinv.data_ptr<float>(), coef, s.dgamma.data_ptr<float>(), s.dbeta.data_ptr<float>(),
                               M, C, accum, cur_stream());
    d.coef = coef;
    d.dx = s.dx.defined() ? bfp(s.dx) : nullptr;
    if (s.wact.has_value() && s.wact->defined()) {
      d.act = cbfp(*s.wact);
      d.ldact = s.wact->stride(0);
      d.wgrad = s.wgrad->data_ptr();
      d.slabs = slabs.data_ptr<float>() + k * ns;
    }
    return d;
  };
  const dtg::DxSide da = side(a, 0), db = b ? side(*b, 1) : dtg::DxSide{};
  dtg::bn_dx_wgrad(cbfp(dp), da, b ? &db : nullptr, M, C, CI, a.wgrad->scalar_type() == at::kBFloat16, cur_stream(),
                   dgf.on() ? &dgd : nullptr);
  return dpo;
}

pybind11::tuple bn_bwd2_part(Tensor dp, Tensor x, Tensor part, Tensor gamma, Tensor smean, Tensor sinv,
                             Tensor dgamma, Tensor dbeta, Tensor x2, Tensor part2, Tensor gamma2,
                             Tensor smean2, Tensor sinv2, Tensor dgamma2, Tensor dbeta2,
                             c10::optional<Tensor> wact, c10::optional<Tensor> wgrad,
                             c10::optional<Tensor> wact2, c10::optional<Tensor> wgrad2,
                             c10::optional<Tensor> dgw, c10::optional<Tensor> dgy, c10::optional<Tensor> dgmean,
                             c10::optional<Tensor> dginv, c10::optional<Tensor> dgbits,
                             c10::optional<Tensor> dgpart, bool dgfull, bool dgx) {
  const DgradFuse dgf{dgw, dgy, dgmean, dginv, dgbits, dgpart, dgfull, dgx};
  TORCH_CHECK(!(dgfull && dgf.on()), "dgfull: the full-width fused dgrad has no dual form (bn_bwd_part only)");
  for (const Tensor* t : {&dp, &x, &x2}) {
    CHECK_IN(*t);
    CHECK_DT(*t, at::kBFloat16);
  }
  TORCH_CHECK(x.dim() == 2 && dp.numel() == x.numel() && x2.sizes() == x.sizes(), "dp/x/x2 must be [M, C]");
  const long long M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
  check_partials({&part, &part2}, C);
  check_per_channel({&gamma, &smean, &sinv, &dgamma, &dbeta, &gamma2, &smean2, &sinv2, &dgamma2, &dbeta2}, C);
  c10::DeviceGuard dg(x.device());
  check_dgx(dgf, x, wact, true);
  TORCH_CHECK(!dgf.on() || (wact.has_value() && wact->defined()), "dgw needs wact");
  Tensor dx, dx2 = at::empty_like(x);
  if (!dgf.on()) dx = at::empty_like(x);
  auto ws = at::empty({6LL * C}, x.options().dtype(at::kFloat));
  if (wact.has_value() && wact->defined()) {
    const DxFuseSide a{x, part, gamma, smean, sinv, dgamma, dbeta, dx, wact, wgrad};
    const DxFuseSide b{x2, part2, gamma2, smean2, sinv2, dgamma2, dbeta2, dx2, wact2, wgrad2};
    const Tensor dpo = bn_dx_wgrad_fused(dp, a, &b, ws, 1, dgf);
    if (dgf.on()) return pybind11::make_tuple(pybind11::none(), dx2, dpo, *dgf.part);
    return pybind11::make_tuple(dx, dx2);
  }
  dtg::bn_bwd2_from_part(cbfp(dp), cbfp(x), cbfp(x2), part.data_ptr<float>(), part2.data_ptr<float>(),
                         gamma.data_ptr<float>(), smean.data_ptr<float>(), sinv.data_ptr<float>(),
                         gamma2.data_ptr<float>(), smean2.data_ptr<float>(), sinv2.data_ptr<float>(), bfp(dx),
                         bfp(dx2), dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), dgamma2.data_ptr<float>(),
                         dbeta2.data_ptr<float>(), ws.data_ptr<float>(), M, C, 1, cur_stream());
  return pybind11::make_tuple(dx, dx2);
}

pybind11::tuple bn_bwd_part(Tensor dp, Tensor x, Tensor part, Tensor gamma, Tensor smean, Tensor sinv, bool want_dres,
                            c10::optional<Tensor> dgamma_acc, c10::optional<Tensor> dbeta_acc,
                            c10::optional<Tensor> wact, c10::optional<Tensor> wgrad, c10::optional<Tensor> dgw,
                            c10::optional<Tensor> dgy, c10::optional<Tensor> dgmean, c10::optional<Tensor> dginv,
                            c10::optional<Tensor> dgbits, c10::optional<Tensor> dgpart, bool dgfull, bool dgx) {
  const DgradFuse dgf{dgw, dgy, dgmean, dginv, dgbits, dgpart, dgfull, dgx};
  CHECK_IN(dp);
  CHECK_IN(x);
  CHECK_DT(dp, at::kBFloat16);
  CHECK_DT(x, at::kBFloat16);
  TORCH_CHECK(x.dim() == 2 && dp.numel() == x.numel(), "dp/x must be [M, C]");
  const long long M = x.size(0);
  const int C = (int)x.size(1);
  TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
  check_partials({&part}, C);
  check_per_channel({&gamma, &smean, &sinv}, C);
  c10::DeviceGuard dg(x.device());
  check_dgx(dgf, x, wact, false);
  TORCH_CHECK(!dgf.on() || (wact.has_value() && wact->defined()), "dgw needs wact");
  Tensor dx;
  if (!dgf.on()) dx = at::empty_like(x);
  c10::optional<Tensor> dres;
  if (want_dres) dres = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  const bool acc = dgamma_acc.has_value() && dgamma_acc->defined() && dbeta_acc.has_value() && dbeta_acc->defined();
  Tensor dgamma, dbeta;
  if (acc) {
    dgamma = *dgamma_acc;
    dbeta = *dbeta_acc;
    check_per_channel({&dgamma, &dbeta}, C);
  } else {
    dgamma = at::empty({C}, fopt);
    dbeta = at::empty({C}, fopt);
  }
  auto ws = at::empty({3LL * C}, fopt);
  if (wact.has_value() && wact->defined()) {
    TORCH_CHECK(!want_dres, "fused dx + wgrad: no dres");
    const Tensor dpo =
        bn_dx_wgrad_fused(dp, {x, part, gamma, smean, sinv, dgamma, dbeta, dx, wact, wgrad}, nullptr, ws, acc, dgf);
    if (dgf.on()) return pybind11::make_tuple(pybind11::none(), dres, dgamma, dbeta, dpo, *dgf.part);
    return pybind11::make_tuple(dx, dres, dgamma, dbeta);
  }
  dtg::bn_bwd_from_part(cbfp(dp), cbfp(x), gamma.data_ptr<float>(), smean.data_ptr<float>(), sinv.data_ptr<float>(),
                        part.data_ptr<float>(), bfp(dx), want_dres ? bfp(*dres) : nullptr, dgamma.data_ptr<float>(),
                        dbeta.data_ptr<float>(), ws.data_ptr<float>(), M, C, acc, cur_stream());
  return pybind11::make_tuple(dx, dres, dgamma, dbeta);
}

// dw (+)= wgrad; dw is [K, R, S, C] contiguous, fp32 or bf16 (beta = 1 accumulates into a flat grad)
void conv_wgrad(Tensor dy, Tensor x, Tensor dw, double beta, int64_t stride, int64_t pad, int64_t stride_w,
                int64_t target_wgs, int64_t sched) {
  check_nhwc(dy, "dy");
  check_nhwc(x, "x");
  CHECK_CUDA(dw);
  TORCH_CHECK(dw.dim() == 4 && dw.is_contiguous(), "dw must be contiguous [K,R,S,C]");
  TORCH_CHECK(dw.scalar_type() == at::kFloat || dw.scalar_type() == at::kBFloat16, "dw fp32/bf16");
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int K = dw.size(0), R = dw.size(1), S = dw.size(2);
  TORCH_CHECK(dw.size(3) == C && dy.size(3) == K && dy.size(0) == N, "wgrad shape mismatch");
  TORCH_CHECK(dtg::conv_supported(C, K, R, S, stride, pad, 2), "wgrad shape not supported by the HIP kernel");
  const int sw = stride_w > 0 ? (int)stride_w : (int)stride;
  const int P = (H + 2 * pad - R) / stride + 1, Q = (W + 2 * pad - S) / sw + 1;
  TORCH_CHECK(dy.size(1) == P && dy.size(2) == Q, "wgrad geometry mismatch");
  c10::DeviceGuard dg(x.device());
  const int split = dtg::conv_wgrad_split(N, H, W, C, K, R, S, stride, pad, sw, (int)target_wgs);
  auto ws = at::empty({(long long)split * K * R * S * C}, x.options().dtype(at::kFloat));
  dtg::conv_wgrad(cbfp(dy), cbfp(x), dw.data_ptr(), dw.scalar_type() == at::kBFloat16, (float)beta,
                  ws.data_ptr<float>(), split, N, H, W, C, K, R, S, stride, pad, cur_stream(), sw, (int)sched);
}

}  // namespace

void register_transformer_ops(pybind11::module_& m);  // transformer_ops.cc
void register_pool_ops(pybind11::module_& m);         // pool_ops.cc
void register_data_ops(pybind11::module_& m);         // data_ops.cc
void register_eval_ops(pybind11::module_& m);         // eval_ops.cc
void register_mlm_ops(pybind11::module_& m);          // mlm_ops.cc
void register_seqpack_ops(pybind11::module_& m);      // seqpack_ops.cc

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("conv_supported", &conv_supported);
  m.def("conv_fwd", &conv_fwd);
  m.def("conv_dgrad", &conv_dgrad, pybind11::arg("dy"), pybind11::arg("w"), pybind11::arg("H"), pybind11::arg("W"),
        pybind11::arg("stride"), pybind11::arg("pad"), pybind11::arg("out") = pybind11::none(),
        pybind11::arg("beta") = 0.0, pybind11::arg("zero_rest") = true);
  m.def("conv_wgrad", &conv_wgrad, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("dw"),
        pybind11::arg("beta"), pybind11::arg("stride"), pybind11::arg("pad"), pybind11::arg("stride_w") = 0,
        pybind11::arg("target_wgs") = 0, pybind11::arg("sched") = 0);
  m.def("gemm_bn", &gemm_bn, pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("mode"),
        pybind11::arg("x") = pybind11::none(), pybind11::arg("mean") = pybind11::none(),
        pybind11::arg("invstd") = pybind11::none(), pybind11::arg("gamma") = pybind11::none(),
        pybind11::arg("beta") = pybind11::none(), pybind11::arg("mask") = pybind11::none(),
        pybind11::arg("out") = pybind11::none(), pybind11::arg("pooled") = false,
        pybind11::arg("x2") = pybind11::none(), pybind11::arg("mean2") = pybind11::none(),
        pybind11::arg("invstd2") = pybind11::none(), pybind11::arg("part2") = pybind11::none(),
        pybind11::arg("sub2_hw") = pybind11::none());
  m.def("bn_part_alloc", [](Tensor like, int64_t C, bool pooled) { return bn_part(like, C, pooled); },
        pybind11::arg("like"), pybind11::arg("C"), pybind11::arg("pooled") = false);
  m.def("bn_bwd2_part", &bn_bwd2_part, pybind11::arg("dp"), pybind11::arg("x"), pybind11::arg("part"),
        pybind11::arg("gamma"), pybind11::arg("smean"), pybind11::arg("sinv"), pybind11::arg("dgamma"),
        pybind11::arg("dbeta"), pybind11::arg("x2"), pybind11::arg("part2"), pybind11::arg("gamma2"),
        pybind11::arg("smean2"), pybind11::arg("sinv2"), pybind11::arg("dgamma2"), pybind11::arg("dbeta2"),
        pybind11::arg("wact") = pybind11::none(), pybind11::arg("wgrad") = pybind11::none(),
        pybind11::arg("wact2") = pybind11::none(), pybind11::arg("wgrad2") = pybind11::none(),
        pybind11::arg("dgw") = pybind11::none(), pybind11::arg("dgy") = pybind11::none(),
        pybind11::arg("dgmean") = pybind11::none(), pybind11::arg("dginv") = pybind11::none(),
        pybind11::arg("dgbits") = pybind11::none(), pybind11::arg("dgpart") = pybind11::none(),
        pybind11::arg("dgfull") = false, pybind11::arg("dgx") = false);
  m.def("bn_dx_wgrad_ok", [](int64_t M, int64_t C, int64_t CI) { return dtg::bn_dx_wgrad_ok(M, (int)C, (int)CI); });
  m.def("bn_dx_dgrad_ok", [](int64_t M, int64_t C, int64_t CI) { return dtg::bn_dx_dgrad_ok(M, (int)C, (int)CI); });
  m.def("bn_dx_dgrad_full_ok",
        [](int64_t M, int64_t C, int64_t CI) { return dtg::bn_dx_dgrad_full_ok(M, (int)C, (int)CI); });
  // the dx pass can form x again from wact and dgw instead of reading it (dgx)
  m.def("bn_dx_recompute_ok",
        [](int64_t M, int64_t C, int64_t CI, bool dual) { return dtg::bn_dx_recompute_ok(M, (int)C, (int)CI, dual); },
        pybind11::arg("M"), pybind11::arg("C"), pybind11::arg("CI"), pybind11::arg("dual") = false);
  // workgroups of the fused dx pass per channel slice (= its fp32 slabs): the grid its row blocks are dealt over
  m.def("bn_dx_wgrad_slabs",
        [](int64_t C, int64_t CI, int64_t w2, bool dg) { return dtg::bn_dx_wgrad_slabs((int)C, (int)CI, (int)w2, dg); },
        pybind11::arg("C"), pybind11::arg("CI"), pybind11::arg("w2") = 0, pybind11::arg("dg") = false);
  m.def("conv_fwd_bn", &conv_fwd_bn, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("stride"),
        pybind11::arg("pad"), pybind11::arg("pooled") = false);
  m.def("conv_dgrad_bn", &conv_dgrad_bn, pybind11::arg("dy"), pybind11::arg("w"), pybind11::arg("H"),
        pybind11::arg("W"), pybind11::arg("stride"), pybind11::arg("pad"), pybind11::arg("x"), pybind11::arg("mean"),
        pybind11::arg("invstd"), pybind11::arg("gamma"), pybind11::arg("beta"), pybind11::arg("pooled") = false,
        pybind11::arg("bits") = pybind11::none());
  m.def("bn_fwd2_part", &bn_fwd2_part, pybind11::arg("x"), pybind11::arg("part"), pybind11::arg("gamma"),
        pybind11::arg("beta"), pybind11::arg("rmean"), pybind11::arg("rvar"), pybind11::arg("r"), pybind11::arg("part2"),
        pybind11::arg("gamma2"), pybind11::arg("beta2"), pybind11::arg("rmean2"), pybind11::arg("rvar2"),
        pybind11::arg("momentum"), pybind11::arg("eps"), pybind11::arg("bits") = pybind11::none(),
        pybind11::arg("next_w") = pybind11::none(), pybind11::arg("next_part") = pybind11::none());
  m.def("bn_apply_gemm_ok", [](int64_t M, int64_t C, int64_t N) { return dtg::bn_apply_gemm_ok(M, (int)C, (int)N); });
  // workgroups of the apply pass that also computes the next conv1: the grid its 32-row blocks are dealt over
  m.def("bn_apply_gemm_grid",
        [](int64_t C, int64_t N, bool two) { return dtg::bn_apply_gemm_grid((int)C, (int)N, two); },
        pybind11::arg("C"), pybind11::arg("N"), pybind11::arg("two") = false);
  m.def("conv_fwd_c8", &conv_fwd_c8, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("R"), pybind11::arg("S"),
        pybind11::arg("stride"), pybind11::arg("pad"), pybind11::arg("with_stats") = false,
        pybind11::arg("stride_w") = 0);
  m.def("bn_fwd_part", &bn_fwd_part, pybind11::arg("x"), pybind11::arg("part"), pybind11::arg("res"),
        pybind11::arg("gamma"), pybind11::arg("beta"), pybind11::arg("rmean"), pybind11::arg("rvar"),
        pybind11::arg("momentum"), pybind11::arg("eps"), pybind11::arg("relu"), pybind11::arg("bits") = pybind11::none(),
        pybind11::arg("next_w") = pybind11::none(), pybind11::arg("next_part") = pybind11::none());
  m.def("bn_bwd_part", &bn_bwd_part, pybind11::arg("dp"), pybind11::arg("x"), pybind11::arg("part"),
        pybind11::arg("gamma"), pybind11::arg("smean"), pybind11::arg("sinv"), pybind11::arg("want_dres"),
        pybind11::arg("dgamma_acc") = pybind11::none(), pybind11::arg("dbeta_acc") = pybind11::none(),
        pybind11::arg("wact") = pybind11::none(), pybind11::arg("wgrad") = pybind11::none(),
        pybind11::arg("dgw") = pybind11::none(), pybind11::arg("dgy") = pybind11::none(),
        pybind11::arg("dgmean") = pybind11::none(), pybind11::arg("dginv") = pybind11::none(),
        pybind11::arg("dgbits") = pybind11::none(), pybind11::arg("dgpart") = pybind11::none(),
        pybind11::arg("dgfull") = false, pybind11::arg("dgx") = false);
  m.doc() = "dtg gfx950 HIP kernels";
  {
    namespace py = pybind11;
    // clip: an optional device scalar multiplied into gscale (the global-norm clip factor); absent = today's launch
    m.def("sgd_apply", &sgd_apply, py::arg("w"), py::arg("mirror"), py::arg("g"), py::arg("hyper"), py::arg("wd"),
          py::arg("gscale"), py::arg("zero_grad"), py::arg("clip") = py::none());
    m.def("momentum_apply", &momentum_apply, py::arg("w"), py::arg("mirror"), py::arg("g"), py::arg("mom"),
          py::arg("hyper"), py::arg("mu"), py::arg("wd"), py::arg("nesterov"), py::arg("gscale"), py::arg("zero_grad"),
          py::arg("clip") = py::none());
    m.def("adagrad_apply", &adagrad_apply, py::arg("w"), py::arg("mirror"), py::arg("g"), py::arg("acc"),
          py::arg("hyper"), py::arg("eps"), py::arg("gscale"), py::arg("zero_grad"), py::arg("clip") = py::none());
    m.def("adam_apply", &adam_apply, py::arg("w"), py::arg("mirror"), py::arg("g"), py::arg("m"), py::arg("v"),
          py::arg("hyper"), py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("wd"), py::arg("gscale"),
          py::arg("zero_grad"), py::arg("clip") = py::none());
  }
  m.attr("LW_CHUNK") = (int)dtg::kLwChunk;
  m.attr("LW_SERIAL") = (int)dtg::kLwSerial;
  m.attr("LW_TREE_DEPTH") = (int)dtg::kLwTreeDepth;
  m.def("lw_chunk_table", &lw_chunk_table);
  m.def("seg_sqnorm", &seg_sqnorm);
  m.def("lamb_moments", &lamb_moments);
  m.def("lamb_apply", &lamb_apply);
  m.def("lars_apply", &lars_apply);
  m.def("seg_finalize", &seg_finalize);
  m.def("axpby", &axpby);
  m.def("sgd_sum_apply", &sgd_sum_apply);
  m.def("momentum_sum_apply", &momentum_sum_apply);
  m.def("adagrad_sum_apply", &adagrad_sum_apply);
  m.def("adam_sum_apply", &adam_sum_apply);
  m.def("grad_sum", &grad_sum);
  m.def("grad_fold", &grad_fold);
  m.def("grad_unfold", &grad_unfold);
  m.def("state_chunk_table", &state_chunk_table);
  m.def("state_pack", &state_pack);
  m.def("state_unpack", &state_unpack);
  m.def("comm_spin", [](double seconds, int64_t wgs, int64_t lds_bytes) {
    dtg::comm_spin(seconds, (int)wgs, (int)lds_bytes, cur_stream());
  }, pybind11::arg("seconds"), pybind11::arg("wgs") = 32, pybind11::arg("lds_bytes") = 0);
  m.def("comm_emu", [](double seconds, int64_t wgs, int64_t mode, c10::optional<Tensor> scratch, int64_t base,
                       int64_t traffic_bytes, c10::optional<Tensor> bucket, double factor) {
    // scratch: a contiguous byte buffer (traffic mode); bucket: the contiguous fp32 / bf16 gradient slice (data mode)
    long long sbytes = 0, n = 0;
    int bf = 0;
    const Tensor* dev_t = nullptr;
    if (scratch.has_value() && scratch->defined()) {
      CHECK_IN(*scratch);
      TORCH_CHECK(((uintptr_t)scratch->data_ptr() % 16) == 0, "scratch: 16-B aligned");
      sbytes = scratch->numel() * scratch->element_size();
      dev_t = &*scratch;
    }
    if (bucket.has_value() && bucket->defined()) {
      CHECK_IN(*bucket);
      TORCH_CHECK(bucket->scalar_type() == at::kFloat || bucket->scalar_type() == at::kBFloat16, "bucket fp32/bf16");
      n = bucket->numel();
      bf = bucket->scalar_type() == at::kBFloat16;
      dev_t = &*bucket;
    }
    TORCH_CHECK(!(mode & 2) || sbytes > 0, "traffic mode needs scratch");
    TORCH_CHECK(!(mode & 4) || n > 0 || !(bucket.has_value() && bucket->defined()), "data mode needs the bucket");
    c10::optional<c10::DeviceGuard> dg;
    if (dev_t) dg.emplace(dev_t->device());
    return dtg::comm_emu(seconds, (int)wgs, (int)mode, sbytes ? scratch->data_ptr() : nullptr, sbytes, base,
                         traffic_bytes, n ? bucket->data_ptr() : nullptr, n, bf, (float)factor, cur_stream());
  }, pybind11::arg("seconds"), pybind11::arg("wgs") = 32, pybind11::arg("mode") = 0,
        pybind11::arg("scratch") = pybind11::none(), pybind11::arg("base") = 0, pybind11::arg("traffic_bytes") = 0,
        pybind11::arg("bucket") = pybind11::none(), pybind11::arg("factor") = 1.0);
  m.def("stem_stream_set", [](int64_t on) { dtg::stem_stream_set((int)on); });
  m.def("gemm_expand_k256_set", [](int64_t on) { dtg::gemm_expand_k256_set((int)on); });
  m.def("stem_pool_rows_set", [](int64_t on) { dtg::stem_pool_rows_set((int)on); });
  m.def("gemm_expand_s2_set", [](int64_t on) { dtg::gemm_expand_s2_set((int)on); });
  m.def("conv_halo_fwd_set", [](int64_t on) { dtg::conv3x3_halo_fwd_set((int)on); });
  m.def("conv_halo_dgrad_set", [](int64_t on) { dtg::conv3x3_halo_dgrad_set((int)on); });
  m.def("conv_halo_wgrad_set", [](int64_t on) { dtg::conv3x3_halo_wgrad_set((int)on); });
  m.def("conv_lin_wgrad_set", [](int64_t on) { dtg::conv3x3_lin_wgrad_set((int)on); });
  m.def("hyper_tick", [](Tensor hyper) {
    check_hyper(hyper);
    c10::DeviceGuard dg(hyper.device());
    dtg::hyper_tick(hyper.data_ptr<float>(), cur_stream());
  });
  m.def("stem_pack_weights", [](Tensor w) {
    CHECK_CUDA(w);
    CHECK_DT(w, at::kBFloat16);
    TORCH_CHECK(w.dim() == 4 && w.is_contiguous(at::MemoryFormat::ChannelsLast) && w.size(1) <= 4,
                "w: channels_last [K, C<=4, R, S]");
    const int K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3), S2 = (S + 1) / 2;
    const int KP = (R * S2 * 8 + 63) / 64 * 64;
    c10::DeviceGuard dg(w.device());
    auto wp = at::empty({K, KP}, w.options().memory_format(at::MemoryFormat::Contiguous));
    dtg::stem_pack_weights(cbfp(w), bfp(wp), K, C, R, S, S2, KP, cur_stream());
    return wp;
  });
  m.def("stem_dw_add", [](Tensor src, Tensor grad, bool pair) {
    // src [K, R, S2, 8] fp32 (pair) or [K, R, S, 8]; grad: the channels_last [K, C, R, S] parameter gradient
    CHECK_IN(src);
    CHECK_DT(src, at::kFloat);
    CHECK_CUDA(grad);
    TORCH_CHECK(grad.dim() == 4 && grad.is_contiguous(at::MemoryFormat::ChannelsLast), "grad: channels_last [K,C,R,S]");
    TORCH_CHECK(grad.scalar_type() == at::kFloat || grad.scalar_type() == at::kBFloat16, "grad fp32/bf16");
    const int K = grad.size(0), C = grad.size(1), R = grad.size(2), S = grad.size(3);
    TORCH_CHECK(src.dim() == 4 && src.size(0) == K && src.size(1) == R && src.size(3) == 8 && C <= 4 &&
                    src.size(2) == (pair ? (S + 1) / 2 : S), "stem dw source shape");
    c10::DeviceGuard dg(grad.device());
    dtg::stem_dw_add(src.data_ptr<float>(), grad.data_ptr(), grad.scalar_type() == at::kBFloat16, K, R, S, C,
                     (int)src.size(2), pair ? 1 : 0, cur_stream());
  });
  m.def("stream_probe", [](int64_t kind, Tensor a, c10::optional<Tensor> b, c10::optional<Tensor> o, Tensor sink,
                           int64_t wgs, int64_t unroll, bool nt) {
    // a / b / o: contiguous GPU buffers of equal byte size (a multiple of 16); sink: int32 [>= wgs]
    CHECK_IN(a);
    CHECK_IN(sink);
    TORCH_CHECK(sink.scalar_type() == at::kInt && sink.numel() >= wgs, "sink: int32 with >= wgs elements");
    const long long bytes = a.numel() * a.element_size();
    TORCH_CHECK(bytes % 16 == 0 && ((uintptr_t)a.data_ptr() % 16) == 0, "a: 16-B multiple, 16-B aligned");
    for (const auto* t : {&b, &o})
      if (t->has_value() && (*t)->defined()) {
        CHECK_IN(**t);
        TORCH_CHECK((*t)->numel() * (*t)->element_size() == bytes && ((uintptr_t)(*t)->data_ptr() % 16) == 0,
                    "b / o: the byte size of a, 16-B aligned");
      }
    TORCH_CHECK(kind >= 0 && kind <= 3, "kind 0..3");
    TORCH_CHECK(kind == 0 || (o.has_value() && o->defined()), "kinds 1-3 write o");
    TORCH_CHECK(kind != 3 || (b.has_value() && b->defined()), "kind 3 reads b");
    TORCH_CHECK(wgs >= 1 && wgs <= 65536, "wgs");
    c10::DeviceGuard dg(a.device());
    dtg::stream_probe((int)kind, a.data_ptr(), opt_ptr<void>(b), opt_ptr<void>(o), bytes / 16,
                      reinterpret_cast<unsigned*>(sink.data_ptr()), (int)wgs, (int)unroll, nt ? 1 : 0, cur_stream());
  }, pybind11::arg("kind"), pybind11::arg("a"), pybind11::arg("b") = pybind11::none(),
        pybind11::arg("o") = pybind11::none(), pybind11::arg("sink"), pybind11::arg("wgs") = 1024,
        pybind11::arg("unroll") = 4, pybind11::arg("nt") = false);
  m.def("launch_probe", [](int64_t grid, int64_t lds_bytes) {
    dtg::launch_probe((int)grid, (int)lds_bytes, cur_stream());
  });
  m.def("f32_to_bf16", &f32_to_bf16);
  m.def("bn_fwd_train", &bn_fwd_train);
  m.def("bn_fwd_infer", &bn_fwd_infer);
  m.def("bn_bwd", &bn_bwd, pybind11::arg("dy"), pybind11::arg("y"), pybind11::arg("x"), pybind11::arg("gamma"),
        pybind11::arg("smean"), pybind11::arg("sinv"), pybind11::arg("relu"), pybind11::arg("want_dres"),
        pybind11::arg("dgamma_acc") = pybind11::none(), pybind11::arg("dbeta_acc") = pybind11::none());
  m.def("softmax_xent", &softmax_xent);
  m.def("gemm_bn_force_cfg", [](int64_t c) { dtg::gemm_bn_force_cfg((int)c); });
  m.def("conv_force_tile", [](int64_t which, int64_t c) { dtg::conv_force_tile((int)which, (int)c); });
  m.def("conv_set_stages", [](int64_t which, int64_t s) { dtg::conv_set_stages((int)which, (int)s); });
  m.def("softmax_xent_bwd", &softmax_xent_bwd);
  m.def("gemm_pick_split", [](int64_t M, int64_t N, int64_t K, bool a_kc, int64_t target_wgs) {
    return dtg::gemm_pick_split((int)M, (int)N, (int)K, a_kc ? 1 : 0, (int)target_wgs);
  }, pybind11::arg("M"), pybind11::arg("N"), pybind11::arg("K"), pybind11::arg("a_kc") = false,
        pybind11::arg("target_wgs") = 0);
  m.def("gemm", &gemm, pybind11::arg("A"), pybind11::arg("a_kc"), pybind11::arg("B"), pybind11::arg("b_kc"),
        pybind11::arg("out"), pybind11::arg("alpha") = 1.0, pybind11::arg("beta") = 0.0,
        pybind11::arg("bias") = pybind11::none(), pybind11::arg("act") = 0, pybind11::arg("split_k") = 0,
        pybind11::arg("aux") = pybind11::none(), pybind11::arg("aux_mode") = 0,
        pybind11::arg("colsum") = pybind11::none());
  register_transformer_ops(m);
  register_pool_ops(m);
  register_data_ops(m);
  register_eval_ops(m);
  register_mlm_ops(m);
  register_seqpack_ops(m);
}
