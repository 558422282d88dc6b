// Host gather of the input pipeline: N memcpys of row_bytes from N source addresses into one contiguous destination,
// on a few short-lived threads with the GIL released.  The addresses are computed in Python from validated record
// indices (base[shard] + local * row_bytes, dtg/data/loader.py); nothing here touches the GPU.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <vector>

namespace py = pybind11;

namespace dtg {

void gather_rows_raw(uint8_t* dst, const int64_t* src, int64_t n, int64_t row_bytes, int nthreads) {
  auto work = [=](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i)
      memcpy(dst + i * row_bytes, reinterpret_cast<const void*>(static_cast<uintptr_t>(src[i])), (size_t)row_bytes);
  };
  const int64_t nt = std::max<int64_t>(1, std::min<int64_t>(nthreads, n));
  if (nt == 1) {
    work(0, n);
    return;
  }
  const int64_t per = (n + nt - 1) / nt;
  std::vector<std::thread> pool;
  pool.reserve((size_t)nt - 1);
  for (int64_t t = 1; t < nt; ++t)
    if (t * per < n) pool.emplace_back(work, t * per, std::min(n, (t + 1) * per));
  work(0, std::min(n, per));
  for (auto& th : pool) th.join();
}

}  // namespace dtg

void register_gather(py::module_& m) {
  m.def(
      "gather_rows",
      [](uintptr_t dst, py::array_t<int64_t, py::array::c_style> src, int64_t row_bytes, int nthreads) {
        if (src.ndim() != 1) throw std::invalid_argument("gather_rows: src_addresses must be a 1-D int64 array");
        if (row_bytes < 0 || nthreads < 1 || nthreads > 64)
          throw std::invalid_argument("gather_rows: row_bytes >= 0 and 1 <= nthreads <= 64 required");
        const int64_t n = src.shape(0);
        if (n == 0 || row_bytes == 0) return;
        if (dst == 0) throw std::invalid_argument("gather_rows: null destination");
        const int64_t* s = src.data();
        for (int64_t i = 0; i < n; ++i)
          if (s[i] == 0) throw std::invalid_argument("gather_rows: null source address");
        py::gil_scoped_release nogil;
        dtg::gather_rows_raw(reinterpret_cast<uint8_t*>(dst), s, n, row_bytes, nthreads);
      },
      py::arg("dst_address"), py::arg("src_addresses"), py::arg("row_bytes"), py::arg("nthreads") = 4,
      "N memcpys of row_bytes from src_addresses[i] to dst_address + i * row_bytes, GIL released");
}
