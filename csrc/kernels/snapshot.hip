// Checkpoint snapshot of a flat parameter group (parallel/ps_ckpt.py, train/saver.py): state_pack copies the
// master and every optimizer slot of a group -- 1..4 fp32 buffers of one layout -- into a checkpoint IMAGE in
// ONE launch, state_unpack copies an image back.  The image has the flat buffer's offsets, but every parameter
// in LOGICAL order: a channels_last conv weight sits in the flat buffer as [O, kh, kw, I] and in the image as
// [O, I, kh, kw], so image[off : off + numel].reshape(p.shape) is the array a checkpoint stores for that key.
//
// The launch is table driven.  rows[p] = (offset, numel, I, RS) per parameter, RS = kh * kw; RS == 1 is an
// identity copy (1-D / 2-D parameters, contiguous 4-D ones, 1x1 convs: both orders coincide), otherwise
//   logical (o * I + i) * RS + r   <->   physical (o * RS + r) * I + i.
// chunks[c] = (row, chunk within the row), one per 2048 elements of a parameter, built on the host: a workgroup
// reads its chunk's row and never searches.  blockIdx.y is the source.  Alignment padding between parameters
// belongs to no chunk, so it is neither read nor written (pack leaves the image's zeros, unpack leaves what
// the optimizer put into a slot's padding).
//
// Identity rows move 16 bytes per lane access with a scalar tail.  Permuted rows walk the IMAGE side linearly
// (coalesced 4-byte accesses: stores for pack, loads for unpack) and gather / scatter the flat side with stride
// I; a chunk's 2048 logical elements cover the same ~2048-element physical span, so those lines are reused out
// of the caches by the same workgroup.
#include "dtg/common.h"
#include "dtg/kernels.h"

namespace dtg {

constexpr int kSnapChunk = 2048;  // elements per workgroup (= kStateChunk in kernels.h)
static_assert(kSnapChunk == kStateChunk, "chunk size mismatch");

template <bool PACK>
__global__ void __launch_bounds__(256) state_copy_kernel(StatePtrs flat, float* __restrict__ image, long long n,
                                                         const long long* __restrict__ rows,
                                                         const int* __restrict__ chunks) {
  const int j = blockIdx.y;
  // wave-uniform select over kernel arguments (a runtime index into the by-value struct would go through scratch)
  float* fbuf = j == 0 ? flat.p[0] : j == 1 ? flat.p[1] : j == 2 ? flat.p[2] : flat.p[3];
  float* img = image + (long long)j * n;
  const int row = chunks[2 * blockIdx.x];
  const int cin = chunks[2 * blockIdx.x + 1];
  const long long off = rows[4 * row];
  const int numel = (int)rows[4 * row + 1];
  const int I = (int)rows[4 * row + 2];
  const int RS = (int)rows[4 * row + 3];
  const int base = cin * kSnapChunk;
  float* f = fbuf + off;
  float* g = img + off;
  if (RS == 1) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = base + h * 1024 + threadIdx.x * 4;
      if (e + 4 <= numel) {
        if (PACK) *reinterpret_cast<float4*>(g + e) = *reinterpret_cast<const float4*>(f + e);
        else *reinterpret_cast<float4*>(f + e) = *reinterpret_cast<const float4*>(g + e);
      } else {
        for (int t = e; t < numel; ++t) {
          if (PACK) g[t] = f[t];
          else f[t] = g[t];
        }
      }
    }
  } else {
    float v[8];
    int ph[8];
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const int l = base + h * 256 + threadIdx.x;  // logical index
      const int oi = l / RS, r = l - oi * RS;
      const int o = oi / I, i = oi - o * I;
      ph[h] = (o * RS + r) * I + i;
      if (l < numel) v[h] = PACK ? f[ph[h]] : g[l];
    }
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const int l = base + h * 256 + threadIdx.x;
      if (l < numel) {
        if (PACK) g[l] = v[h];
        else f[ph[h]] = v[h];
      }
    }
  }
}

static void launch_state_copy(bool pack, const StatePtrs& flat, int k, float* image, long long n,
                              const long long* rows, const int* chunks, int n_chunks, hipStream_t st) {
  if (k < 1 || k > kMaxStateSrcs) throw std::runtime_error("dtg: state_pack / state_unpack take 1..4 buffers");
  if (n_chunks <= 0) return;
  const dim3 grid((unsigned)n_chunks, (unsigned)k);
  if (pack) state_copy_kernel<true><<<grid, 256, 0, st>>>(flat, image, n, rows, chunks);
  else state_copy_kernel<false><<<grid, 256, 0, st>>>(flat, image, n, rows, chunks);
  DTG_LAUNCH_CHECK();
}

void state_pack(const StatePtrs& src, int k, float* image, long long n, const long long* rows, const int* chunks,
                int n_chunks, hipStream_t st) {
  launch_state_copy(true, src, k, image, n, rows, chunks, n_chunks, st);
}

void state_unpack(const StatePtrs& dst, int k, const float* image, long long n, const long long* rows,
                  const int* chunks, int n_chunks, hipStream_t st) {
  launch_state_copy(false, dst, k, const_cast<float*>(image), n, rows, chunks, n_chunks, st);
}

}  // namespace dtg
