// Input pipeline, device side: random-resized-crop + flip + normalize + cast in one launch per batch.
//
//   raw u8 [N,H,W,3], params i32 [N,5] = (x0, y0, cw, ch, flip)  ->  out bf16 [N,S,S,3] (channels_last [N,3,S,S])
//
// The arithmetic is integer up to the last two fp32 operations, so dtg/ops/augment.py::crop_resize_norm_ref
// reproduces it bit for bit:
//   step = (c << 16) / S;  u = o * step + (step >> 1) - 32768, clamped to [0, (c - 1) << 16];
//   i = u >> 16, f = (u >> 8) & 255, i1 = min(i + 1, c - 1)                        (columns and rows alike)
//   p = (a*(256-fx) + b*fx) * (256-fy) + (c*(256-fx) + d*fx) * fy                   (<= 255 * 65536: exact in fp32)
//   out = bf16_rne(float(p) * scale[ch] + shift[ch])                               (multiply and add rounded apart)
//
// Structure: a workgroup of `wpb` waves takes `wpb` adjacent output rows of one image; a wave owns one output row, so
// the parameter row and the row's (iy, iy1, fy) are wave-uniform.  Each wave brings its two source row segments
// [x0, x0 + cw) x 3 bytes into its own LDS rows with coalesced aligned 16-byte loads (source rows are not even 4-byte
// aligned in general: W * 3 is odd for odd W) and gathers the four taps of a pixel from LDS.  A lane produces 8
// adjacent output pixels (48 bytes, three 16-byte stores) when S % 8 == 0 and `out` is 16-byte aligned; any other
// S takes the scalar path.  Parameters are made and validated on the host (dtg/data/augment_params.py), and every
// coordinate is clamped into the image again here, so no parameter table can make the kernel read outside `raw`.
#include "dtg/augment.h"
#include "dtg/common.h"

namespace dtg {
namespace {

constexpr int kAugWaves = 4;           // waves per workgroup when the rows fit
constexpr int kAugLdsBudget = 65536;   // bytes of LDS one workgroup may ask for

inline int aug_rowbuf(int W) { return ((W * 3 + 15) & ~15) + 32; }  // one staged row: segment + both alignment slacks

// Multiply and add with one rounding each, as the mirror's two eager ops.  The kernels are built with
// -ffp-contract=fast, which lets the backend fuse a * b + c whatever the source says: `#pragma clang fp contract(off)`
// and __fmul_rn / __fadd_rn (plain * and + in this HIP) are both ignored, and the fused result differs from the mirror
// wherever the unfused sum lands on a bf16 rounding tie (about one output in 4000 near zero).  The empty asm makes the
// product opaque, so there is nothing left to fuse.  (Check the ISA of a one-step compile: -save-temps compiles in
// phases and does not fuse.)
__device__ __forceinline__ float affine_rn(float p, float s, float b) {
  float m = p * s;
  asm volatile("" : "+v"(m));
  return m + b;
}

// Bytes [off, off + len) of raw -> LDS, as whole aligned 16-byte vectors around them; byte off lands at
// dst[lead], lead = the segment's misalignment (returned).  A vector that is not wholly inside [raw, raw + total)
// is put together from guarded byte loads (bytes outside read as 0), so nothing outside the tensor is touched.
__device__ __forceinline__ int stage_row(const uint8_t* __restrict__ raw, long long total, long long off, int len,
                                         uint8_t* dst, int lane) {
  const int lead = (int)((uintptr_t)(raw + off) & 15);
  const int nvec = (lead + len + 15) >> 4;
  const long long rel0 = off - lead;
  for (int v = lane; v < nvec; v += kWave) {
    const long long rel = rel0 + 16LL * v;
    uint4 q;
    if (rel >= 0 && rel + 16 <= total) {
      q = *reinterpret_cast<const uint4*>(raw + rel);
    } else {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const long long r = rel + b;
        if (r >= 0 && r < total) w[b >> 2] |= (uint32_t)raw[r] << (8 * (b & 3));
      }
      q = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(dst + 16 * v) = q;
  }
  return lead;
}

struct AugRow {          // wave-uniform state of one output row
  const uint8_t* top;    // LDS: byte 0 of source row iy's segment
  const uint8_t* bot;    // LDS: byte 0 of source row iy1's segment
  int step_x, cw, fy, flip, S;
  float sc[3], sh[3];
};

// output column ox -> its three normalized channels
__device__ __forceinline__ void aug_pixel(const AugRow& r, int ox, float (&o)[3]) {
  const int sx = r.flip ? r.S - 1 - ox : ox;
  int u = sx * r.step_x + (r.step_x >> 1) - 32768;
  u = min(max(u, 0), (r.cw - 1) << 16);
  const int ix = u >> 16, fx = (u >> 8) & 255, ix1 = min(ix + 1, r.cw - 1);
  const int gx = 256 - fx, gy = 256 - r.fy;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int a = r.top[ix * 3 + c], b = r.top[ix1 * 3 + c];
    const int e = r.bot[ix * 3 + c], d = r.bot[ix1 * 3 + c];
    const int p = (a * gx + b * fx) * gy + (e * gx + d * fx) * r.fy;
    o[c] = affine_rn((float)p, r.sc[c], r.sh[c]);
  }
}

__global__ void __launch_bounds__(kAugWaves * kWave)
crop_resize_norm_kernel(const uint8_t* __restrict__ raw, const int* __restrict__ params, bf16_t* __restrict__ out,
                        const float* __restrict__ scale, const float* __restrict__ shift, int N, int H, int W, int S,
                        int rowbuf, int vec) {
  extern __shared__ __attribute__((aligned(16))) uint8_t aug_lds[];
  const int wpb = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint8_t* const bufA = aug_lds + (size_t)wave * 2 * rowbuf;
  uint8_t* const bufB = bufA + rowbuf;
  const int groups = (S + wpb - 1) / wpb;
  const long long items = (long long)N * groups;
  const long long total = (long long)N * H * W * 3;
  AugRow r;
  r.S = S;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    r.sc[c] = scale[c];
    r.sh[c] = shift[c];
  }
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int n = (int)(it / groups);
    const int oy = (int)(it % groups) * wpb + wave;
    const bool live = oy < S;  // the last row group of an image may be short; dead waves only keep the barriers
    const int* p = params + (long long)n * 5;
    const int x0 = min(max(p[0], 0), W - 1), y0 = min(max(p[1], 0), H - 1);
    const int cw = min(max(p[2], 1), W - x0), ch = min(max(p[3], 1), H - y0);
    r.flip = p[4] != 0;
    r.cw = cw;
    r.step_x = (cw << 16) / S;
    const int step_y = (ch << 16) / S;
    if (live) {
      int v = oy * step_y + (step_y >> 1) - 32768;
      v = min(max(v, 0), (ch - 1) << 16);
      const int iy = v >> 16, iy1 = min(iy + 1, ch - 1);
      r.fy = (v >> 8) & 255;
      const long long rowbytes = (long long)W * 3;
      const long long off = ((long long)n * H + y0 + iy) * rowbytes + (long long)x0 * 3;
      r.top = bufA + stage_row(raw, total, off, cw * 3, bufA, lane);
      r.bot = r.top;
      if (iy1 != iy) r.bot = bufB + stage_row(raw, total, off + rowbytes, cw * 3, bufB, lane);
    }
    __syncthreads();
    if (live) {
      bf16_t* orow = out + ((long long)n * S + oy) * S * 3;
      if (vec) {
        for (int ox0 = lane * 8; ox0 < S; ox0 += kWave * 8) {
          uint32_t w[12];
#pragma unroll
          for (int j = 0; j < 8; j += 2) {
            float a[3], b[3];
            aug_pixel(r, ox0 + j, a);
            aug_pixel(r, ox0 + j + 1, b);
            w[(j >> 1) * 3 + 0] = pack_bf2(a[0], a[1]);
            w[(j >> 1) * 3 + 1] = pack_bf2(a[2], b[0]);
            w[(j >> 1) * 3 + 2] = pack_bf2(b[1], b[2]);
          }
          uint4* dst = reinterpret_cast<uint4*>(orow + (long long)ox0 * 3);
          dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
          dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
          dst[2] = make_uint4(w[8], w[9], w[10], w[11]);
        }
      } else {
        for (int ox = lane; ox < S; ox += kWave) {
          float a[3];
          aug_pixel(r, ox, a);
#pragma unroll
          for (int c = 0; c < 3; ++c) orow[(long long)ox * 3 + c] = f2bf(a[c]);
        }
      }
    }
    __syncthreads();  // the rows are overwritten by the next item
  }
}

}  // namespace

void crop_resize_norm(const uint8_t* raw, const int* params, bf16_t* out, const float* scale, const float* shift,
                      int N, int H, int W, int S, int grid, hipStream_t st) {
  if (N <= 0) return;
  const int rowbuf = aug_rowbuf(W);
  int wpb = kAugLdsBudget / (2 * rowbuf);  // W = 8192 still leaves room for one wave
  wpb = wpb > kAugWaves ? kAugWaves : wpb;
  const long long items = (long long)N * ((S + wpb - 1) / wpb);
  if (grid <= 0) grid = (int)(items < 8192 ? items : 8192);
  const int vec = (S % 8 == 0) && ((uintptr_t)out % 16 == 0);
  hipLaunchKernelGGL(crop_resize_norm_kernel, dim3(grid), dim3(wpb * kWave), (size_t)wpb * 2 * rowbuf, st, raw,
                     params, out, scale, shift, N, H, W, S, rowbuf, vec);
  DTG_LAUNCH_CHECK();
}

}  // namespace dtg
