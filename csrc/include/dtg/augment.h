// Launcher of the input-pipeline kernel (csrc/kernels/augment.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dtg {

constexpr int kAugMaxSide = 8192;  // H, W <= this: (cw << 16) and every product below it stay inside 32 bits

// raw u8 [N,H,W,3], params i32 [N,5] = (x0, y0, cw, ch, flip) -> out bf16 [N,S,S,3]:
// random-resized-crop by 8.8 fixed-point bilinear weights, flip, per-channel affine, cast.  grid <= 0: heuristic.
void crop_resize_norm(const uint8_t* raw, const int* params, unsigned short* out, const float* scale,
                      const float* shift, int N, int H, int W, int S, int grid, hipStream_t st);

}  // namespace dtg
