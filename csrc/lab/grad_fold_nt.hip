// The non-temporal-store form of grad_fold (dtg/grad_fold.cuh), for the A/B of tools/bench_accum.py.
#include "dtg/grad_fold.cuh"
#include "lab_api.h"

namespace dtg {

void grad_fold_nt(float* acc, void* g, int g_bf16, long long n, int first, hipStream_t st) {
  launch_grad_fold<true>(acc, g, g_bf16, n, first, st);
}

}  // namespace dtg
