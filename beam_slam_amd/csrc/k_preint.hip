// IMU pre-integration for a batch of keyframe intervals — the factor producer on the input side of the solve
// (SURVEY.md §8f rank 4).  Restates bs_common::PreIntegrator (bs_common/src/bs_common/preintegrator.cpp); the recursion of one
// interval is preint_core.h, shared with the CPU tests.
// One lane per interval: an interval is a strictly sequential recursion over its samples (20 at 200 Hz / 10 Hz),
// a window has a few hundred intervals, so this is latency work — it is here to keep the IMU samples and the
// factor constants on the device, not for throughput.
#include "bsgpu_device.h"
#include "preint_core.h"

namespace bsg {

__global__ __launch_bounds__(64) void preintegrate_kernel(int n_int, const int* __restrict__ sample_start, const double* __restrict__ ts,
                                                          const double* __restrict__ wm, const double* __restrict__ am,
                                                          const double* __restrict__ t_end, const double* __restrict__ bgs,
                                                          const double* __restrict__ bas, const double* __restrict__ covs /* cov_w, cov_a, cov_bg, cov_ba: 4 x 9 */,
                                                          double info_weight, double* __restrict__ out /* n_int x 287 */) {
  const int iv = blockIdx.x * 64 + threadIdx.x;
  if (iv >= n_int) return;
  preintegrate_interval(sample_start[iv], sample_start[iv + 1], ts, wm, am, t_end[iv], bgs + 3 * iv, bas + 3 * iv, covs, info_weight,
                        out + (size_t)iv * kPreintOut);
}

void launch_preintegrate(hipStream_t s, int n_int, const int* sample_start, const double* ts, const double* wm, const double* am,
                         const double* t_end, const double* bg, const double* ba, const double* covs, double info_weight, double* out) {
  if (n_int > 0)
    hipLaunchKernelGGL(preintegrate_kernel, dim3((n_int + 63) / 64), dim3(64), 0, s, n_int, sample_start, ts, wm, am, t_end, bg, ba, covs,
                       info_weight, out);
}

}  // namespace bsg
