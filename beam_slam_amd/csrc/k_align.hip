// Visual-inertial alignment for a batch of candidate paths (bsgpu_inertial_alignment) — the link between the up-to-scale camera path
// and the first large solve of SLAMInitialization: imu::EstimateParameters (bs_models/src/lib/imu/inertial_alignment.cpp:4-202), the
// scale gate and AlignPathAndVelocities (bs_models/src/slam_initialization.cpp:312-316, :400-431).  The steps of one path are
// inertial_align.h, shared with the CPU tests.
// One workgroup of one wave per path, blockIdx.x = path; in the per-frame steps a lane per frame (a loop when the path has more
// frames than lanes), the sums over frames and the least-squares chain on lane 0 in frame order — a path's bits depend neither on
// its neighbours nor on the launch shape.  A frame's delta is a strictly sequential recursion over its samples (20 at 200 Hz /
// 10 Hz) and frame 0's interval — everything before the first pose — is the straggler; it stays serial, because composing partial
// deltas would change bits.  Like k_preint.hip this is latency work: it keeps the whole initialisation behind one boundary.
#include "bsgpu_device.h"
#include "inertial_align.h"

namespace bsg {

struct AlignWorkgroup {
  __device__ __forceinline__ int any(int x) const { return __syncthreads_or(x); }
  __device__ __forceinline__ void barrier() const { __syncthreads(); }
};

__global__ __launch_bounds__(64) void inertial_alignment_kernel(
    const int* frame_start, const double* t_frame, const double* q_frame, const double* p_frame, const int* imu_range, const double* t,
    const double* w, const double* a, int bridge_gap, double min_excitation, int apply_scale, double scale_min, double scale_max,
    double rank_tol, double* gravity, double* bg, double* scale, double* excitation, int* gyro_rank, double* velocity, double* q_out,
    double* p_out, double* v_out, int* status, int* own, double* fs, double* ps) {
  __shared__ double ws[kAlignWork];          // lane 0's block of the least-squares sweep: indexed by row and column at run time
  align_path_of_call((int)blockIdx.x, frame_start, t_frame, q_frame, p_frame, imu_range, t, w, a, bridge_gap, min_excitation, apply_scale,
                     scale_min, scale_max, rank_tol, gravity, bg, scale, excitation, gyro_rank, velocity, q_out, p_out, v_out, status, own,
                     fs, ps, ws, (int)threadIdx.x, 64, AlignWorkgroup{});
}

void launch_inertial_alignment(hipStream_t s, int n_paths, const int* frame_start, const double* t_frame, const double* q_frame,
                               const double* p_frame, const int* imu_range, const double* t, const double* w, const double* a,
                               int bridge_gap, double min_excitation, int apply_scale, double scale_min, double scale_max, double rank_tol,
                               double* gravity, double* bg, double* scale, double* excitation, int* gyro_rank, double* velocity,
                               double* q_out, double* p_out, double* v_out, int* status, int* own, double* fs, double* ps) {
  if (n_paths > 0)
    hipLaunchKernelGGL(inertial_alignment_kernel, dim3(n_paths), dim3(64), 0, s, frame_start, t_frame, q_frame, p_frame, imu_range, t, w, a,
                       bridge_gap, min_excitation, apply_scale, scale_min, scale_max, rank_tol, gravity, bg, scale, excitation, gyro_rank,
                       velocity, q_out, p_out, v_out, status, own, fs, ps);
}

}  // namespace bsg
