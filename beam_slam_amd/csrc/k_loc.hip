// Frame localisation for a batch of frames (bsgpu_localize_frames): VisualOdometry::LocalizeFrame's pose refinement
// (bs_models/src/visual_odometry.cpp:217-300) and ComputeAverageReprojection (:1247-1272), frame_lm.h's loop on the device.
//
// One launch, one 256-thread workgroup per frame, every LM iteration inside the kernel: a frame's whole normal system is 6x6, so an
// evaluation is a pass over its observations (strided over the lanes, 28 running sums per lane) and one block reduction — within each
// wave by cross-lane butterflies, across the four waves through LDS in a fixed order — whose result every lane reads back.  The loop
// itself (Cholesky, decision, radius) runs redundantly in every lane on those identical sums.  Workgroups never wait on each other,
// and a frame's reduction order depends only on its own observation count: a frame's results are the same bits alone or in a batch.
#include "bsgpu_device.h"
#include "frame_lm.h"

namespace bsg {

namespace {

constexpr int kLocThreads = 256;
constexpr int kLocWaves = kLocThreads / 64;

// the K first sums over the workgroup; every lane receives the same bits
template <int K>
__device__ __forceinline__ void loc_block_sum(double* v, double* sred /* kLocWaves * kFlmSums */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sred[wave * kFlmSums + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ((sred[k] + sred[kFlmSums + k]) + sred[2 * kFlmSums + k]) + sred[3 * kFlmSums + k];
  __syncthreads();   // (the next reduction overwrites sred)
}

struct LocEval {
  int o0, o1;
  const double2* pix;
  const double* pts;      // 3 per observation, or
  const int* pt_off;      // ... the offset of the observation's landmark block in x
  const double* x;
  DevCamera cam;
  int loss_kind;
  double loss_a, w;
  int truncate;
  double* sred;

  __device__ __forceinline__ void point(int o, double P[3]) const {
    const double* src = pt_off ? x + pt_off[o] : pts + 3 * (size_t)o;
    P[0] = src[0]; P[1] = src[1]; P[2] = src[2];
  }
  __device__ __forceinline__ double2 pixel(int o) const {
    double2 z = pix[o];
    if (truncate) { z.x = trunc(z.x); z.y = trunc(z.y); }
    return z;
  }
  __device__ void operator()(const double q[4], const double t[3], bool with_J, FlmSums& s) const {
    for (int k = 0; k < kFlmSums; ++k) s.v[k] = 0.0;
    double R[9];
    flm_quat_to_rot(q, R);
    for (int o = o0 + (int)threadIdx.x; o < o1; o += kLocThreads) {
      double P[3];
      point(o, P);
      const double2 z = pixel(o);
      flm_obs_accum(cam, R, t, P, z.x, z.y, w, loss_kind, loss_a, with_J, s);
    }
    if (with_J) loc_block_sum<kFlmSums>(s.v, sred);
    else loc_block_sum<1>(s.v, sred);
  }
};

__global__ void __launch_bounds__(kLocThreads) localize_kernel(const int* __restrict__ obs_start, const double2* __restrict__ pix,
                                                               const double* __restrict__ pts, const int* __restrict__ pt_off,
                                                               const double* __restrict__ x, const DevCamera* __restrict__ cams,
                                                               const int* __restrict__ cam_of, const double* __restrict__ pose_in,
                                                               int loss_kind, double loss_a, double sqrt_info, int truncate, int min_points,
                                                               int width, int height, const bsgpu_options opt, double* __restrict__ out,
                                                               int* __restrict__ out_i) {
  __shared__ double sred[kLocWaves * kFlmSums];
  const int f = blockIdx.x;
  LocEval ev;
  ev.o0 = obs_start[f]; ev.o1 = obs_start[f + 1];
  ev.pix = pix; ev.pts = pts; ev.pt_off = pt_off; ev.x = x;
  ev.cam = cams[cam_of[f]];
  ev.loss_kind = loss_kind; ev.loss_a = loss_a; ev.w = sqrt_info; ev.truncate = truncate;
  ev.sred = sred;
  const double q0[4] = {pose_in[7 * f], pose_in[7 * f + 1], pose_in[7 * f + 2], pose_in[7 * f + 3]};
  const double p0[3] = {pose_in[7 * f + 4], pose_in[7 * f + 5], pose_in[7 * f + 6]};
  FlmResult res;
  flm_localize(opt, ev.o1 - ev.o0, min_points, q0, p0, ev, res);
  // ComputeAverageReprojection at the returned pose: the in-image errors over ALL of the frame's pairs
  double R[9];
  flm_quat_to_rot(res.q, R);
  double e[1] = {0.0};
  for (int o = ev.o0 + (int)threadIdx.x; o < ev.o1; o += kLocThreads) {
    double P[3];
    ev.point(o, P);
    const double2 z = ev.pixel(o);
    e[0] += flm_pixel_error(ev.cam, R, res.p, P, z.x, z.y, width, height);
  }
  loc_block_sum<1>(e, sred);
  // [q 4 | p 3 | cost | avg | cov 36] per frame, by lane 0 (every lane holds the same values; constant indices keep them in registers)
  if (threadIdx.x == 0) {
    double* of = out + (size_t)kLocOutStride * f;
    const int n = ev.o1 - ev.o0;
#pragma unroll
    for (int i = 0; i < 4; ++i) of[i] = res.q[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) of[4 + i] = res.p[i];
    of[7] = res.cost;
    of[8] = n > 0 ? e[0] / (double)n : 0.0;
#pragma unroll
    for (int i = 0; i < 36; ++i) of[9 + i] = res.cov[i];
    out_i[2 * f] = res.iterations;
    out_i[2 * f + 1] = res.status;
  }
}

}  // namespace

void launch_localize(hipStream_t s, int n_frames, const int* obs_start, const double2* pix, const double* pts, const int* pt_off,
                     const double* x, const DevCamera* cams, const int* cam_of, const double* pose_in, int loss_kind, double loss_a,
                     double sqrt_info, int truncate, int min_points, int width, int height, const bsgpu_options& opt, double* out,
                     int* out_i) {
  if (n_frames <= 0) return;
  hipLaunchKernelGGL(localize_kernel, dim3(n_frames), dim3(kLocThreads), 0, s, obs_start, pix, pts, pt_off, x, cams, cam_of, pose_in,
                     loss_kind, loss_a, sqrt_info, truncate, min_points, width, height, opt, out, out_i);
}

}  // namespace bsg
