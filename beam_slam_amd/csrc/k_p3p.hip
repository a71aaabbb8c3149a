// P3P RANSAC frame poses for a batch of frames (bsgpu_absolute_pose_ransac): the
// beam_cv::AbsolutePoseEstimator::RANSACEstimator call of bs_models::vision::ComputePathWithVision
// (bs_models/src/lib/vision/utils.cpp:168), p3p.h's loop on the device.
//
// One launch, one 256-thread workgroup per frame, every RANSAC round inside the kernel.  A round evaluates kPpSamples = 64
// consecutive samples, one per group of 4 lanes.  Each lane of a group draws the sample and repeats the part of Lambda Twist its
// solutions share (bearings, the cubic's root, the two planes: a few hundred flops, cheaper than passing it round), then owns one of
// the up to four solutions: its depth triple, polish and pose in registers, its rank inside the group (ascending depth of the
// sample's first point) by shuffles.  The round's hypothesis table, 4 * sample + rank, is the only thing in LDS.
// All 256 threads then score every hypothesis of the round against the frame's pairs (a pair per thread, inlier counts by ballot
// and integer LDS atomics, so the counts do not depend on any order), and thread 0 applies the round's improving updates in sample
// order, ignoring the samples at or past the iteration bound then in force: the serial loop of the contract, whatever the round size.
// Workgroups never wait on each other: a frame's results are the same bits alone or in a batch.
#include "bsgpu_device.h"
#include "p3p.h"

namespace bsg {

namespace {

constexpr int kPpThreads = 256;
constexpr int kPpGroup = 4;
constexpr int kPpSamples = kPpThreads / kPpGroup;

struct PpShared {
  double hyp[kPpSamples][kP3pMaxSol * 12];
  double best_T[12];
  int idx[kPpSamples][3];
  int nsol[kPpSamples];
  int count[kPpSamples * kP3pMaxSol];
  int best_idx[3];
  int niters, best, consumed;
};

__global__ void __launch_bounds__(kPpThreads) p3p_kernel(const int* __restrict__ obs_start, const double2* __restrict__ pix,
                                                         const double* __restrict__ pts, const DevCamera* __restrict__ cams,
                                                         const int* __restrict__ cam_of, double prob, double threshold_px, int max_iters,
                                                         unsigned long long seed, int truncate, unsigned char* __restrict__ mask,
                                                         double* __restrict__ out_d, int* __restrict__ out_i) {
  __shared__ PpShared sh;
  const int frame = blockIdx.x, tid = threadIdx.x, g = tid / kPpGroup, l = tid % kPpGroup;
  const int o0 = obs_start[frame], n = obs_start[frame + 1] - o0;
  const DevCamera& cam = cams[cam_of[frame]];
  const double K[4] = {cam.fx, cam.fy, cam.cx, cam.cy};
  double* od = out_d + (size_t)kP3pOutDoubles * frame;
  int* oi = out_i + (size_t)kP3pOutInts * frame;
  if (n < 4) {   // three pairs cannot tell P3P's solutions apart: no pose
    for (int i = tid; i < n; i += kPpThreads) mask[o0 + i] = 0;
    if (tid < kP3pOutDoubles) od[tid] = NAN;
    if (tid == 0) { oi[0] = 0; oi[1] = 0; oi[5] = P3P_TOO_FEW; }
    if (tid < 3) oi[2 + tid] = -1;
    return;
  }
  const double thr2 = threshold_px * threshold_px;
  if (tid == 0) { sh.niters = max_iters; sh.best = 0; sh.consumed = 0; }
  if (tid < 12) sh.best_T[tid] = NAN;
  if (tid < 3) sh.best_idx[tid] = -1;
  __syncthreads();
  const int shift = kPpGroup * ((tid & 63) / kPpGroup);
  for (long long base = 0;; base += kPpSamples) {
    const int niters = sh.niters;
    if (base >= niters) break;
    const long long s = base + g;
    const bool active = s < niters;
    // the sample's solutions, one per lane of its group
    double T[12], key = INFINITY;
    bool has = false;
    int i0 = 0, i1 = 0, i2 = 0;
    if (active) {
      p3p_sample(seed, (uint64_t)frame, (uint64_t)s, n, i0, i1, i2);
      const double2 a0 = pix[o0 + i0], a1 = pix[o0 + i1], a2 = pix[o0 + i2];
      const double px[6] = {p3p_pixel(a0.x, truncate), p3p_pixel(a0.y, truncate), p3p_pixel(a1.x, truncate),
                            p3p_pixel(a1.y, truncate), p3p_pixel(a2.x, truncate), p3p_pixel(a2.y, truncate)};
      const double *q0 = pts + 3 * (size_t)(o0 + i0), *q1 = pts + 3 * (size_t)(o0 + i1), *q2 = pts + 3 * (size_t)(o0 + i2);
      const double P[9] = {q0[0], q0[1], q0[2], q1[0], q1[1], q1[2], q2[0], q2[1], q2[2]};
      P3pSetup S;
      p3p_setup(px, P, K, S);
      double lam[3];
      if (p3p_candidate(S, l, lam)) {
        p3p_polish(S, lam);
        has = p3p_pose(S, lam, T);
        if (has) key = p3p_key(S, lam);
      }
    }
    int rank = 0;
#pragma unroll
    for (int j = 0; j < kPpGroup; ++j) {
      const double kj = __shfl(key, j, kPpGroup);
      rank += (kj < key || (kj == key && j < l)) ? 1 : 0;
    }
    if (has) {
#pragma unroll
      for (int e = 0; e < 12; ++e) sh.hyp[g][12 * rank + e] = T[e];
    }
    const unsigned bits = (unsigned)((__ballot(has) >> shift) & 0xFull);
    if (l == 0) {
      sh.nsol[g] = __popc(bits);
      sh.idx[g][0] = i0; sh.idx[g][1] = i1; sh.idx[g][2] = i2;
    }
    sh.count[tid] = 0;
    __syncthreads();
    // the round's hypotheses against every pair
    for (int c0 = 0; c0 < n; c0 += kPpThreads) {
      const int i = c0 + tid;
      const bool valid = i < n;
      double u = 0.0, v = 0.0, X = 0.0, Y = 0.0, Z = 0.0;
      if (valid) {
        const double2 a = pix[o0 + i];
        const double* q = pts + 3 * (size_t)(o0 + i);
        u = p3p_pixel(a.x, truncate); v = p3p_pixel(a.y, truncate);
        X = q[0]; Y = q[1]; Z = q[2];
      }
      for (int sg = 0; sg < kPpSamples; ++sg) {
        const int ns = sh.nsol[sg];
        for (int h = 0; h < ns; ++h) {
          const bool inl = valid && p3p_inlier(sh.hyp[sg] + 12 * h, K, u, v, X, Y, Z, thr2);
          const int cnt = __popcll(__ballot(inl));
          if ((tid & 63) == 0 && cnt > 0) atomicAdd(&sh.count[sg * kP3pMaxSol + h], cnt);
        }
      }
    }
    __syncthreads();
    // the improving updates, in sample order
    if (tid == 0) {
      int nit = niters, best = sh.best, consumed = sh.consumed, pick = -1;
      for (int sg = 0; sg < kPpSamples && base + sg < nit; ++sg) {
        consumed = (int)(base + sg + 1);
        for (int h = 0; h < sh.nsol[sg]; ++h) {
          const int c = sh.count[sg * kP3pMaxSol + h];
          if (c > (best > 3 ? best : 3)) {
            best = c; pick = sg * kP3pMaxSol + h;
            nit = p3p_update_niters(prob, (double)(n - c) / (double)n, nit);
          }
        }
      }
      if (pick >= 0) {
        const int sg = pick / kP3pMaxSol, h = pick % kP3pMaxSol;
        for (int e = 0; e < 12; ++e) sh.best_T[e] = sh.hyp[sg][12 * h + e];
        for (int k = 0; k < 3; ++k) sh.best_idx[k] = sh.idx[sg][k];
      }
      sh.niters = nit; sh.best = best; sh.consumed = consumed;
    }
    __syncthreads();
  }
  // the best model's inlier set and the pose in bsgpu_localize_frames' layout; without a model no pose: mask 0, NaN
  const int best = sh.best;
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = sh.best_T[e];
  for (int i = tid; i < n; i += kPpThreads) {
    unsigned char keep = 0;
    if (best > 0) {
      const double2 a = pix[o0 + i];
      const double* q = pts + 3 * (size_t)(o0 + i);
      keep = p3p_inlier(T, K, p3p_pixel(a.x, truncate), p3p_pixel(a.y, truncate), q[0], q[1], q[2], thr2) ? 1 : 0;
    }
    mask[o0 + i] = keep;
  }
  if (tid < 12) od[tid] = sh.best_T[tid];
  if (tid == 0) {
    double q[4] = {NAN, NAN, NAN, NAN}, p[3] = {NAN, NAN, NAN};
    if (best > 0) p3p_baselink_pose(T, cam.R, cam.t, q, p);
    for (int e = 0; e < 4; ++e) od[12 + e] = q[e];
    for (int e = 0; e < 3; ++e) od[16 + e] = p[e];
    oi[0] = best; oi[1] = sh.consumed; oi[5] = best > 0 ? P3P_OK : P3P_NO_MODEL;
  }
  if (tid < 3) oi[2 + tid] = sh.best_idx[tid];
}

}  // namespace

void launch_absolute_pose_ransac(hipStream_t s, int n_frames, const int* obs_start, const double2* pix, const double* pts,
                                 const DevCamera* cams, const int* cam_of, double prob, double threshold_px, int max_iters, uint64_t seed,
                                 int truncate, unsigned char* mask, double* out_d, int* out_i) {
  if (n_frames <= 0) return;
  hipLaunchKernelGGL(p3p_kernel, dim3(n_frames), dim3(kPpThreads), 0, s, obs_start, pix, pts, cams, cam_of, prob, threshold_px, max_iters,
                     (unsigned long long)seed, truncate, mask, out_d, out_i);
}

}  // namespace bsg
