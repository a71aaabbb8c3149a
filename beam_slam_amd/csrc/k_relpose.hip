// Seven-point RANSAC two-view bootstrap for a batch of match sets (bsgpu_relative_pose_ransac): the
// beam_cv::RelativePoseEstimator::RANSACEstimator / Triangulation::TriangulatePoints / inlier-ratio steps of
// bs_models::vision::ComputePathWithVision (bs_models/src/lib/vision/utils.cpp:44-94), seven_point.h's loop on the device.
//
// One launch, one 256-thread workgroup per set, every RANSAC round inside the kernel.  A round evaluates kRpSamples = 16 consecutive
// samples, one per group of 16 lanes.  Twelve lanes of a group each draw the sample and repeat the part its hypotheses share (the
// null space, the cubic, the up to three essential matrices in ascending order: a few thousand flops, all in registers), then own
// one hypothesis, root x decomposition, and write its pose to the round's table, 12 * sample + 4 * root + decomposition: the only
// thing in LDS.  All 256 threads then score every hypothesis of the round against the set's matches (a match per thread: its
// triangulation — the 4 x 4 eigenproblem in registers — and both reprojections; inlier counts by ballot and integer LDS atomics, so
// the counts do not depend on any order), and thread 0 applies the round's improving updates in sample and hypothesis order, ignoring
// the samples at or past the iteration bound then in force: the serial loop of the contract, whatever the round size.
// Workgroups never wait on each other: a set's results are the same bits alone or in a batch.
#include "bsgpu_device.h"
#include "seven_point.h"

namespace bsg {

namespace {

constexpr int kRpThreads = 256;
constexpr int kRpGroup = 16;
constexpr int kRpSamples = kRpThreads / kRpGroup;

struct RpShared {
  double hyp[kRpSamples][kSp7MaxHyp * 12];
  double best_T[12];
  int idx[kRpSamples][7];
  int nhyp[kRpSamples];
  int count[kRpSamples * kSp7MaxHyp];
  int best_idx[7];
  int niters, best, consumed, n_valid;
};

struct RpMatch {
  double u1, v1, u2, v2;
};

__device__ inline RpMatch load_match(const double2* __restrict__ pf, const double2* __restrict__ pl, int i, int truncate) {
  const double2 a = pf[i], b = pl[i];
  return {sp7_pixel(a.x, truncate), sp7_pixel(a.y, truncate), sp7_pixel(b.x, truncate), sp7_pixel(b.y, truncate)};
}

__global__ void __launch_bounds__(kRpThreads) relpose_kernel(const int* __restrict__ match_start, const double2* __restrict__ pix_first,
                                                             const double2* __restrict__ pix_last, const DevCamera* __restrict__ cams,
                                                             const int* __restrict__ cam_of, double prob, double threshold_px, int max_iters,
                                                             unsigned long long seed, int truncate, double validate_px,
                                                             double min_inlier_ratio, unsigned char* __restrict__ mask,
                                                             unsigned char* __restrict__ valid_mask, double* __restrict__ points,
                                                             double* __restrict__ out_d, int* __restrict__ out_i) {
  __shared__ RpShared sh;
  const int set = blockIdx.x, tid = threadIdx.x, g = tid / kRpGroup, l = tid % kRpGroup;
  const int o0 = match_start[set], n = match_start[set + 1] - o0;
  const DevCamera& cam = cams[cam_of[set]];
  const double K[4] = {cam.fx, cam.fy, cam.cx, cam.cy};
  const double2* pf = pix_first + o0;
  const double2* pl = pix_last + o0;
  double* od = out_d + (size_t)kRelposeOutDoubles * set;
  int* oi = out_i + (size_t)kRelposeOutInts * set;
  if (n < 8) {   // seven matches always fit their own model: no pose
    for (int i = tid; i < n; i += kRpThreads) {
      mask[o0 + i] = 0; valid_mask[o0 + i] = 0;
      points[3 * (size_t)(o0 + i)] = NAN; points[3 * (size_t)(o0 + i) + 1] = NAN; points[3 * (size_t)(o0 + i) + 2] = NAN;
    }
    if (tid < kRelposeOutDoubles) od[tid] = NAN;
    if (tid == 0) { oi[0] = 0; oi[1] = 0; oi[9] = SP7_TOO_FEW; oi[10] = 0; }
    if (tid < 7) oi[2 + tid] = -1;
    return;
  }
  const double thr2 = threshold_px * threshold_px, val2 = validate_px * validate_px;
  if (tid == 0) { sh.niters = max_iters; sh.best = 0; sh.consumed = 0; sh.n_valid = 0; }
  if (tid < 12) sh.best_T[tid] = NAN;
  if (tid < 7) sh.best_idx[tid] = -1;
  __syncthreads();
  for (long long base = 0;; base += kRpSamples) {
    const int niters = sh.niters;
    if (base >= niters) break;
    const long long s = base + g;
    // the sample's hypotheses, one per lane of its group
    if (l == 0) sh.nhyp[g] = 0;
    if (s < niters && l < kSp7MaxHyp) {
      int idx[7];
      sp7_sample(seed, (uint64_t)set, (uint64_t)s, n, idx);
      double m[28];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const RpMatch q = load_match(pf, pl, idx[k], truncate);
        m[4 * k] = (q.u1 - K[2]) / K[0]; m[4 * k + 1] = (q.v1 - K[3]) / K[1];
        m[4 * k + 2] = (q.u2 - K[2]) / K[0]; m[4 * k + 3] = (q.v2 - K[3]) / K[1];
      }
      double E[9 * kSp7MaxSol];
      const int ns = sp7_models(m, E);
      const int root = l / 4;
      if (root < ns) {
        double Er[9], T[12];
#pragma unroll
        for (int e = 0; e < 9; ++e) Er[e] = root == 0 ? E[e] : root == 1 ? E[9 + e] : E[18 + e];
        sp7_decompose(Er, l % 4, T);
#pragma unroll
        for (int e = 0; e < 12; ++e) sh.hyp[g][12 * l + e] = T[e];
      }
      if (l == 0) {
        sh.nhyp[g] = 4 * ns;
#pragma unroll
        for (int k = 0; k < 7; ++k) sh.idx[g][k] = idx[k];
      }
    }
    if (tid < kRpSamples * kSp7MaxHyp) sh.count[tid] = 0;
    __syncthreads();
    // the round's hypotheses against every match
    for (int c0 = 0; c0 < n; c0 += kRpThreads) {
      const int i = c0 + tid;
      const bool valid = i < n;
      if (__ballot(valid) == 0) continue;   // a wave without a match of this chunk
      const RpMatch q = load_match(pf, pl, valid ? i : 0, truncate);
      for (int sg = 0; sg < kRpSamples; ++sg) {
        const int nh = sh.nhyp[sg];
        for (int h = 0; h < nh; ++h) {
          double T[12], P[3];
#pragma unroll
          for (int e = 0; e < 12; ++e) T[e] = sh.hyp[sg][12 * h + e];
          const bool inl = sp7_score(T, K, q.u1, q.v1, q.u2, q.v2, thr2, P) && valid;
          const int cnt = __popcll(__ballot(inl));
          if ((tid & 63) == 0 && cnt > 0) atomicAdd(&sh.count[sg * kSp7MaxHyp + h], cnt);
        }
      }
    }
    __syncthreads();
    // the improving updates, in sample and hypothesis order
    if (tid == 0) {
      int nit = niters, best = sh.best, consumed = sh.consumed, pick = -1;
      for (int sg = 0; sg < kRpSamples && base + sg < nit; ++sg) {
        consumed = (int)(base + sg + 1);
        for (int h = 0; h < sh.nhyp[sg]; ++h) {
          const int c = sh.count[sg * kSp7MaxHyp + h];
          if (c > (best > 7 ? best : 7)) {
            best = c; pick = sg * kSp7MaxHyp + h;
            nit = sp7_update_niters(prob, (double)(n - c) / (double)n, nit);
          }
        }
      }
      if (pick >= 0) {
        const int sg = pick / kSp7MaxHyp, h = pick % kSp7MaxHyp;
        for (int e = 0; e < 12; ++e) sh.best_T[e] = sh.hyp[sg][12 * h + e];
        for (int k = 0; k < 7; ++k) sh.best_idx[k] = sh.idx[sg][k];
      }
      sh.niters = nit; sh.best = best; sh.consumed = consumed;
    }
    __syncthreads();
  }
  // under the best model: the inlier set, the points, the validity gate; without a model no pose: masks 0, NaN
  const int best = sh.best;
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = sh.best_T[e];
  for (int c0 = 0; c0 < n; c0 += kRpThreads) {
    const int i = c0 + tid;
    bool keep = false, ok = false;
    double P[3] = {NAN, NAN, NAN};
    if (i < n && best > 0) {
      const RpMatch q = load_match(pf, pl, i, truncate);
      keep = sp7_score(T, K, q.u1, q.v1, q.u2, q.v2, thr2, P);
      ok = sp7_inlier(T, K, q.u1, q.v1, q.u2, q.v2, P, val2);
    }
    if (i < n) {
      mask[o0 + i] = keep ? 1 : 0; valid_mask[o0 + i] = ok ? 1 : 0;
      points[3 * (size_t)(o0 + i)] = P[0]; points[3 * (size_t)(o0 + i) + 1] = P[1]; points[3 * (size_t)(o0 + i) + 2] = P[2];
    }
    const int cnt = __popcll(__ballot(ok));
    if ((tid & 63) == 0 && cnt > 0) atomicAdd(&sh.n_valid, cnt);
  }
  __syncthreads();
  if (tid < 12) od[tid] = sh.best_T[tid];
  if (tid == 0) {
    double q[8], p[6], ratio = NAN;
    for (int e = 0; e < 8; ++e) q[e] = NAN;
    for (int e = 0; e < 6; ++e) p[e] = NAN;
    int pair_valid = 0;
    if (best > 0) {
      sp7_baselink_poses(T, cam.R, cam.t, q, p);
      ratio = (double)sh.n_valid / (double)n;
      pair_valid = ratio < min_inlier_ratio ? 0 : 1;
    }
    for (int e = 0; e < 8; ++e) od[12 + e] = q[e];
    for (int e = 0; e < 6; ++e) od[20 + e] = p[e];
    od[26] = ratio;
    oi[0] = best; oi[1] = sh.consumed; oi[9] = best > 0 ? SP7_OK : SP7_NO_MODEL; oi[10] = pair_valid;
  }
  if (tid < 7) oi[2 + tid] = sh.best_idx[tid];
}

}  // namespace

void launch_relative_pose_ransac(hipStream_t s, int n_sets, const int* match_start, const double2* pix_first, const double2* pix_last,
                                 const DevCamera* cams, const int* cam_of, double prob, double threshold_px, int max_iters, uint64_t seed,
                                 int truncate, double validate_px, double min_inlier_ratio, unsigned char* mask, unsigned char* valid_mask,
                                 double* points, double* out_d, int* out_i) {
  if (n_sets <= 0) return;
  hipLaunchKernelGGL(relpose_kernel, dim3(n_sets), dim3(kRpThreads), 0, s, match_start, pix_first, pix_last, cams, cam_of, prob,
                     threshold_px, max_iters, (unsigned long long)seed, truncate, validate_px, min_inlier_ratio, mask, valid_mask, points,
                     out_d, out_i);
}

}  // namespace bsg
