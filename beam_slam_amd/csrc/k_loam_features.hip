// LOAM feature extraction for a batch of scans (bsgpu_extract_loam_features) — the feature_extractor->ExtractFeatures(cloud) that every
// lidar scan of the reference goes through before a matcher sees it (bs_models/src/lib/lidar/scan_pose.cpp:34-37, 63-66, 92-95).  The
// rules of one ring are loam_features.h, shared with the CPU tests.
//   loam_ring_kernel       a lane per point of the call: validity and ring (the ring field, or the elevation compared against the
//                          host's tangents); clears the point's label and curvature
//   loam_features_kernel   ONE workgroup of kLoamFeatThreads lanes per (scan, ring).  It compacts its ring's points from the scan in
//                          chunks of a workgroup by wave ballots and a prefix over the waves' counts — a stable partition, whatever the
//                          schedule —, keeps the positions' indices, curvature, picked / far flags and labels in LDS, computes far flags,
//                          unreliable marks and curvature with a lane per position, and then walks the regions in order: every pick is a
//                          workgroup arg-max (arg-min) of the key (curvature, position) over the region's eligible positions, whose
//                          neighbour marks lane 0 makes on the LDS flags.
// The key is a total order, so a pick does not depend on the number of lanes or waves.  A ring is a serial chain of at most
// regions x (max_corner_less_sharp + max_surface_flat) picks of two barriers each; the rings of a call run side by side.  Workgroups
// never wait on each other, and there are no atomics, floating-point or other: every output word has one writer (the overflow flag is
// only ever set to 1).
// The picks go to fixed-capacity slots, pick_cap per (scan, ring) in pick order with two counts per region; the host packs them into the
// caller's arrays during the copy-out.
// This translation unit is compiled with floating-point contraction off (Makefile): the device must return the bits of the header on
// the host.
#include "bsgpu_internal.h"
#include "loam_features.h"

namespace bsg {

namespace {

constexpr int kLoamFeatThreads = 256;
constexpr int kLoamFeatWaves = kLoamFeatThreads / 64;

__global__ __launch_bounds__(kLoamFeatThreads) void loam_ring_kernel(int n_points, const double* __restrict__ pts, const int* __restrict__ ring,
                                                                      int axis, int beams, const double* __restrict__ bound,
                                                                      int* __restrict__ ring_id, int* __restrict__ label, double* __restrict__ curvature) {
  const int i = (int)(blockIdx.x * (unsigned)kLoamFeatThreads + threadIdx.x);
  if (i >= n_points) return;
  const double p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
  int r = -1;
  if (loam_feat_valid(p)) {
    if (ring) { const int v = ring[i]; r = v >= 0 && v < beams ? v : -1; }
    else r = loam_feat_ring(p, axis, beams, bound);
  }
  ring_id[i] = r;
  label[i] = LOAM_FEAT_DROPPED;
  curvature[i] = __builtin_nan("");
}

// One pick of a walk: the best eligible position of sp .. ep by the walk's order, -1 when there is none; the same value in every lane.
// red_v / red_i: kLoamFeatWaves entries of LDS.  Ends with the reduction's entries read by every lane; the caller's barrier after the
// pick's marks also keeps the next pick's entries apart from these.
template <bool EDGE>
__device__ __forceinline__ int loam_feat_pick(int sp, int ep, double threshold, const double* curv, const unsigned char* picked, double* red_v, int* red_i) {
  double bv = 0.0;
  int bi = -1;
  for (int i = sp + (int)threadIdx.x; i <= ep; i += kLoamFeatThreads) {
    const double cv = curv[i];
    const bool eligible = !picked[i] && (EDGE ? cv > threshold : cv < threshold);
    if (eligible && (EDGE ? loam_feat_better_edge(cv, i, bv, bi) : loam_feat_better_flat(cv, i, bv, bi))) { bv = cv; bi = i; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (oi >= 0 && (EDGE ? loam_feat_better_edge(ov, oi, bv, bi) : loam_feat_better_flat(ov, oi, bv, bi))) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = bv; red_i[threadIdx.x >> 6] = bi; }
  __syncthreads();
  bv = red_v[0]; bi = red_i[0];
#pragma unroll
  for (int w = 1; w < kLoamFeatWaves; ++w) {
    const double ov = red_v[w];
    const int oi = red_i[w];
    if (oi >= 0 && (EDGE ? loam_feat_better_edge(ov, oi, bv, bi) : loam_feat_better_flat(ov, oi, bv, bi))) { bv = ov; bi = oi; }
  }
  return bi;
}

// ring_id, label, curvature: per point of the call (loam_ring_kernel's); picks: pick_cap per (scan, ring); counts: 2 per (scan, ring,
// region): edges taken, surfaces taken; overflow: set when a ring has more than kLoamMaxRingPoints points (the call is then refused).
__global__ __launch_bounds__(kLoamFeatThreads) void loam_features_kernel(const int* __restrict__ scan_start, const double* __restrict__ points,
                                                                          const int* __restrict__ ring_id, const LoamFeatParams P, int pick_cap,
                                                                          int* __restrict__ label, double* __restrict__ curvature,
                                                                          int* __restrict__ picks, int* __restrict__ counts, int* __restrict__ overflow) {
  __shared__ double curv[kLoamMaxRingPoints];
  __shared__ int idx[kLoamMaxRingPoints];
  __shared__ unsigned char picked[kLoamMaxRingPoints];
  __shared__ unsigned char far[kLoamMaxRingPoints];
  __shared__ signed char lab[kLoamMaxRingPoints];
  __shared__ double red_v[kLoamFeatWaves];
  __shared__ int red_i[kLoamFeatWaves];
  __shared__ int wave_count[kLoamFeatWaves];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int scan = (int)blockIdx.x / P.beams, ring = (int)blockIdx.x % P.beams;
  const int s0 = scan_start[scan], s1 = scan_start[scan + 1];
  const double* pts = points + 3 * (size_t)s0;
  int* my_counts = counts + 2 * (size_t)blockIdx.x * P.regions;
  int* my_picks = picks + (size_t)blockIdx.x * pick_cap;
  for (int k = tid; k < 2 * P.regions; k += kLoamFeatThreads) my_counts[k] = 0;

  // ---- the ring's points, in their order of arrival ----
  int n = 0;
  for (int base = s0; base < s1; base += kLoamFeatThreads) {
    const int i = base + tid;
    const bool mine = i < s1 && ring_id[i] == ring;
    const unsigned long long ballot = __ballot(mine);
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int before = n, total = 0;
#pragma unroll
    for (int w = 0; w < kLoamFeatWaves; ++w) {
      const int cnt = wave_count[w];
      before += w < wave ? cnt : 0;
      total += cnt;
    }
    const int at = before + __popcll(ballot & ((1ull << lane) - 1ull));
    if (mine && at < kLoamMaxRingPoints) idx[at] = i - s0;
    n += total;
    __syncthreads();      // (the next chunk overwrites the waves' counts; idx is complete after the last)
  }
  if (n > kLoamMaxRingPoints) {
    if (tid == 0) *overflow = 1;
    return;
  }
  const int c = P.c;
  if (n - 1 <= 2 * c) return;      // the ring is skipped whole: its points stay DROPPED

  // ---- flags, unreliable marks, curvature: a lane per position ----
  for (int i = tid; i < n; i += kLoamFeatThreads) {
    picked[i] = 0;
    lab[i] = (signed char)LOAM_FEAT_DROPPED;
    far[i] = i + 1 < n && loam_feat_far(pts, idx, i) ? 1 : 0;
  }
  __syncthreads();
  for (int i = c + tid; i < n - c; i += kLoamFeatThreads) {
    if (i < n - 1 - c) loam_feat_unreliable(pts, idx, c, i, picked);      // (lanes may set the same flag: every store is a 1)
    const double cv = loam_feat_curvature(pts, idx, c, i);
    curv[i] = cv;
    curvature[(size_t)s0 + idx[i]] = cv;
  }
  __syncthreads();

  // ---- the regions, in order ----
  int written = 0;      // picks of this ring so far (the same in every lane)
  for (int j = 0; j < P.regions; ++j) {
    int sp, ep;
    loam_feat_region(n, c, P.regions, j, &sp, &ep);
    if (ep <= sp) continue;
    int n_edges = 0, n_flat = 0;
    for (; n_edges < P.max_less_sharp; ++n_edges) {
      const int best = loam_feat_pick<true>(sp, ep, P.threshold, curv, picked, red_v, red_i);
      if (best < 0) break;
      if (tid == 0) {
        lab[best] = (signed char)(n_edges < P.max_sharp ? LOAM_FEAT_SHARP : LOAM_FEAT_LESS_SHARP);
        if (written < pick_cap) my_picks[written] = idx[best];
        loam_feat_mark_picked(far, n, c, best, picked);
      }
      ++written;
      __syncthreads();
    }
    __syncthreads();      // (a walk that ended without a pick: its reduction entries are read before the next walk's are written)
    for (; n_flat < P.max_flat; ++n_flat) {
      const int best = loam_feat_pick<false>(sp, ep, P.threshold, curv, picked, red_v, red_i);
      if (best < 0) break;
      if (tid == 0) {
        lab[best] = (signed char)LOAM_FEAT_FLAT;
        if (written < pick_cap) my_picks[written] = idx[best];
        loam_feat_mark_picked(far, n, c, best, picked);
      }
      ++written;
      __syncthreads();
    }
    __syncthreads();
    if (tid == 0) { my_counts[2 * j] = n_edges; my_counts[2 * j + 1] = n_flat; }
    for (int i = sp + tid; i <= ep; i += kLoamFeatThreads)
      if (lab[i] == (signed char)LOAM_FEAT_DROPPED) lab[i] = (signed char)LOAM_FEAT_LESS_FLAT;
  }
  __syncthreads();
  for (int i = tid; i < n; i += kLoamFeatThreads) label[(size_t)s0 + idx[i]] = (int)lab[i];
}

}  // namespace

void launch_extract_loam_features(hipStream_t s, int n_scans, int n_points, const int* scan_start, const double* points, const int* ring,
                                  const LoamFeatParams& P, const double* bound, int pick_cap, int* ring_id, int* label, double* curvature,
                                  int* picks, int* counts, int* overflow) {
  if (n_scans <= 0) return;
  (void)hipMemsetAsync(overflow, 0, sizeof(int), s);
  if (n_points > 0)
    hipLaunchKernelGGL(loam_ring_kernel, dim3((unsigned)((n_points + kLoamFeatThreads - 1) / kLoamFeatThreads)), dim3(kLoamFeatThreads), 0, s, n_points,
                       points, ring, P.axis, P.beams, bound, ring_id, label, curvature);
  hipLaunchKernelGGL(loam_features_kernel, dim3((unsigned)n_scans * (unsigned)P.beams), dim3(kLoamFeatThreads), 0, s, scan_start, points, ring_id, P,
                     pick_cap, label, curvature, picks, counts, overflow);
}

}  // namespace bsg
