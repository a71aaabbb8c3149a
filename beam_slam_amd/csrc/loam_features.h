// LOAM feature extraction of one scan (bsgpu_extract_loam_features, k_loam_features.hip): the reference's
// feature_extractor->ExtractFeatures(cloud) (bs_models/src/lib/lidar/scan_pose.cpp:34-37), as include/bsgpu.h pins it.  libbeam's
// LoamFeatureExtractor is not in the reference checkout: the rules below are RECALLED from it and from the LOAM scan registration it
// derives from, not verified.  This header is the definition: the kernel returns its outputs exactly, indices and labels equal, points
// and curvature bit for bit.  Host- and device-compilable; it includes nothing of HIP, so the CPU tests build it with g++ alone.
//
//   loam_feat_valid            finite and |p|^2 >= 1e-4
//   loam_feat_ring             the ring of a point by elevation: comparisons of v against tan(beta) h only
//   loam_feat_far              |p_{i+1} - p_i|^2 > 0.05: where MarkAsPicked stops
//   loam_feat_unreliable       the marks of one position (occlusion edges, beams nearly parallel to a surface)
//   loam_feat_curvature        the curvature of one position
//   loam_feat_region           the bounds of region j of a ring
//   loam_feat_better_edge / _flat   the total order (curvature, position) of the two walks
//   loam_feat_mark_picked      MarkAsPicked
//   loam_feat_bounds           (host only) the tangents of the beams + 1 boundary angles, once per call
//   loam_extract_serial        (host only) one scan on one core
//
// A ring is handled through idx (n positions: the ring's points in their order of arrival, as indices into the scan) over the scan's
// packed points; picked, far and the labels are per position.
//
// Bits.  Contraction is off in every body here (the pragma is clang's; a GCC build passes -ffp-contract=off), and the kernel's object is
// compiled with contraction off as a whole (csrc/Makefile).  Nothing here calls a library function on the device but sqrt, which is
// correctly rounded on both sides; the one tangent per boundary is the host's (loam_feat_bounds).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define BSG_FEAT_FN __host__ __device__ inline
#else
#define BSG_FEAT_FN inline
#endif
#if defined(__clang__)
#define BSG_FEAT_EXACT _Pragma("clang fp contract(off)")
#else
#define BSG_FEAT_EXACT
#endif

namespace bsg {

enum { LOAM_FEAT_DROPPED = -1, LOAM_FEAT_LESS_FLAT = 0, LOAM_FEAT_FLAT = 1, LOAM_FEAT_LESS_SHARP = 2, LOAM_FEAT_SHARP = 3 };

constexpr int kLoamMaxRings = 128;
constexpr int kLoamMaxRingPoints = 4096;
constexpr int kLoamMaxCurvatureRegion = 16;
constexpr int kLoamMaxRegions = 64;

struct LoamFeatParams {
  int beams, regions, c;                       // number_of_beams, n_feature_regions, curvature_region
  int max_sharp, max_less_sharp, max_flat;
  int axis;                                    // vertical_axis: 0 X, 1 Y, 2 Z
  double threshold;                            // surface_curvature_threshold
};

// (a.x^2 + a.y^2) + a.z^2 of a difference or of a point: every squared length of the contract has this order
BSG_FEAT_FN double loam_feat_sq(double x, double y, double z) {
  BSG_FEAT_EXACT
  return (x * x + y * y) + z * z;
}
BSG_FEAT_FN double loam_feat_d2(const double* a, const double* b) { return loam_feat_sq(a[0] - b[0], a[1] - b[1], a[2] - b[2]); }

BSG_FEAT_FN bool loam_feat_valid(const double* p) {
  // (x - x is 0 for a finite x and NaN otherwise: no isfinite, whose host and device spellings differ)
  if (!(p[0] - p[0] == 0.0) || !(p[1] - p[1] == 0.0) || !(p[2] - p[2] == 0.0)) return false;
  return !(loam_feat_sq(p[0], p[1], p[2]) < 1e-4);
}

// The ring of a valid point by elevation, -1: dropped.  v: the coordinate along the vertical axis, h: the root of the other two
// squared.  With t = (angle + fov / 2) (beams - 1) / fov + 0.5 the ring is trunc(t): ring 0 is -1 < t < 1 and ring r >= 1 is
// r <= t < r + 1.  bound (beams + 1): the tangents of the angles at t = -1, 1, 2 .. beams; t >= k is v >= bound[k] h.  A boundary at
// or below -90 degrees is -infinity (every point is above it), one at or above +90 degrees +infinity (no point is).
BSG_FEAT_FN bool loam_feat_above(double v, double h, double b, bool strict) {
  BSG_FEAT_EXACT
  if (b == -std::numeric_limits<double>::infinity()) return true;
  if (b == std::numeric_limits<double>::infinity()) return false;
  const double bh = b * h;
  return strict ? v > bh : v >= bh;
}
BSG_FEAT_FN int loam_feat_ring(const double* p, int axis, int beams, const double* bound) {
  BSG_FEAT_EXACT
  const double v = p[axis], a = p[axis == 0 ? 1 : 0], b = p[axis == 2 ? 1 : 2];
  const double h = sqrt(a * a + b * b);
  if (!loam_feat_above(v, h, bound[0], true)) return -1;
  int r = 0;
  for (int k = 1; k <= beams; ++k) r += loam_feat_above(v, h, bound[k], false) ? 1 : 0;
  return r < beams ? r : -1;
}

BSG_FEAT_FN const double* loam_feat_at(const double* pts, const int* idx, int i) { return pts + 3 * (size_t)idx[i]; }

// position i in [0, n - 1): MarkAsPicked does not pass from i to i + 1 or back
BSG_FEAT_FN bool loam_feat_far(const double* pts, const int* idx, int i) {
  return loam_feat_d2(loam_feat_at(pts, idx, i + 1), loam_feat_at(pts, idx, i)) > 0.05;
}

// The marks of position i in [c, n - 1 - c).  They set flags and read none, so their order does not matter.
BSG_FEAT_FN void loam_feat_unreliable(const double* pts, const int* idx, int c, int i, unsigned char* picked) {
  BSG_FEAT_EXACT
  const double *p = loam_feat_at(pts, idx, i), *q = loam_feat_at(pts, idx, i + 1), *o = loam_feat_at(pts, idx, i - 1);
  const double dn = loam_feat_d2(q, p), dp = loam_feat_d2(p, o), pp = loam_feat_sq(p[0], p[1], p[2]);
  if (dn > 0.1) {
    const double r1 = sqrt(pp), r2 = sqrt(loam_feat_sq(q[0], q[1], q[2]));
    if (r1 > r2) {
      const double k = r2 / r1;
      if (sqrt(loam_feat_sq(q[0] - p[0] * k, q[1] - p[1] * k, q[2] - p[2] * k)) / r2 < 0.1)
        for (int j = i - c; j <= i; ++j) picked[j] = 1;
    } else {
      const double k = r1 / r2;
      if (sqrt(loam_feat_sq(q[0] * k - p[0], q[1] * k - p[1], q[2] * k - p[2])) / r1 < 0.1)
        for (int j = i + 1; j <= i + c + 1; ++j) picked[j] = 1;
    }
  }
  const double bar = 0.0002 * pp;
  if (dn > bar && dp > bar) picked[i] = 1;
}

// position i in [c, n - c)
BSG_FEAT_FN double loam_feat_curvature(const double* pts, const int* idx, int c, int i) {
  BSG_FEAT_EXACT
  const double* p = loam_feat_at(pts, idx, i);
  const double w = -2.0 * (double)c;
  double s[3] = {w * p[0], w * p[1], w * p[2]};
  for (int j = 1; j <= c; ++j) {
    const double *a = loam_feat_at(pts, idx, i + j), *b = loam_feat_at(pts, idx, i - j);
    s[0] = s[0] + a[0]; s[1] = s[1] + a[1]; s[2] = s[2] + a[2];
    s[0] = s[0] + b[0]; s[1] = s[1] + b[1]; s[2] = s[2] + b[2];
  }
  return loam_feat_sq(s[0], s[1], s[2]);
}

// Region j of a ring of n points: positions sp .. ep.  A region with ep <= sp is skipped, and its point, if it has one, stays DROPPED.
BSG_FEAT_FN void loam_feat_region(int n, int c, int regions, int j, int* sp, int* ep) {
  const int L = n - 1 - 2 * c;
  *sp = c + (L * j) / regions;
  *ep = c + (L * (j + 1)) / regions - 1;
}

// The walks' total order is the key (curvature, position).  Candidate (cv, i) against the best so far (bv, bi; bi < 0: none yet).
BSG_FEAT_FN bool loam_feat_better_edge(double cv, int i, double bv, int bi) { return bi < 0 || cv > bv || (cv == bv && i > bi); }
BSG_FEAT_FN bool loam_feat_better_flat(double cv, int i, double bv, int bi) { return bi < 0 || cv < bv || (cv == bv && i < bi); }

// far: loam_feat_far per position
BSG_FEAT_FN void loam_feat_mark_picked(const unsigned char* far, int n, int c, int i, unsigned char* picked) {
  picked[i] = 1;
  for (int k = 1; k <= c; ++k) {
    if (i + k >= n || far[i + k - 1]) break;
    picked[i + k] = 1;
  }
  for (int k = 1; k <= c; ++k) {
    if (i - k < 0 || far[i - k]) break;
    picked[i - k] = 1;
  }
}

// ---- host only --------------------------------------------------------------------------------------------------------------------------------
// bound (beams + 1): the one library function of the contract, and never the device's.  beams == 1: t is 0.5 for every point.
inline void loam_feat_bounds(int beams, double fov_deg, double* bound) {
  const double inf = std::numeric_limits<double>::infinity();
  for (int k = 0; k <= beams; ++k) {
    if (beams == 1) { bound[k] = k == 0 ? -inf : inf; continue; }
    const double t = k == 0 ? -1.0 : (double)k;
    const double deg = (t - 0.5) * fov_deg / (double)(beams - 1) - 0.5 * fov_deg;
    bound[k] = deg <= -90.0 ? -inf : deg >= 90.0 ? inf : std::tan(deg * (3.14159265358979323846 / 180.0));
  }
}

struct LoamFeatures {
  std::vector<int32_t> sharp, less_sharp, flat, less_flat;      // indices into the scan; ring, then region, then pick order
  std::vector<int32_t> label;                                   // per point
  std::vector<double> curvature;                                // per point, NaN where none is defined
};

// bsgpu_extract_loam_features for one scan.  ring: optional, one per point; bound: loam_feat_bounds (read only without ring).
// false: a ring has more than kLoamMaxRingPoints points (the entry point's BSGPU_ERR_UNSUPPORTED).
inline bool loam_extract_serial(int n, const double* pts, const int32_t* ring, const LoamFeatParams& P, const double* bound, LoamFeatures* out) {
  out->sharp.clear(); out->less_sharp.clear(); out->flat.clear(); out->less_flat.clear();
  out->label.assign((size_t)n, LOAM_FEAT_DROPPED);
  out->curvature.assign((size_t)n, std::numeric_limits<double>::quiet_NaN());
  std::vector<std::vector<int>> rings((size_t)P.beams);
  for (int i = 0; i < n; ++i) {
    const double* p = pts + 3 * (size_t)i;
    if (!loam_feat_valid(p)) continue;
    const int r = ring ? (ring[i] >= 0 && ring[i] < P.beams ? (int)ring[i] : -1) : loam_feat_ring(p, P.axis, P.beams, bound);
    if (r >= 0) rings[(size_t)r].push_back(i);
  }
  for (const auto& R : rings) if (R.size() > (size_t)kLoamMaxRingPoints) return false;
  std::vector<unsigned char> picked, far;
  std::vector<double> curv;
  std::vector<int> lab;
  const int c = P.c;
  for (const auto& R : rings) {
    const int m = (int)R.size();
    if (m - 1 <= 2 * c) continue;
    const int* idx = R.data();
    picked.assign((size_t)m, 0); far.assign((size_t)m, 0); curv.assign((size_t)m, 0.0); lab.assign((size_t)m, LOAM_FEAT_DROPPED);
    for (int i = 0; i + 1 < m; ++i) far[(size_t)i] = loam_feat_far(pts, idx, i) ? 1 : 0;
    for (int i = c; i < m - 1 - c; ++i) loam_feat_unreliable(pts, idx, c, i, picked.data());
    for (int i = c; i < m - c; ++i) out->curvature[(size_t)idx[i]] = curv[(size_t)i] = loam_feat_curvature(pts, idx, c, i);
    for (int j = 0; j < P.regions; ++j) {
      int sp, ep;
      loam_feat_region(m, c, P.regions, j, &sp, &ep);
      if (ep <= sp) continue;
      for (int taken = 0; taken < P.max_less_sharp; ++taken) {
        int best = -1;
        for (int i = sp; i <= ep; ++i)
          if (!picked[(size_t)i] && curv[(size_t)i] > P.threshold && loam_feat_better_edge(curv[(size_t)i], i, best < 0 ? 0.0 : curv[(size_t)best], best)) best = i;
        if (best < 0) break;
        lab[(size_t)best] = taken < P.max_sharp ? LOAM_FEAT_SHARP : LOAM_FEAT_LESS_SHARP;
        (taken < P.max_sharp ? out->sharp : out->less_sharp).push_back(idx[best]);
        loam_feat_mark_picked(far.data(), m, c, best, picked.data());
      }
      for (int taken = 0; taken < P.max_flat; ++taken) {
        int best = -1;
        for (int i = sp; i <= ep; ++i)
          if (!picked[(size_t)i] && curv[(size_t)i] < P.threshold && loam_feat_better_flat(curv[(size_t)i], i, best < 0 ? 0.0 : curv[(size_t)best], best)) best = i;
        if (best < 0) break;
        lab[(size_t)best] = LOAM_FEAT_FLAT;
        out->flat.push_back(idx[best]);
        loam_feat_mark_picked(far.data(), m, c, best, picked.data());
      }
      for (int i = sp; i <= ep; ++i) {
        if (lab[(size_t)i] == LOAM_FEAT_DROPPED) { lab[(size_t)i] = LOAM_FEAT_LESS_FLAT; out->less_flat.push_back(idx[i]); }
      }
    }
    for (int i = 0; i < m; ++i) out->label[(size_t)idx[i]] = lab[(size_t)i];
  }
  return true;
}

}  // namespace bsg
