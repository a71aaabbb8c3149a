// The reference clouds of scan-to-map registration (bsgpu_build_registration_maps): the scans of a map under their T_Map_Scan, merged and
// reduced to one centroid per occupied voxel — what RegistrationMap::GetLoamCloudMap / GetPointCloudMap
// (bs_models/src/lib/scan_registration/registration_map.cpp:96-135) rebuild for every incoming scan.  Host- and device-compilable in the
// style of point_grid.h and loam_features.h: plain C++, nothing from HIP but the qualifiers.
//
//   map_finite, map_in_range, map_point_key   a transformed point's 63-bit voxel key; the range rule; the sentinel of a dropped point
//   map_centroid_add, map_centroid_div        the sequential sum of a voxel and its division
//   registration_map_serial                   (host only) the whole contract on one core, std::stable_sort on the keys
//
// Bits.  The device (k_registration_map.hip) must return this header's doubles bit for bit, so every body switches floating-point
// contraction off (point_grid.h, "Bits"); the only fused multiply-adds are grid_apply's, which are written.  A voxel's sum runs over its
// points in input order (scan order, then point order), one addition after the other from +0.0, and is divided once by the count: the
// device sorts (key, index) stably and walks a voxel's run, which is that order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "point_grid.h"

namespace bsg {

constexpr int kMapMaxPoints = 8388608;                   // 2^23 input points per call (BSGPU_MAP_MAX_POINTS)
constexpr int kMapSortTile = 1024;                       // keys per workgroup of the device's radix sort (BSGPU_MAP_SORT_TILE)
constexpr double kMapMergeOnly = -1.0;                   // voxel_size: the reference's sentinel of "no filter"
constexpr double kMapCellRange = 1048576.0;              // 2^20: |q / v| must stay below
constexpr int kMapAxisBits = 21;
constexpr uint64_t kMapDropped = ~(uint64_t)0;           // the key of a dropped point: above every voxel's, so it sorts last

BSG_GRID_FN bool map_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // (false for a NaN)
// |q / v| < 2^20, with the quotient grid_cell_f floors: the cell then lies in [-2^20, 2^20) and its biased index has 21 bits
BSG_GRID_FN bool map_in_range(double q, double v) {
  BSG_GRID_EXACT
  return fabs((q - 0.0) / v) < kMapCellRange;
}
// The key of a transformed point: (iz, iy, ix) biased by 2^20, iz most significant, so that ascending keys are ascending (iz, iy, ix).
// kMapDropped for a point with a coordinate that is not finite; also, with *out_of_range set to 1 (and never to anything else), for a
// finite point outside the range.
BSG_GRID_FN uint64_t map_point_key(const double* q, double v, int* out_of_range) {
  if (!map_finite(q[0]) || !map_finite(q[1]) || !map_finite(q[2])) return kMapDropped;
  if (!map_in_range(q[0], v) || !map_in_range(q[1], v) || !map_in_range(q[2], v)) { *out_of_range = 1; return kMapDropped; }
  const uint64_t ix = (uint64_t)((int64_t)grid_cell_f(q[0], 0.0, v) + (int64_t)kMapCellRange);
  const uint64_t iy = (uint64_t)((int64_t)grid_cell_f(q[1], 0.0, v) + (int64_t)kMapCellRange);
  const uint64_t iz = (uint64_t)((int64_t)grid_cell_f(q[2], 0.0, v) + (int64_t)kMapCellRange);
  return (iz << (2 * kMapAxisBits)) | (iy << kMapAxisBits) | ix;
}
// a point through its scan's transform; T null: the point as it is
BSG_GRID_FN void map_transform(const double* T, const double* p, double* q) {
  if (T) grid_apply(T, p, q);
  else { q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; }
}
BSG_GRID_FN void map_centroid_add(double* s, const double* q) {
  BSG_GRID_EXACT
  s[0] = s[0] + q[0]; s[1] = s[1] + q[1]; s[2] = s[2] + q[2];
}
BSG_GRID_FN void map_centroid_div(const double* s, int count, double* out) {
  BSG_GRID_EXACT
  const double k = (double)count;
  out[0] = s[0] / k; out[1] = s[1] / k; out[2] = s[2] / k;
}

// ---- host only ----
struct RegistrationMaps {
  std::vector<int32_t> start;      // n_maps + 1
  std::vector<double> points;      // packed xyz
  std::vector<int32_t> count;      // input points per output point
};

// bsgpu_build_registration_maps on one core.  Map m owns scans [map_scan_start[m], map_scan_start[m + 1]); T: 12 per scan or null;
// v: kMapMergeOnly, or positive and finite.  The tables and v are the caller's to check.  false: a finite transformed coordinate with
// |q / v| >= 2^20 (the entry point's BSGPU_ERR_UNSUPPORTED); *out is then unspecified.
inline bool registration_map_serial(int n_maps, const int32_t* map_scan_start, const int32_t* scan_start, const double* points, const double* T,
                                    double v, RegistrationMaps* out) {
  out->start.assign((size_t)n_maps + 1, 0);
  out->points.clear(); out->count.clear();
  std::vector<double> tq;
  std::vector<uint64_t> key;
  std::vector<int32_t> order;
  for (int m = 0; m < n_maps; ++m) {
    tq.clear(); key.clear();
    int bad = 0;
    for (int s = map_scan_start[m]; s < map_scan_start[m + 1]; ++s) {
      for (int i = scan_start[s]; i < scan_start[s + 1]; ++i) {
        double q[3];
        map_transform(T ? T + 12 * (size_t)s : nullptr, points + 3 * (size_t)i, q);
        tq.insert(tq.end(), q, q + 3);
        if (v != kMapMergeOnly) key.push_back(map_point_key(q, v, &bad));
      }
    }
    if (bad) return false;
    const size_t n = tq.size() / 3;
    if (v == kMapMergeOnly) {
      out->points.insert(out->points.end(), tq.begin(), tq.end());
      out->count.insert(out->count.end(), n, 1);
    } else {
      order.resize(n);
      for (size_t i = 0; i < n; ++i) order[i] = (int32_t)i;
      std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
      for (size_t at = 0; at < n && key[(size_t)order[at]] != kMapDropped;) {
        const uint64_t k = key[(size_t)order[at]];
        double s[3] = {0.0, 0.0, 0.0}, c[3];
        int count = 0;
        for (; at < n && key[(size_t)order[at]] == k; ++at, ++count) map_centroid_add(s, &tq[3 * (size_t)order[at]]);
        map_centroid_div(s, count, c);
        out->points.insert(out->points.end(), c, c + 3);
        out->count.push_back(count);
      }
    }
    out->start[(size_t)m + 1] = (int32_t)out->count.size();
  }
  return true;
}
}  // namespace bsg
