// bs_models::scan_registration::LoamFeatureExtractor — a stand-in for the interface of libbeam's LoamFeatureExtractor as the reference
// uses it: feature_extractor->ExtractFeatures(cloud) -> LoamPointCloud in ScanPose's constructors (bs_models/src/lib/lidar/
// scan_pose.cpp:34-37, 63-66, 92-95), over bsgpu_extract_loam_features:
//   * ExtractFeatures(cloud) takes one scan as packed xyz (and, optionally, its ring field) and returns loam_matcher.h's LoamPointCloud —
//     edges.strong and surfaces.strong, what every shipped matcher reads — extended by the weak clouds (LESS_SHARP, LESS_FLAT; disjoint
//     from the strong ones);
//   * ExtractAll(clouds) extracts a batch of scans — the scans that arrived since the last optimisation, or a bag's — as ONE call.
// With device >= 0 the entry point of the back-end is called (without one in the back-end, or when the call fails, ok stays false and
// the clouds empty).  With device < 0 the same contract runs on one core through the shared header (csrc/loam_features.h:
// loam_extract_serial), which needs nothing of HIP.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/bsgpu.h"
#include "../csrc/loam_features.h"
#include "loam_matcher.h"

// optional in a back-end: without it nothing is extracted on a device
extern "C" int bsgpu_extract_loam_features(int device, int32_t n_scans, const int32_t* scan_start, const double* points, const int32_t* ring,
                                           int32_t number_of_beams, double fov_deg, int32_t vertical_axis, int32_t n_feature_regions,
                                           int32_t curvature_region, int32_t max_corner_sharp, int32_t max_corner_less_sharp,
                                           int32_t max_surface_flat, double surface_curvature_threshold, int32_t downsample_less_flat_features,
                                           int32_t* edge_start, int32_t* edge_index, double* edge_points, int32_t* surf_start, int32_t* surf_index,
                                           double* surf_points, int32_t* weak_edge_start, int32_t* weak_edge_index, double* weak_edge_points,
                                           int32_t* weak_surf_start, int32_t* weak_surf_index, double* weak_surf_points, int32_t* label,
                                           double* curvature) __attribute__((weak));

namespace bs_models { namespace scan_registration {

struct LoamFeatureExtractorParams {      // config/matchers/loam_vlp16.json
  int number_of_beams = 16;
  double fov_deg = 30.0;
  int vertical_axis = BSGPU_AXIS_Z;
  int n_feature_regions = 6, curvature_region = 5, max_corner_sharp = 2, max_corner_less_sharp = 20, max_surface_flat = 4;
  double surface_curvature_threshold = 0.1;
};

struct LoamFeatureCloud : LoamPointCloud {      // edges, surfaces: the strong features
  std::vector<double> weak_edges, weak_surfaces;
  bool ok = false;                              // false: no back-end, or the call failed
};

class LoamFeatureExtractor {
 public:
  explicit LoamFeatureExtractor(int device = 0, const LoamFeatureExtractorParams& params = {}) : device_(device), m_(params) {}

  // cloud: packed xyz; ring (optional): one per point
  LoamFeatureCloud ExtractFeatures(const std::vector<double>& cloud, const std::vector<int32_t>* ring = nullptr) const {
    return ExtractAll({&cloud}, ring ? std::vector<const std::vector<int32_t>*>{ring} : std::vector<const std::vector<int32_t>*>{})[0];
  }

  // rings: empty (every scan by elevation) or one per scan
  std::vector<LoamFeatureCloud> ExtractAll(const std::vector<const std::vector<double>*>& clouds,
                                           const std::vector<const std::vector<int32_t>*>& rings = {}) const {
    const int32_t S = (int32_t)clouds.size();
    std::vector<LoamFeatureCloud> out((size_t)S);
    if (S == 0 || (!rings.empty() && rings.size() != clouds.size())) return out;
    if (device_ >= 0) {
      if (!bsgpu_extract_loam_features) return out;
      std::vector<int32_t> start(1, 0), ring;
      std::vector<double> pts;
      for (int32_t s = 0; s < S; ++s) {
        pts.insert(pts.end(), clouds[s]->begin(), clouds[s]->end());
        start.push_back((int32_t)(pts.size() / 3));
        if (!rings.empty()) {
          if (rings[s]->size() != clouds[s]->size() / 3) return out;
          ring.insert(ring.end(), rings[s]->begin(), rings[s]->end());
        }
      }
      const size_t n = pts.size() / 3;
      pts.push_back(0.0); ring.push_back(0);      // (never read: non-null data() for empty scans)
      // the contract's capacities are all bounded by the points of the call
      std::vector<int32_t> st[4], idx[4];
      std::vector<double> xyz[4];
      for (int k = 0; k < 4; ++k) { st[k].assign((size_t)S + 1, 0); idx[k].assign(n + 1, 0); xyz[k].assign(3 * n + 3, 0.0); }
      if (bsgpu_extract_loam_features(device_, S, start.data(), pts.data(), rings.empty() ? nullptr : ring.data(), m_.number_of_beams, m_.fov_deg,
                                      m_.vertical_axis, m_.n_feature_regions, m_.curvature_region, m_.max_corner_sharp, m_.max_corner_less_sharp,
                                      m_.max_surface_flat, m_.surface_curvature_threshold, 0, st[0].data(), idx[0].data(), xyz[0].data(), st[1].data(),
                                      idx[1].data(), xyz[1].data(), st[2].data(), idx[2].data(), xyz[2].data(), st[3].data(), idx[3].data(),
                                      xyz[3].data(), nullptr, nullptr) != BSGPU_OK)
        return out;
      for (int32_t s = 0; s < S; ++s) {
        std::vector<double>* dst[4] = {&out[(size_t)s].edges, &out[(size_t)s].surfaces, &out[(size_t)s].weak_edges, &out[(size_t)s].weak_surfaces};
        for (int k = 0; k < 4; ++k) dst[k]->assign(xyz[k].begin() + 3 * (size_t)st[k][(size_t)s], xyz[k].begin() + 3 * (size_t)st[k][(size_t)s + 1]);
        out[(size_t)s].ok = true;
      }
    } else {
      if (m_.number_of_beams < 1 || m_.number_of_beams > bsg::kLoamMaxRings || m_.n_feature_regions < 1 || m_.n_feature_regions > bsg::kLoamMaxRegions ||
          m_.curvature_region < 1 || m_.curvature_region > bsg::kLoamMaxCurvatureRegion || !(m_.fov_deg > 0.0) || !(m_.fov_deg < 180.0) ||
          m_.vertical_axis < 0 || m_.vertical_axis > 2 || m_.max_corner_sharp < 0 || m_.max_corner_less_sharp < 0 || m_.max_surface_flat < 0)
        return out;
      bsg::LoamFeatParams P;
      P.beams = m_.number_of_beams; P.regions = m_.n_feature_regions; P.c = m_.curvature_region; P.max_sharp = m_.max_corner_sharp;
      P.max_less_sharp = m_.max_corner_less_sharp; P.max_flat = m_.max_surface_flat; P.axis = m_.vertical_axis; P.threshold = m_.surface_curvature_threshold;
      std::vector<double> bound((size_t)P.beams + 1);
      bsg::loam_feat_bounds(P.beams, m_.fov_deg, bound.data());
      for (int32_t s = 0; s < S; ++s) {
        const std::vector<double>& c = *clouds[s];
        if (!rings.empty() && rings[s]->size() != c.size() / 3) return std::vector<LoamFeatureCloud>((size_t)S);
        bsg::LoamFeatures F;
        if (!bsg::loam_extract_serial((int)(c.size() / 3), c.data(), rings.empty() ? nullptr : rings[s]->data(), P, bound.data(), &F))
          return std::vector<LoamFeatureCloud>((size_t)S);      // (a ring above the cap fails the call, as on the device)
        const std::vector<int32_t>* src[4] = {&F.sharp, &F.flat, &F.less_sharp, &F.less_flat};
        std::vector<double>* dst[4] = {&out[(size_t)s].edges, &out[(size_t)s].surfaces, &out[(size_t)s].weak_edges, &out[(size_t)s].weak_surfaces};
        for (int k = 0; k < 4; ++k)
          for (int32_t i : *src[k]) dst[k]->insert(dst[k]->end(), c.begin() + 3 * (size_t)i, c.begin() + 3 * (size_t)i + 3);
        out[(size_t)s].ok = true;
      }
    }
    return out;
  }

 private:
  int device_;
  LoamFeatureExtractorParams m_;
};

}}  // namespace bs_models::scan_registration
