// bs_models::scan_registration::RegistrationMap — a stand-in for the reference's RegistrationMap
// (bs_models/include/bs_models/scan_registration/registration_map.h, src/lib/scan_registration/registration_map.cpp) as
// ScanToMapLoamRegistration uses it (scan_to_map_registration.cpp:168-197), over bsgpu_build_registration_maps:
//   * SetMapSize / AddPointCloud keep the last map_size scans by stamp; trimming the oldest stays here (registration_map.cpp:31-50, 72-94);
//   * UpdateScan replaces a scan's T_Map_Scan unless ArePosesEqual finds the new pose within both thresholds (:147-174);
//   * GetPointCloudMap is ONE call with one map (:96-107); GetLoamCloudMap is ONE call with two maps — every scan's strong edges, then
//     every scan's strong surfaces — and returns loam_matcher.h's LoamPointCloud (:109-126);
//   * GetScanPose, NumScans, MapSize, Empty, Clear as there.
// The library's choice: a scan is stored in its own frame with its current T_Map_Scan and transformed on every Get — the reference
// stores transformed float clouds and re-transforms them incrementally in UpdateScan.  Out of scope: publishing, saving, and the
// graph-message updates.  [EXT] beam::ArePosesEqual is libbeam's and not in the reference checkout: its rule below is RECALLED.
// With device >= 0 the entry point of the back-end is called (without one in the back-end, or when the call fails, ok() is false and
// the clouds are empty).  With device < 0 the same contract runs on one core through the shared header (csrc/registration_map.h:
// registration_map_serial), which needs nothing of HIP.
#pragma once
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

#include "../../include/bsgpu.h"
#include "../csrc/registration_map.h"
#include "loam_matcher.h"

// optional in a back-end: without it no map is built on a device
extern "C" int bsgpu_build_registration_maps(int device, int32_t n_maps, const int32_t* map_scan_start, const int32_t* scan_start,
                                             const double* points, const double* T_map_scan, double voxel_size, int32_t* map_start,
                                             double* map_points, int32_t* map_count) __attribute__((weak));

namespace bs_models { namespace scan_registration {

// [EXT] beam::ArePosesEqual, recalled: the angle of R1^T R2 within the rotation threshold AND |t1 - t2| within the translation one
inline bool ArePosesEqual(const LoamMat4& T1, const LoamMat4& T2, double rotation_threshold_deg, double translation_threshold_m) {
  double trace = 0.0, d2 = 0.0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) trace += T1(j, i) * T2(j, i);      // trace(R1^T R2)
    d2 += (T1(i, 3) - T2(i, 3)) * (T1(i, 3) - T2(i, 3));
  }
  const double c = 0.5 * (trace - 1.0), angle_deg = std::acos(c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c)) * 180.0 / 3.14159265358979323846;
  return angle_deg <= rotation_threshold_deg && std::sqrt(d2) <= translation_threshold_m;
}

class RegistrationMap {
 public:
  explicit RegistrationMap(int device = 0) : device_(device) {}

  void SetMapSize(int map_size) {
    map_size_ = map_size;
    Trim();
  }
  void SetVoxelDownsampleSize(double downsample_voxel_size) { voxel_ = downsample_voxel_size; }      // -1: merge only
  int MapSize() const { return map_size_; }
  int NumScans() const { return (int)scans_.size(); }
  bool Empty() const { return scans_.empty(); }
  void Clear() { scans_.clear(); }
  bool ok() const { return ok_; }      // the last Get: false without a back-end, or when the call failed

  // cloud: the whole scan, packed xyz in the scan's frame; loam_cloud: its strong features in the same frame
  void AddPointCloud(const std::vector<double>& cloud, const LoamPointCloud& loam_cloud, uint64_t stamp_ns, const LoamMat4& T_Map_Scan) {
    scans_[stamp_ns] = Scan{cloud, loam_cloud, T_Map_Scan};
    Trim();
  }
  bool UpdateScan(uint64_t stamp_ns, const LoamMat4& T_Map_Scan, double rotation_threshold_deg = 0.5, double translation_threshold_m = 0.005) {
    const auto it = scans_.find(stamp_ns);
    if (it == scans_.end()) return false;
    if (ArePosesEqual(T_Map_Scan, it->second.T_Map_Scan, rotation_threshold_deg, translation_threshold_m)) return false;
    it->second.T_Map_Scan = T_Map_Scan;
    return true;
  }
  bool GetScanPose(uint64_t stamp_ns, LoamMat4& T_Map_Scan) const {
    const auto it = scans_.find(stamp_ns);
    if (it == scans_.end()) return false;
    T_Map_Scan = it->second.T_Map_Scan;
    return true;
  }

  std::vector<double> GetPointCloudMap() const {
    std::vector<const std::vector<double>*> clouds;
    for (const auto& s : scans_) clouds.push_back(&s.second.cloud);
    std::vector<std::vector<double>> out = Build(clouds, 1);
    return out.empty() ? std::vector<double>() : out[0];
  }
  LoamPointCloud GetLoamCloudMap() const {
    std::vector<const std::vector<double>*> clouds;
    for (const auto& s : scans_) clouds.push_back(&s.second.loam.edges);
    for (const auto& s : scans_) clouds.push_back(&s.second.loam.surfaces);
    std::vector<std::vector<double>> out = Build(clouds, 2);
    LoamPointCloud map;
    if (out.size() == 2) { map.edges = out[0]; map.surfaces = out[1]; }
    return map;
  }

 private:
  struct Scan {
    std::vector<double> cloud;
    LoamPointCloud loam;
    LoamMat4 T_Map_Scan;
  };

  void Trim() {
    while (map_size_ >= 0 && (int)scans_.size() > map_size_) scans_.erase(scans_.begin());      // the oldest stamp goes first
  }

  // clouds: n_maps groups of one cloud per stored scan, in stamp order -> per map its packed xyz (empty: the call failed)
  std::vector<std::vector<double>> Build(const std::vector<const std::vector<double>*>& clouds, int n_maps) const {
    ok_ = false;
    std::vector<int32_t> map_scan_start(1, 0), scan_start(1, 0);
    std::vector<double> pts, T;
    for (int m = 0; m < n_maps; ++m) {
      size_t k = 0;
      for (const auto& s : scans_) {
        const std::vector<double>& c = *clouds[(size_t)m * scans_.size() + k++];
        pts.insert(pts.end(), c.begin(), c.end());
        scan_start.push_back((int32_t)(pts.size() / 3));
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) T.push_back(s.second.T_Map_Scan(i, j));
      }
      map_scan_start.push_back((int32_t)(scan_start.size() - 1));
    }
    const size_t n = pts.size() / 3;
    std::vector<std::vector<double>> out;
    if (!(voxel_ == bsg::kMapMergeOnly) && !(voxel_ > 0.0 && std::isfinite(voxel_))) return out;
    for (double x : T) if (!std::isfinite(x)) return out;
    if (n > (size_t)bsg::kMapMaxPoints) return out;
    std::vector<int32_t> start((size_t)n_maps + 1, 0);
    std::vector<double> xyz;
    if (device_ >= 0) {
      if (!bsgpu_build_registration_maps) return out;
      pts.push_back(0.0); T.push_back(0.0);      // (never read: non-null data() for empty maps)
      xyz.assign(3 * n + 3, 0.0);
      if (bsgpu_build_registration_maps(device_, n_maps, map_scan_start.data(), scan_start.data(), pts.data(), T.data(), voxel_, start.data(),
                                        xyz.data(), nullptr) != BSGPU_OK)
        return out;
    } else {
      bsg::RegistrationMaps R;
      if (!bsg::registration_map_serial(n_maps, map_scan_start.data(), scan_start.data(), pts.data(), T.data(), voxel_, &R)) return out;
      start = R.start;
      xyz = R.points;
    }
    for (int m = 0; m < n_maps; ++m) out.emplace_back(xyz.begin() + 3 * (size_t)start[(size_t)m], xyz.begin() + 3 * (size_t)start[(size_t)m + 1]);
    ok_ = true;
    return out;
  }

  int device_;
  int map_size_ = 10;
  double voxel_ = -1.0;
  std::map<uint64_t, Scan> scans_;
  mutable bool ok_ = false;
};

}}  // namespace bs_models::scan_registration
