// bs_models::TrackOutlierFilter — the track screening VisualOdometry::AddMeasurementsToContainer
// (bs_models/src/visual_odometry.cpp:481-527) runs on every incoming camera measurement before the frame is localised, with the
// cv::findEssentialMat call itself on the device (bsgpu_essential_ransac, one call for any number of frame pairs):
//   * the matches are the landmark ids measured in BOTH frames, in ascending id order — the reference iterates a
//     std::map<uint64_t, Eigen::Vector2d> of the previous frame's measurements (:503-514);
//   * the pixels are truncated to integers when truncate_pixels is set: the reference undistorts `measurement.cast<int>()` into an
//     Eigen::Vector2i (:491-495), so what reaches OpenCV are whole pixels;
//   * every match the mask rules out is erased from the CURRENT frame (:521-526); fewer than 5 matches, or no model at all, erase
//     nothing — the reference's loop then runs over an empty mask;
//   * prob = 0.99 (:518) and track_outlier_pixel_threshold = 1.0 (vo/vo_params.json:6).
// Undistortion ([EXT] beam_calibration::CameraModel::UndistortPixel) and the landmark container ([EXT] beam_containers) stay with the
// caller: the maps handed in hold undistorted pixels, the ids handed back are the caller's to erase.  SLAMInitialization makes the
// same call (bs_models/src/slam_initialization.cpp:882-910).  What cv::findEssentialMat does is recalled, not verified
// (include/bsgpu.h).
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

#include "../../include/bsgpu.h"

// optional in a back-end: without it nothing is screened (every call counts as failed and erases nothing)
extern "C" int bsgpu_essential_ransac(bsgpu_ctx* ctx, int32_t n_sets, const int32_t* match_start, const double* px_prev, const double* px_cur,
                                      const double* K, double prob, double threshold_px, int32_t max_iters, uint64_t seed, uint8_t* mask,
                                      double* E, int32_t* n_inliers, int32_t* n_iters, int32_t* best_sample, int32_t* status)
    __attribute__((weak));

namespace bs_models {

using PixelMap = std::map<uint64_t, std::array<double, 2>>;   // landmark id -> (undistorted) pixel

struct TrackOutlierFilterParams {
  double fx = 0.0, fy = 0.0, cx = 0.0, cy = 0.0;    // K_ (visual_odometry.cpp:66-69)
  double track_outlier_pixel_threshold = 1.0;        // vo/vo_params.json:6
  double confidence = 0.99;                          // visual_odometry.cpp:518
  int32_t max_iters = 1000;                          // OpenCV's default
  bool truncate_pixels = true;                       // cast<int>() (:491), Eigen::Vector2i (:493)
  uint64_t seed = 0;                                 // the sampler's (OpenCV's generator is not reproduced)
};

struct FramePair {
  const PixelMap* prev;
  const PixelMap* cur;
};

struct TrackScreening {
  std::vector<uint64_t> matched_ids;                 // ascending
  std::vector<uint64_t> erase;                       // the ids to erase from the current frame, ascending
  std::array<double, 9> E{};                         // row-major, on normalised coordinates; zeros without a model
  int32_t n_inliers = 0, n_iters = 0;
  int32_t status = -1;                               // BSGPU_RANSAC_*; -1: the back-end call failed (nothing erased)
};

class TrackOutlierFilter {
 public:
  TrackOutlierFilter(bsgpu_ctx* ctx, const TrackOutlierFilterParams& params) : ctx_(ctx), params_(params) {}

  // the screening of every frame pair at once: one device call; pair k draws its samples from stream (seed, k)
  std::vector<TrackScreening> Screen(const std::vector<FramePair>& pairs) const {
    const int32_t S = (int32_t)pairs.size();
    std::vector<TrackScreening> out(S);
    std::vector<int32_t> start(1, 0), status(S, -1), n_inl(S, 0), n_it(S, 0);
    std::vector<double> p1, p2, K, E(9 * (size_t)S, 0.0);
    for (int32_t k = 0; k < S; ++k) {
      for (const auto& [id, pixel] : *pairs[k].prev) {
        const auto it = pairs[k].cur->find(id);
        if (it == pairs[k].cur->end()) continue;
        out[k].matched_ids.push_back(id);
        for (int a = 0; a < 2; ++a) {
          p1.push_back(params_.truncate_pixels ? std::trunc(pixel[a]) : pixel[a]);
          p2.push_back(params_.truncate_pixels ? std::trunc(it->second[a]) : it->second[a]);
        }
      }
      start.push_back((int32_t)(p1.size() / 2));
      K.insert(K.end(), {params_.fx, params_.fy, params_.cx, params_.cy});
    }
    std::vector<uint8_t> mask(p1.size() / 2 + 1, 1);
    p1.push_back(0.0); p2.push_back(0.0);   // (never read: non-null data() for a call without matches)
    int rc = BSGPU_ERR_UNSUPPORTED;
    if (bsgpu_essential_ransac && S > 0)
      rc = bsgpu_essential_ransac(ctx_, S, start.data(), p1.data(), p2.data(), K.data(), params_.confidence,
                                  params_.track_outlier_pixel_threshold, params_.max_iters, params_.seed, mask.data(), E.data(), n_inl.data(),
                                  n_it.data(), nullptr, status.data());
    for (int32_t k = 0; k < S; ++k) {
      TrackScreening& r = out[k];
      if (rc != BSGPU_OK) continue;
      r.status = status[k];
      r.n_inliers = n_inl[k]; r.n_iters = n_it[k];
      for (int e = 0; e < 9; ++e) r.E[e] = E[9 * (size_t)k + e];
      for (size_t i = 0; i < r.matched_ids.size(); ++i)
        if (mask[(size_t)start[k] + i] == 0) r.erase.push_back(r.matched_ids[i]);
    }
    return out;
  }

  TrackScreening Screen(const PixelMap& prev, const PixelMap& cur) const { return Screen({FramePair{&prev, &cur}})[0]; }

 private:
  bsgpu_ctx* ctx_;
  TrackOutlierFilterParams params_;
};

}  // namespace bs_models
