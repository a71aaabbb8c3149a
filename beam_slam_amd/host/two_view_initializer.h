// bs_models::TwoViewInitializer — steps 1 and 2 of bs_models::vision::ComputePathWithVision (bs_models/src/lib/vision/utils.cpp:15-115)
// with the seven-point RANSAC, the triangulation of every match and the validity gate on the device, in one call
// (bsgpu_relative_pose_ransac):
//   * the matches are the landmark ids of the last image that the first image holds too, in ascending id order (:28-41);
//   * the pixels are truncated to integers when truncate_pixels is set: the reference casts to Eigen::Vector2i (:34-36);
//   * RelativePoseEstimator::RANSACEstimator(cam, cam, first, last, SEVENPOINT, 100) (:44-47): max_iters = 100, no early termination
//     (prob = 0), libbeam's default inlier threshold of 5 px — recalled, not verified (include/bsgpu.h);
//   * TriangulatePoints, a point valid within 10 px in both images, the pair refused below 80 % valid points (:57-94);
//   * world = first camera: T_WORLD_BASELINK of the first and of the last image (AddCameraPose, :108-109) and the valid points as
//     landmarks (:112-115) — the LandmarkPoints that KeyframeRansacLocalizer takes for the keyframes in between.
// The landmark container ([EXT] beam_containers) and the visual map stay with the caller: the maps handed in hold undistorted pixels.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

#include "../../include/bsgpu.h"
#include "bs_common.h"
#include "keyframe_ransac_localizer.h"

// optional in a back-end: without it no pair is initialised (every call counts as failed)
extern "C" int bsgpu_relative_pose_ransac(bsgpu_ctx* ctx, int32_t n_sets, const int32_t* match_start, const double* px_first,
                                          const double* px_last, const int32_t* camera, double prob, double threshold_px,
                                          int32_t max_iters, uint64_t seed, int32_t truncate_pixels, double validate_px,
                                          double min_inlier_ratio, uint8_t* mask, double* T_last_first, double* q_out, double* p_out,
                                          double* points, uint8_t* valid_mask, double* inlier_ratio, int32_t* pair_valid,
                                          int32_t* n_inliers, int32_t* n_iters, int32_t* best_sample, int32_t* status) __attribute__((weak));

namespace bs_models {

struct TwoViewInitializerParams {
  int32_t max_iters = 100;           // utils.cpp:46
  double confidence = 0.0;           // 0: libbeam's fixed loop as recalled; inside (0, 1): early termination
  double inlier_threshold_px = 5.0;  // libbeam's default, recalled
  double validate_px = 10.0;         // utils.cpp:70-78
  double min_inlier_ratio = 0.8;     // utils.cpp:88
  bool truncate_pixels = true;       // cast<int>() (utils.cpp:34-36)
  uint64_t seed = 0;                 // the sampler's (libbeam's generator is not reproduced)
};

struct TwoViewResult {
  bool has_value = false;                         // false: status not OK, the pair refused by the gate, or the back-end call failed
  bs_math::Mat<4, 4> T_WORLD_BASELINK_first;      // identity when has_value is false
  bs_math::Mat<4, 4> T_WORLD_BASELINK_last;
  LandmarkPoints landmarks;                       // the valid points, world = first camera
  std::vector<uint64_t> matched_ids;              // ascending
  std::vector<uint64_t> inlier_ids;               // the best model's inliers at the RANSAC threshold, ascending
  double inlier_ratio = 0.0;
  int32_t n_inliers = 0, n_iters = 0;
  int32_t pair_valid = 0;
  int32_t status = -1;                            // BSGPU_RANSAC_*; -1: the back-end call failed
};

class TwoViewInitializer {
 public:
  // ctx: a context with the camera table set; camera: the index of the images' camera in it
  TwoViewInitializer(bsgpu_ctx* ctx, int32_t camera, const TwoViewInitializerParams& params = {})
      : ctx_(ctx), camera_(camera), params_(params) {}

  TwoViewResult Initialize(const KeyframePixels& first, const KeyframePixels& last) const {
    TwoViewResult r;
    r.T_WORLD_BASELINK_first = bs_math::Mat<4, 4>::Identity();
    r.T_WORLD_BASELINK_last = bs_math::Mat<4, 4>::Identity();
    std::vector<double> p0, p1;
    for (const auto& [id, pixel] : last) {
      const auto it = first.find(id);
      if (it == first.end()) continue;
      r.matched_ids.push_back(id);
      for (int a = 0; a < 2; ++a) {
        p0.push_back(params_.truncate_pixels ? std::trunc(it->second[a]) : it->second[a]);
        p1.push_back(params_.truncate_pixels ? std::trunc(pixel[a]) : pixel[a]);
      }
    }
    const size_t n = r.matched_ids.size();
    const int32_t start[2] = {0, (int32_t)n};
    std::vector<uint8_t> mask(n + 1, 0), valid(n + 1, 0);
    std::vector<double> pts(3 * n + 3, 0.0);
    double q[8], p[6];
    p0.push_back(0.0); p1.push_back(0.0);   // (never read: non-null data() for a call without matches)
    int rc = BSGPU_ERR_UNSUPPORTED;
    if (bsgpu_relative_pose_ransac)
      rc = bsgpu_relative_pose_ransac(ctx_, 1, start, p0.data(), p1.data(), &camera_, params_.confidence, params_.inlier_threshold_px,
                                      params_.max_iters, params_.seed, params_.truncate_pixels ? 1 : 0, params_.validate_px,
                                      params_.min_inlier_ratio, mask.data(),
                                      nullptr, q, p, pts.data(), valid.data(), &r.inlier_ratio, &r.pair_valid, &r.n_inliers, &r.n_iters,
                                      nullptr, &r.status);
    if (rc != BSGPU_OK) { r.status = -1; return r; }
    for (size_t i = 0; i < n; ++i)
      if (mask[i] != 0) r.inlier_ids.push_back(r.matched_ids[i]);
    if (r.status != BSGPU_RANSAC_OK || r.pair_valid == 0) return r;
    r.has_value = true;
    for (int v = 0; v < 2; ++v) {
      bs_math::Mat<4, 4>& T = v == 0 ? r.T_WORLD_BASELINK_first : r.T_WORLD_BASELINK_last;
      const bs_math::Mat3 R = bs_math::quatToRot({q[4 * v], q[4 * v + 1], q[4 * v + 2], q[4 * v + 3]});
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T(i, j) = R(i, j);
        T(i, 3) = p[3 * v + i];
      }
    }
    for (size_t i = 0; i < n; ++i)
      if (valid[i] != 0) r.landmarks[r.matched_ids[i]] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    return r;
  }

 private:
  bsgpu_ctx* ctx_;
  int32_t camera_;
  TwoViewInitializerParams params_;
};

}  // namespace bs_models
