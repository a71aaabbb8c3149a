// bs_models::KeyframeRansacLocalizer — the per-keyframe loop of bs_models::vision::ComputePathWithVision
// (bs_models/src/lib/vision/utils.cpp:143-188) with the beam_cv::AbsolutePoseEstimator::RANSACEstimator call itself on the device,
// for ALL keyframes in one call (bsgpu_absolute_pose_ransac).  The loop is serial in the reference but its iterations are
// independent: the landmark points do not change between them (nothing is optimised before :197).
//   * the pairs of a keyframe are the landmark ids present in both the landmark map and the frame, in ascending id order
//     (:153-165; ids_in_frame);
//   * the pixels are truncated to integers when truncate_pixels is set: the reference casts to Eigen::Vector2i (:158-159);
//   * RANSACEstimator(camera_model, pixels, points, 100) (:168): max_iters = 100, no early termination (prob = 0), and libbeam's
//     default inlier threshold of 5 px — recalled, not verified (include/bsgpu.h);
//   * T_WORLD_BASELINK of the keyframe (:172, AddCameraPose(InvertTransform(T_CAMERA_WORLD_est)) with the camera-to-baselink
//     extrinsic applied as in visual_odometry.cpp:252-253).
// A frame without a model (fewer than 4 pairs, or no solution with 4 inliers) reports "no pose" instead of inventing one; what
// libbeam returns there cannot be read here.  The landmark container ([EXT] beam_containers) and the visual map stay with the
// caller: the maps handed in hold undistorted pixels and world points.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

#include "../../include/bsgpu.h"
#include "bs_common.h"

// optional in a back-end: without it no keyframe gets a pose (every call counts as failed)
extern "C" int bsgpu_absolute_pose_ransac(bsgpu_ctx* ctx, int32_t n_frames, const int32_t* obs_start, const double* pixels,
                                          const double* points, const int32_t* camera, double prob, double threshold_px,
                                          int32_t max_iters, uint64_t seed, int32_t truncate_pixels, uint8_t* mask, double* q_out,
                                          double* p_out, double* T_cam_world, int32_t* n_inliers, int32_t* n_iters, int32_t* best_sample,
                                          int32_t* status) __attribute__((weak));

namespace bs_models {

using KeyframePixels = std::map<uint64_t, std::array<double, 2>>;   // landmark id -> (undistorted) pixel
using LandmarkPoints = std::map<uint64_t, std::array<double, 3>>;   // landmark id -> world point

struct KeyframeRansacLocalizerParams {
  int32_t max_iters = 100;          // utils.cpp:169
  double confidence = 0.0;          // 0: libbeam's fixed loop as recalled; inside (0, 1): early termination
  double inlier_threshold_px = 5.0; // libbeam's default, recalled
  bool truncate_pixels = true;      // cast<int>() (utils.cpp:159)
  uint64_t seed = 0;                // the sampler's (libbeam's generator is not reproduced)
};

struct KeyframePose {
  bool has_pose = false;                                          // false: fewer than 4 pairs, no model, or the back-end call failed
  bs_math::Mat<4, 4> T_WORLD_BASELINK;                            // identity when has_pose is false
  std::vector<uint64_t> ids_in_frame;                             // ascending
  std::vector<uint64_t> inlier_ids;                               // the best model's inliers, ascending
  int32_t n_inliers = 0, n_iters = 0;
  int32_t status = -1;                                            // BSGPU_RANSAC_*; -1: the back-end call failed
};

class KeyframeRansacLocalizer {
 public:
  // ctx: a context with the camera table set; camera: the index of the keyframes' camera in it
  KeyframeRansacLocalizer(bsgpu_ctx* ctx, int32_t camera, const KeyframeRansacLocalizerParams& params = {})
      : ctx_(ctx), camera_(camera), params_(params) {}

  // every keyframe at once: one device call; keyframe k draws its samples from stream (seed, k)
  std::vector<KeyframePose> Localize(const LandmarkPoints& landmarks, const std::vector<const KeyframePixels*>& keyframes) const {
    const int32_t F = (int32_t)keyframes.size();
    std::vector<KeyframePose> out(F);
    std::vector<int32_t> start(1, 0), cam(F, camera_), status(F, -1), n_inl(F, 0), n_it(F, 0);
    std::vector<double> pix, pts, q(4 * (size_t)F + 1), p(3 * (size_t)F + 1);
    for (int32_t k = 0; k < F; ++k) {
      out[k].T_WORLD_BASELINK = bs_math::Mat<4, 4>::Identity();
      for (const auto& [id, pixel] : *keyframes[k]) {
        const auto it = landmarks.find(id);
        if (it == landmarks.end()) continue;
        out[k].ids_in_frame.push_back(id);
        for (int a = 0; a < 2; ++a) pix.push_back(params_.truncate_pixels ? std::trunc(pixel[a]) : pixel[a]);
        pts.insert(pts.end(), it->second.begin(), it->second.end());
      }
      start.push_back((int32_t)(pix.size() / 2));
    }
    std::vector<uint8_t> mask(pix.size() / 2 + 1, 0);
    pix.push_back(0.0); pts.push_back(0.0);   // (never read: non-null data() for a call without pairs)
    int rc = BSGPU_ERR_UNSUPPORTED;
    if (bsgpu_absolute_pose_ransac && F > 0)
      rc = bsgpu_absolute_pose_ransac(ctx_, F, start.data(), pix.data(), pts.data(), cam.data(), params_.confidence,
                                      params_.inlier_threshold_px, params_.max_iters, params_.seed, 0, mask.data(), q.data(), p.data(),
                                      nullptr, n_inl.data(), n_it.data(), nullptr, status.data());
    for (int32_t k = 0; k < F; ++k) {
      KeyframePose& r = out[k];
      if (rc != BSGPU_OK) continue;
      r.status = status[k];
      r.n_inliers = n_inl[k]; r.n_iters = n_it[k];
      if (r.status != BSGPU_RANSAC_OK) continue;
      r.has_pose = true;
      const bs_math::Mat3 R = bs_math::quatToRot({q[4 * (size_t)k], q[4 * (size_t)k + 1], q[4 * (size_t)k + 2], q[4 * (size_t)k + 3]});
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) r.T_WORLD_BASELINK(i, j) = R(i, j);
        r.T_WORLD_BASELINK(i, 3) = p[3 * (size_t)k + i];
      }
      for (size_t i = 0; i < r.ids_in_frame.size(); ++i)
        if (mask[(size_t)start[k] + i] != 0) r.inlier_ids.push_back(r.ids_in_frame[i]);
    }
    return out;
  }

 private:
  bsgpu_ctx* ctx_;
  int32_t camera_;
  KeyframeRansacLocalizerParams params_;
};

}  // namespace bs_models
