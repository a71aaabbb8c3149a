// bs_models::FrameLocalizer — the decisions VisualOdometry::LocalizeFrame (bs_models/src/visual_odometry.cpp:217-300) takes around
// its pose refinement, with the refinement itself on the device (bsgpu_localize_frames, one call for any number of frames):
//   * the required_points_to_refine gate (:230; vo/vo_params.json:5 ships 20);
//   * T_CAMERA_WORLD_est = (T_WORLD_BASELINK T_cam_baselink^-1)^-1 in, T_WORLD_BASELINK = T_CAMERA_WORLD^-1 T_cam_baselink out (:233-254)
//     — the device refines T_WORLD_BASELINK itself, both forms are returned;
//   * the covariance in (x, y, z, roll, pitch, yaw) order (:243-247): bsgpu_localize_frames already hands [p, q tangent] on the
//     baselink pose; libbeam's RefinePose hands [rotation, translation] on T_CAMERA_WORLD's parameters, and SwapRotationTranslation
//     is LocalizeFrame's block swap for a matrix in that order;
//   * the fallback on any failure (:262-284): the initial pose and invalid_localization_covariance_weight * I
//     (vo/vo_params.json:10 ships 1e-1).
// The validator (vo_localization_validation.cpp:12-30) is the caller's: an optional callback receives T_init_refined, the covariance
// and the average reprojection.  libbeam's PoseRefinement is not in the reference checkout: the loss, its scale, the pixel weight and
// the LM options below are UNPINNED defaults (the reference constructs PoseRefinement(0.02, true, 0.2), visual_odometry.cpp:72, whose
// meaning cannot be read here).
#pragma once
#include <array>
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/bsgpu.h"
#include "bs_common.h"

// optional in a back-end: without it every refinement counts as failed (the fallback)
extern "C" int bsgpu_localize_frames(bsgpu_ctx* ctx, int32_t n_frames, const int32_t* obs_start, const double* pixels, const double* points,
                                     const int32_t* lm_block, const int32_t* camera, const double* q_init, const double* p_init,
                                     int32_t loss_kind, double loss_a, double sqrt_info, int32_t truncate_pixels, int32_t min_points,
                                     int32_t image_width, int32_t image_height, const bsgpu_options* options, double* q_out, double* p_out,
                                     double* cov_out, double* avg_reproj, double* final_cost, int32_t* iterations, int32_t* status)
    __attribute__((weak));

namespace bs_models {

using bs_math::Mat;
using bs_math::Mat3;
using bs_math::Quat;
using bs_math::Vec3;

struct FrameLocalizerParams {
  int required_points_to_refine = 20;                  // vo/vo_params.json:5
  double invalid_localization_covariance_weight = 0.1; // vo/vo_params.json:10
  int32_t loss_kind = BSGPU_LOSS_CAUCHY;               // unpinned (libbeam PoseRefinement)
  double loss_a = 1.0, sqrt_info = 1.0;                // unpinned
  bool truncate_pixels = true;                         // GetPixelPointPairs' cast<int>() (visual_odometry.cpp:612-650)
  int32_t image_width = 0, image_height = 0;           // the camera model's image (ComputeAverageReprojection's bounds); 0: none
};

struct FrameInput {
  std::vector<std::array<double, 2>> pixels;
  std::vector<Vec3> points;                            // world frame
  Mat<4, 4> T_WORLD_BASELINK_init;                     // the frame's initial estimate (T_WORLD_BASELINKcur)
};

struct FrameLocalization {
  Mat<4, 4> T_WORLD_BASELINK, T_CAMERA_WORLD;
  Mat<6, 6> covariance;                                // (x, y, z, roll, pitch, yaw)
  double avg_reprojection = 0.0;
  int32_t status = -1;                                 // bsgpu_localize_frames' status (-1: the back-end call failed)
  bool localized = false;                              // refinement and validation passed; otherwise the fallback was applied
};

inline Mat<4, 4> InvertTransform(const Mat<4, 4>& T) {
  Mat<4, 4> o;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o(i, j) = T(j, i);
    o(i, 3) = -(T(0, i) * T(0, 3) + T(1, i) * T(1, 3) + T(2, i) * T(2, 3));
  }
  o(3, 3) = 1.0;
  return o;
}
inline Quat RotToQuat(const Mat<4, 4>& T) {
  const double tr = T(0, 0) + T(1, 1) + T(2, 2);
  Quat q;
  if (tr > 0.0) {
    const double s = 2.0 * std::sqrt(1.0 + tr);
    q = {0.25 * s, (T(2, 1) - T(1, 2)) / s, (T(0, 2) - T(2, 0)) / s, (T(1, 0) - T(0, 1)) / s};
  } else if (T(0, 0) > T(1, 1) && T(0, 0) > T(2, 2)) {
    const double s = 2.0 * std::sqrt(1.0 + T(0, 0) - T(1, 1) - T(2, 2));
    q = {(T(2, 1) - T(1, 2)) / s, 0.25 * s, (T(0, 1) + T(1, 0)) / s, (T(0, 2) + T(2, 0)) / s};
  } else if (T(1, 1) > T(2, 2)) {
    const double s = 2.0 * std::sqrt(1.0 + T(1, 1) - T(0, 0) - T(2, 2));
    q = {(T(0, 2) - T(2, 0)) / s, (T(0, 1) + T(1, 0)) / s, 0.25 * s, (T(1, 2) + T(2, 1)) / s};
  } else {
    const double s = 2.0 * std::sqrt(1.0 + T(2, 2) - T(0, 0) - T(1, 1));
    q = {(T(1, 0) - T(0, 1)) / s, (T(0, 2) + T(2, 0)) / s, (T(1, 2) + T(2, 1)) / s, 0.25 * s};
  }
  return bs_math::quatNormalized(q);
}
inline Mat<4, 4> PoseToTransform(const Quat& q, const Vec3& p) {
  const Mat3 R = bs_math::quatToRot(q);
  Mat<4, 4> T = Mat<4, 4>::Identity();
  for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) T(i, j) = R(i, j); T(i, 3) = p[i]; }
  return T;
}
// LocalizeFrame's reorder (visual_odometry.cpp:243-247): the 3x3 blocks of a [a, b] covariance as [b, a] (an involution)
inline Mat<6, 6> SwapRotationTranslation(const Mat<6, 6>& c) {
  Mat<6, 6> o;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) o((i + 3) % 6, (j + 3) % 6) = c(i, j);
  return o;
}

class FrameLocalizer {
 public:
  using Validator = std::function<bool(const Mat<4, 4>& T_init_refined, const Mat<6, 6>& covariance, double avg_reprojection)>;

  // ctx: a context with the camera table set (points-only calls need nothing else; a context is single-caller)
  FrameLocalizer(bsgpu_ctx* ctx, int32_t camera, const Mat<4, 4>& T_cam_baselink, const FrameLocalizerParams& params = {},
                 const bsgpu_options* options = nullptr)
      : ctx_(ctx), camera_(camera), T_cam_baselink_(T_cam_baselink), params_(params) {
    if (options) options_ = *options; else bsgpu_options_default(&options_);
  }

  // LocalizeFrame for every frame at once: one device call; each frame is decided on its own
  std::vector<FrameLocalization> Localize(const std::vector<FrameInput>& frames, const Validator& validate = nullptr) const {
    const int32_t F = (int32_t)frames.size();
    std::vector<int32_t> start(1, 0), cam(F, camera_), status(F, -1);
    std::vector<double> pix, pts, q0, p0, q(4 * (size_t)F), p(3 * (size_t)F), cov(36 * (size_t)F), avg(F);
    for (const FrameInput& f : frames) {
      const size_t n = std::min(f.pixels.size(), f.points.size());
      for (size_t i = 0; i < n; ++i) {
        pix.insert(pix.end(), f.pixels[i].begin(), f.pixels[i].end());
        pts.insert(pts.end(), f.points[i].begin(), f.points[i].end());
      }
      start.push_back(start.back() + (int32_t)n);
      const Quat qi = RotToQuat(f.T_WORLD_BASELINK_init);
      q0.insert(q0.end(), qi.begin(), qi.end());
      for (int i = 0; i < 3; ++i) p0.push_back(f.T_WORLD_BASELINK_init(i, 3));
    }
    int rc = BSGPU_ERR_UNSUPPORTED;
    if (bsgpu_localize_frames && F > 0)
      rc = bsgpu_localize_frames(ctx_, F, start.data(), pix.data(), pts.data(), nullptr, cam.data(), q0.data(), p0.data(), params_.loss_kind,
                                 params_.loss_a, params_.sqrt_info, params_.truncate_pixels ? 1 : 0, params_.required_points_to_refine,
                                 params_.image_width, params_.image_height, &options_, q.data(), p.data(), cov.data(), avg.data(),
                                 nullptr, nullptr, status.data());
    std::vector<FrameLocalization> out(F);
    for (int32_t f = 0; f < F; ++f) {
      FrameLocalization& r = out[f];
      r.status = rc == BSGPU_OK ? status[f] : -1;
      bool ok = r.status == 0;
      if (ok) {
        r.T_WORLD_BASELINK = PoseToTransform({q[4 * f], q[4 * f + 1], q[4 * f + 2], q[4 * f + 3]}, {p[3 * f], p[3 * f + 1], p[3 * f + 2]});
        for (int i = 0; i < 36; ++i) r.covariance.a[i] = cov[36 * (size_t)f + i];
        r.avg_reprojection = avg[f];
        if (validate)
          ok = validate(InvertTransform(frames[f].T_WORLD_BASELINK_init) * r.T_WORLD_BASELINK, r.covariance, r.avg_reprojection);
      }
      if (!ok) {   // the fallback: the frame's initial estimate, invalid_localization_covariance_weight * I
        r.T_WORLD_BASELINK = frames[f].T_WORLD_BASELINK_init;
        r.covariance = Mat<6, 6>::Identity();
        for (double& v : r.covariance.a) v *= params_.invalid_localization_covariance_weight;
      }
      r.T_CAMERA_WORLD = InvertTransform(r.T_WORLD_BASELINK * InvertTransform(T_cam_baselink_));
      r.localized = ok;
    }
    return out;
  }

 private:
  bsgpu_ctx* ctx_;
  int32_t camera_;
  Mat<4, 4> T_cam_baselink_;
  FrameLocalizerParams params_;
  bsgpu_options options_;
};

}  // namespace bs_models
