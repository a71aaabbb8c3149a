// bs_models::InertialAligner — what SLAMInitialization does with its initial path between ComputePathWithVision and the first large
// solve: imu::EstimateParameters (bs_models/src/lib/imu/inertial_alignment.cpp:4-112), the scale gate
// (bs_models/src/slam_initialization.cpp:312-316) and AlignPathAndVelocities (:400-431), on the device for one path or for a batch
// of candidate paths in one call (bsgpu_inertial_alignment).
//   * the path is the reference's std::map<uint64_t, Eigen::Matrix4d>: nanosecond stamps in ascending order, T_WORLD_BASELINK; the
//     quaternion is taken from the rotation block as Eigen::Quaterniond(R) does (beam::TransformMatrixToQuaternionAndTranslation);
//   * the IMU buffer is handed over whole: every path of a batch uses all of it, as every candidate of the reference would;
//   * the defaults are the reference's: excitation 0.25 (inertial_alignment.cpp:84), scale gate [0.02, 1.0] (:313), and
//     bridge_gap = false — frame j's delta starts at its first sample, not at t_{j-1} (include/bsgpu.h);
//   * the result holds what the two reference calls leave behind: gravity, bg, ba = 0 (never estimated, :14), scale, the velocities
//     map and the aligned path; `initialized` is the reference's `return true` (:371), i.e. status BSGPU_ALIGN_OK.
// Nothing is computed on the host: without the entry point in the back-end, or when the call fails, no path is initialised.
#pragma once
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

#include "../../include/bsgpu.h"
#include "bs_common.h"

// optional in a back-end: without it no path is initialised
extern "C" int bsgpu_inertial_alignment(int device, int32_t n_paths, const int32_t* frame_start, const double* t_frame,
                                        const double* q_frame, const double* p_frame, const int32_t* imu_range, const double* t,
                                        const double* w, const double* a, int32_t bridge_gap, double min_excitation, int32_t apply_scale,
                                        double scale_min, double scale_max, double rank_tol, double* gravity, double* bg, double* scale,
                                        double* excitation, int32_t* gyro_rank, double* velocity, double* q_out, double* p_out,
                                        double* v_out, int32_t* status) __attribute__((weak));

namespace bs_models {

using InitPath = std::map<uint64_t, bs_math::Mat<4, 4>>;   // stamp [ns] -> T_WORLD_BASELINK

struct ImuSample { double t; bs_math::Vec3 w, a; };          // stamp [s], gyroscope, accelerometer

struct InertialAlignerParams {
  double min_excitation = 0.25;     // inertial_alignment.cpp:84
  double scale_min = 0.02;          // slam_initialization.cpp:313
  double scale_max = 1.0;
  bool apply_scale = true;          // mode_ == VISUAL && !frame_initializer_ (:312, :321)
  bool bridge_gap = false;          // false: the reference's deltas
  double rank_tol = 1e-10;
};

struct InertialAlignment {
  bool initialized = false;                       // status == BSGPU_ALIGN_OK
  int32_t status = -1;                            // BSGPU_ALIGN_*; -1: no back-end, or the call failed
  bs_math::Vec3 gravity{0, 0, 0}, bg{0, 0, 0}, ba{0, 0, 0};
  double scale = 1.0, excitation = 0.0;
  int32_t gyro_rank = 0;
  std::map<uint64_t, bs_math::Vec3> velocities;   // aligned (world) velocities, as AlignPathAndVelocities leaves velocities_
  InitPath path;                                  // the aligned path; the input when not initialised
};

class InertialAligner {
 public:
  explicit InertialAligner(int device = 0, const InertialAlignerParams& params = {}) : device_(device), params_(params) {}

  // Eigen::Quaterniond(R) of the rotation block, (w, x, y, z)
  static bs_math::Quat QuaternionOf(const bs_math::Mat<4, 4>& T) {
    const double tr = T(0, 0) + T(1, 1) + T(2, 2);
    bs_math::Quat q;
    if (tr > 0.0) {
      double s = std::sqrt(tr + 1.0);
      q[0] = 0.5 * s;
      s = 0.5 / s;
      q[1] = (T(2, 1) - T(1, 2)) * s; q[2] = (T(0, 2) - T(2, 0)) * s; q[3] = (T(1, 0) - T(0, 1)) * s;
    } else {
      int i = 0;
      if (T(1, 1) > T(0, 0)) i = 1;
      if (T(2, 2) > T(i, i)) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      double s = std::sqrt(T(i, i) - T(j, j) - T(k, k) + 1.0);
      q[1 + i] = 0.5 * s;
      s = 0.5 / s;
      q[0] = (T(k, j) - T(j, k)) * s;
      q[1 + j] = (T(j, i) + T(i, j)) * s;
      q[1 + k] = (T(k, i) + T(i, k)) * s;
    }
    return q;
  }
  static double Seconds(uint64_t nsec) { return (double)(nsec / 1000000000ull) + 1e-9 * (double)(nsec % 1000000000ull); }

  InertialAlignment Align(const InitPath& path, const std::vector<ImuSample>& imu) const { return AlignBatch({&path}, imu)[0]; }

  // every candidate path at once: one device call
  std::vector<InertialAlignment> AlignBatch(const std::vector<const InitPath*>& paths, const std::vector<ImuSample>& imu) const {
    const int32_t P = (int32_t)paths.size(), S = (int32_t)imu.size();
    std::vector<InertialAlignment> out(P);
    std::vector<int32_t> start(1, 0), range;
    std::vector<double> tf, qf, pf, t(S + 1), w(3 * (size_t)S + 1), a(3 * (size_t)S + 1);
    for (int32_t k = 0; k < P; ++k) {
      out[k].path = *paths[k];
      for (const auto& [nsec, T] : *paths[k]) {
        tf.push_back(Seconds(nsec));
        const bs_math::Quat q = QuaternionOf(T);
        qf.insert(qf.end(), q.begin(), q.end());
        for (int i = 0; i < 3; ++i) pf.push_back(T(i, 3));
      }
      start.push_back((int32_t)tf.size());
      range.push_back(0); range.push_back(S);
    }
    for (int32_t s = 0; s < S; ++s) {
      t[s] = imu[s].t;
      for (int i = 0; i < 3; ++i) { w[3 * (size_t)s + i] = imu[s].w[i]; a[3 * (size_t)s + i] = imu[s].a[i]; }
    }
    const size_t F = tf.size();
    tf.push_back(0.0); qf.push_back(0.0); pf.push_back(0.0);   // (never read: non-null data() for a call without frames)
    std::vector<double> grav(3 * (size_t)P + 1), bg(3 * (size_t)P + 1), scale(P + 1), exc(P + 1), vel(3 * F + 1), qo(4 * F + 1), po(3 * F + 1),
        vo(3 * F + 1);
    std::vector<int32_t> rank(P + 1), status(P + 1, -1);
    int rc = BSGPU_ERR_UNSUPPORTED;
    if (bsgpu_inertial_alignment && P > 0)
      rc = bsgpu_inertial_alignment(device_, P, start.data(), tf.data(), qf.data(), pf.data(), range.data(), t.data(), w.data(), a.data(),
                                    params_.bridge_gap ? 1 : 0, params_.min_excitation, params_.apply_scale ? 1 : 0, params_.scale_min,
                                    params_.scale_max, params_.rank_tol, grav.data(), bg.data(), scale.data(), exc.data(), rank.data(),
                                    vel.data(), qo.data(), po.data(), vo.data(), status.data());
    if (rc != BSGPU_OK) return out;
    for (int32_t k = 0; k < P; ++k) {
      InertialAlignment& r = out[k];
      r.status = status[k];
      r.initialized = r.status == BSGPU_ALIGN_OK;
      for (int i = 0; i < 3; ++i) { r.gravity[i] = grav[3 * (size_t)k + i]; r.bg[i] = bg[3 * (size_t)k + i]; }
      r.scale = scale[k]; r.excitation = exc[k]; r.gyro_rank = rank[k];
      size_t f = (size_t)start[k];
      for (auto& [nsec, T] : r.path) {
        r.velocities[nsec] = {vo[3 * f], vo[3 * f + 1], vo[3 * f + 2]};
        if (r.initialized) {
          const bs_math::Mat3 R = bs_math::quatToRot({qo[4 * f], qo[4 * f + 1], qo[4 * f + 2], qo[4 * f + 3]});
          for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) T(i, j) = R(i, j);
            T(i, 3) = po[3 * f + i];
          }
        }
        ++f;
      }
    }
    return out;
  }

 private:
  int device_;
  InertialAlignerParams params_;
};

}  // namespace bs_models
