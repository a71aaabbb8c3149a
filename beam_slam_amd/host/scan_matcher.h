// bs_models::scan_registration::ScanMatcher — a stand-in for MultiScanRegistration::MatchScans
// (bs_models/src/lib/scan_registration/multi_scan_registration.cpp:451-487) around one bsgpu_register_scans call: a new scan against
// its neighbours (num_neighbors = 3, config/registration/multi_scan.json:7), or loop-closure candidates, as ONE batch.
//   * PassedMotionThresholds (scan_registration_base.cpp:175-207) with its three returns: translation alone when min_motion_rot_deg
//     == 0, rotation alone when min_motion_trans_m == 0, either otherwise; a translation above max_motion_trans_m fails first.  The
//     angle is Eigen::AngleAxis's, in [0, pi];
//   * the pairs that pass go to the device in one call: T_LidarRefEst_LidarTgt = inv(T_REFFRAME_LIDAR ref) T_REFFRAME_LIDAR tgt as T_init,
//     the reference cloud as the matcher's ref, the target cloud as its target (:454-467); the match is never computed on the host;
//   * T_LIDARREF_LIDARTGT = inv(T_RefEst_Ref) T_LidarRefEst_LidarTgt (:474-476) comes back from the same call;
//   * RegistrationValidation::Validate (registration_validation.cpp:11-115) with a fixed covariance, per matcher in the order of the
//     batch.  Its windowed branch reads r_diffsqrd, t_diffsqrd and entropy_diffsqrd uninitialised (:47-53); here they start at 0
//     (INTEGRATION.md);
// A pair's `matched` is the reference's `return`: motion thresholds passed, the matcher converged, the validation passed.  Without the
// entry point in the back-end, or when the call fails, nothing is matched.
#pragma once
#include <cmath>
#include <cstdint>
#include <deque>
#include <vector>

#include "../../include/bsgpu.h"
#include "bs_common.h"

// optional in a back-end: without it no pair is matched
extern "C" int bsgpu_register_scans(int device, int32_t n_pairs, const int32_t* ref_start, const double* ref_points, const int32_t* tgt_start,
                                    const double* tgt_points, const double* T_init, double max_corr, int32_t max_iter, double t_eps,
                                    double fit_eps, double rotation_threshold, double rel_mse_eps, double* T_refest_ref, double* T_ref_tgt,
                                    double* mse, int32_t* n_corr, int32_t* n_iters, int32_t* status) __attribute__((weak));

namespace bs_models { namespace scan_registration {

using Mat4 = bs_math::Mat<4, 4>;
using Cov6 = bs_math::Mat<6, 6>;

struct ScanPose {                        // what MatchScans reads of a bs_common::ScanPose
  Mat4 T_REFFRAME_LIDAR = Mat4::Identity();
  std::vector<double> cloud;             // packed xyz, lidar frame
};

struct IcpMatcherParams {                // config/matchers/icp.json; the last two: PCL's defaults (recalled)
  double max_corr = 1.0;
  int max_iter = 50;
  double t_eps = 1e-8, fit_eps = 1e-2;
  double rotation_threshold = 0.99999, rel_mse_eps = 1e-5;
};

struct ScanRegistrationParamsBase {      // scan_registration_base.h:27-34
  double min_motion_trans_m = 0.0, min_motion_rot_deg = 0.0, max_motion_trans_m = 10.0;
};

inline Mat4 InvertTransform(const Mat4& T) {
  Mat4 o = Mat4::Identity();
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o(i, j) = T(j, i);
    o(i, 3) = -(T(0, i) * T(0, 3) + T(1, i) * T(1, 3) + T(2, i) * T(2, 3));
  }
  return o;
}
// Eigen::AngleAxis<double>(R).angle(), in [0, pi]: |(R32 - R23, R13 - R31, R21 - R12)| = 2 sin, trace = 1 + 2 cos
inline double RotationAngle(const Mat4& T) {
  const double x = T(2, 1) - T(1, 2), y = T(0, 2) - T(2, 0), z = T(1, 0) - T(0, 1);
  return std::atan2(0.5 * std::sqrt(x * x + y * y + z * z), 0.5 * (T(0, 0) + T(1, 1) + T(2, 2) - 1.0));
}
inline double TranslationNorm(const Mat4& T) { return std::sqrt(T(0, 3) * T(0, 3) + T(1, 3) * T(1, 3) + T(2, 3) * T(2, 3)); }

// bs_common::ShannonEntropyFromPoseCovariance (bs_common/src/bs_common/utils.cpp:81-86): 1/2 log((2 pi e)^6 det(cov))
inline double ShannonEntropyFromPoseCovariance(const Cov6& cov) {
  double a[36], det = 1.0;
  for (int i = 0; i < 36; ++i) a[i] = cov.a[i];
  for (int c = 0; c < 6; ++c) {                          // Gaussian elimination with partial pivoting
    int piv = c;
    for (int r = c + 1; r < 6; ++r) if (std::fabs(a[6 * r + c]) > std::fabs(a[6 * piv + c])) piv = r;
    if (a[6 * piv + c] == 0.0) { det = 0.0; break; }
    if (piv != c) { for (int k = 0; k < 6; ++k) { const double t = a[6 * c + k]; a[6 * c + k] = a[6 * piv + k]; a[6 * piv + k] = t; } det = -det; }
    det *= a[6 * c + c];
    for (int r = c + 1; r < 6; ++r) {
      const double f = a[6 * r + c] / a[6 * c + c];
      for (int k = c; k < 6; ++k) a[6 * r + k] -= f * a[6 * c + k];
    }
  }
  return 0.5 * std::log(std::pow(2.0 * M_PI * std::exp(1.0), 6.0) * det);
}

struct RegistrationMetrics { double r, t, entropy; };

class RegistrationValidation {           // registration_validation.h:53-59 defaults
 public:
  int list_size = 15;
  double t_init_thresh = 0.5, r_init_thresh = 3.14 / 6, entropy_init_thresh = -4.0;

  bool Validate(const Mat4& T_measured, const Cov6& covariance) {
    const RegistrationMetrics m{RotationAngle(T_measured), TranslationNorm(T_measured), ShannonEntropyFromPoseCovariance(covariance)};
    return Validate(m);
  }
  bool Validate(const RegistrationMetrics& m) {
    metrics_.push_back(m);
    if ((int)metrics_.size() > list_size) {
      metrics_.pop_front();
      return CheckStoredMetrics();
    }
    return CheckMetricInitial(m);
  }
  const std::deque<RegistrationMetrics>& metrics() const { return metrics_; }

 private:
  bool CheckStoredMetrics() const {
    double r_sum = 0, t_sum = 0, e_sum = 0;
    for (const auto& m : metrics_) { r_sum += m.r; t_sum += m.t; e_sum += m.entropy; }
    const double r_mean = r_sum / list_size, t_mean = t_sum / list_size, e_mean = e_sum / list_size;
    double r_d = 0, t_d = 0, e_d = 0;      // the reference reads these uninitialised (:47-49)
    for (const auto& m : metrics_) {
      r_d += (m.r - r_mean) * (m.r - r_mean); t_d += (m.t - t_mean) * (m.t - t_mean); e_d += (m.entropy - e_mean) * (m.entropy - e_mean);
    }
    const double r_sd = std::sqrt(r_d / list_size), t_sd = std::sqrt(t_d / list_size), e_sd = std::sqrt(e_d / list_size);
    const RegistrationMetrics& m = metrics_.back();
    if (m.r > r_mean + 2 * r_sd || m.r < r_mean - 2 * r_sd) return false;
    if (m.t > t_mean + 2 * t_sd || m.t < t_mean - 2 * t_sd) return false;
    if (m.entropy > e_mean + 5 * e_sd || m.entropy < e_mean - 5 * e_sd) return false;
    return true;
  }
  bool CheckMetricInitial(const RegistrationMetrics& m) const {
    return !(m.t > t_init_thresh) && !(m.r > r_init_thresh) && !(m.entropy > entropy_init_thresh);
  }
  std::deque<RegistrationMetrics> metrics_;
};

struct ScanMatch {
  bool matched = false;                  // MatchScans' return value
  bool passed_motion = false;            // PassedMotionThresholds
  bool converged = false;                // matcher_->Match()
  bool validated = false;                // RegistrationValidation::Validate
  int32_t status = -1;                   // BSGPU_ICP_*; -1: not sent to the device, no back-end, or the call failed
  int32_t n_iters = 0, n_corr = 0;
  double mse = 0.0;
  Mat4 T_RefEst_Ref = Mat4::Identity();
  Mat4 T_LIDARREF_LIDARTGT = Mat4::Identity();
};

class ScanMatcher {
 public:
  explicit ScanMatcher(int device = 0, const IcpMatcherParams& matcher = {}, const ScanRegistrationParamsBase& base = {},
                       const Cov6& fixed_covariance = DefaultCovariance())
      : device_(device), matcher_(matcher), base_(base), covariance_(fixed_covariance) {}

  static Cov6 DefaultCovariance() {        // a diagonal whose entropy passes the initial threshold (-4): 1e-3 on every axis
    Cov6 c;
    for (int i = 0; i < 6; ++i) c(i, i) = 1e-3;
    return c;
  }

  bool PassedMotionThresholds(const Mat4& T_CLOUD1_CLOUD2) const {
    const double d_12 = TranslationNorm(T_CLOUD1_CLOUD2);
    if (base_.max_motion_trans_m > 0 && d_12 > base_.max_motion_trans_m) return false;
    const bool passed_trans = !(base_.min_motion_trans_m > 0 && d_12 < base_.min_motion_trans_m);
    const double angle_deg = RotationAngle(T_CLOUD1_CLOUD2) * 180.0 / M_PI;
    const bool passed_rot = !(base_.min_motion_rot_deg > 0 && angle_deg < base_.min_motion_rot_deg);
    if (base_.min_motion_rot_deg == 0) return passed_trans;
    if (base_.min_motion_trans_m == 0) return passed_rot;
    return passed_trans || passed_rot;
  }

  ScanMatch MatchScans(const ScanPose& ref, const ScanPose& tgt) { return MatchScansBatch({&ref}, tgt)[0]; }

  // the target scan against every reference scan: one device call for the pairs that pass the motion thresholds
  std::vector<ScanMatch> MatchScansBatch(const std::vector<const ScanPose*>& refs, const ScanPose& tgt) {
    std::vector<ScanMatch> out(refs.size());
    std::vector<int32_t> rs(1, 0), ts(1, 0);
    std::vector<double> rp, tp, init;
    std::vector<size_t> sent;
    for (size_t k = 0; k < refs.size(); ++k) {
      const Mat4 T_est = InvertTransform(refs[k]->T_REFFRAME_LIDAR) * tgt.T_REFFRAME_LIDAR;
      out[k].passed_motion = PassedMotionThresholds(T_est);
      if (!out[k].passed_motion) continue;
      sent.push_back(k);
      rp.insert(rp.end(), refs[k]->cloud.begin(), refs[k]->cloud.end());
      tp.insert(tp.end(), tgt.cloud.begin(), tgt.cloud.end());
      rs.push_back((int32_t)(rp.size() / 3)); ts.push_back((int32_t)(tp.size() / 3));
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) init.push_back(T_est(i, j));
    }
    const int32_t P = (int32_t)sent.size();
    if (P == 0 || !bsgpu_register_scans) return out;
    rp.push_back(0.0); tp.push_back(0.0);    // (never read: non-null data() for empty clouds)
    std::vector<double> T(12 * (size_t)P), Trt(12 * (size_t)P), mse(P);
    std::vector<int32_t> nc(P), ni(P), st(P, -1);
    const int rc = bsgpu_register_scans(device_, P, rs.data(), rp.data(), ts.data(), tp.data(), init.data(), matcher_.max_corr, matcher_.max_iter,
                                        matcher_.t_eps, matcher_.fit_eps, matcher_.rotation_threshold, matcher_.rel_mse_eps, T.data(), Trt.data(),
                                        mse.data(), nc.data(), ni.data(), st.data());
    if (rc != BSGPU_OK) return out;
    for (int32_t p = 0; p < P; ++p) {
      ScanMatch& m = out[sent[p]];
      m.status = st[p]; m.n_iters = ni[p]; m.n_corr = nc[p]; m.mse = mse[p];
      m.converged = m.status != BSGPU_ICP_TOO_FEW_CORRESPONDENCES;
      if (!m.converged) continue;            // "Failed scan matching within matcher class. Skipping measurement." (:468-472)
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) { m.T_RefEst_Ref(i, j) = T[12 * (size_t)p + 4 * i + j]; m.T_LIDARREF_LIDARTGT(i, j) = Trt[12 * (size_t)p + 4 * i + j]; }
      m.validated = validation_.Validate(m.T_RefEst_Ref, covariance_);
      m.matched = m.validated;
    }
    return out;
  }

  RegistrationValidation& validation() { return validation_; }

 private:
  int device_;
  IcpMatcherParams matcher_;
  ScanRegistrationParamsBase base_;
  Cov6 covariance_;
  RegistrationValidation validation_;
};

}}  // namespace bs_models::scan_registration
