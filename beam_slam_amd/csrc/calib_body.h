// The extrinsic part of the online-calibration reprojection factor (BSGPU_F_REPROJ_ONLINE_CALIB with a free extrinsic pair):
// bs_constraints::EuclideanReprojectionConstraintOnlineCalib
// (visual/euclidean_reprojection_functor_online_calib.h:38-77, AutoDiff<2,4,3,3,4,3>) differentiated in closed form with respect to
// its last two parameter blocks, q_BASELINK_CAM (right perturbation q <- q (x) Exp(theta)) and p_BASELINK_CAM.
//
//   P_b = R_wb^T (P - t_wb),  R_cb = R(q_bc)^T,  P_c = R_cb (P_b - p_bc) = R_cb P_b + t_cb,  r = w (z - pi(K P_c)),  ws = w sqrt(rho')
//   E_theta = -ws Jpi(P_c) [P_c]x        E_p = +ws Jpi(P_c) R_cb
//
// Host- and device-compilable, in the style of unicycle_body.h: k_calib.hip runs it a factor per lane, tests/plan/calib_body_capi.cpp
// exposes the same functions on the CPU for tests/test_calib_body.py.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define BSG_CALIB_FN __host__ __device__ __forceinline__
#else
#define BSG_CALIB_FN inline
#endif

namespace bsg {

// Eigen::Quaternion::toRotationMatrix() (no normalisation), row-major: what the functor applies (helpers.h:27-35)
BSG_CALIB_FN void calib_quat_to_rot(const double q[4], double R[9]) {
  const double tx = 2.0 * q[1], ty = 2.0 * q[2], tz = 2.0 * q[3];
  const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
  const double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
  const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

// T_CAM_BASELINK = InvertTransform(T_BASELINK_CAM): R_cb = R(q_bc)^T, t_cb = -R_cb p_bc — the derived camera entry of the pair, in the
// arithmetic finalize() folds a constant pair with
BSG_CALIB_FN void calib_camera(const double q_bc[4], const double p_bc[3], double R_cb[9], double t_cb[3]) {
  double Rbc[9];
  calib_quat_to_rot(q_bc, Rbc);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R_cb[3 * i + j] = Rbc[3 * j + i];
  for (int i = 0; i < 3; ++i) t_cb[i] = -(R_cb[3 * i] * p_bc[0] + R_cb[3 * i + 1] * p_bc[1] + R_cb[3 * i + 2] * p_bc[2]);
}

// rho'(s) of ceres::CauchyLoss (kind 1) / HuberLoss (kind 2) / no loss (kind 0): include/bsgpu.h BSGPU_LOSS_*, in loss_eval's arithmetic
BSG_CALIB_FN double calib_rho1(int kind, double a, double s) {
  if (kind == 1) { const double c = 1.0 / (a * a); return fmax(2.2250738585072014e-308, 1.0 / (1.0 + s * c)); }
  if (kind == 2 && s > a * a) return fmax(2.2250738585072014e-308, a / sqrt(s));
  return 1.0;
}

// E = [E row 0 (theta: 3, p: 3) | E row 1] of one factor, robustified as reproj_eval_body robustifies A and B (the corrector's
// sqrt(rho') scale); a block that is constant gets zero columns.  Same arithmetic for P_c as reproj_eval_body.
BSG_CALIB_FN void calib_E(const double q_wb[4], const double t_wb[3], const double P[3], const double R_cb[9], const double t_cb[3], double fx,
                          double fy, double cx, double cy, double u_m, double v_m, double w, int loss_kind, double loss_a, bool theta_free,
                          bool p_free, double E[12]) {
  double R[9];
  calib_quat_to_rot(q_wb, R);
  double a[3], b[3];
  for (int i = 0; i < 3; ++i) {
    a[i] = R[i] * P[0] + R[3 + i] * P[1] + R[6 + i] * P[2];
    b[i] = R[i] * t_wb[0] + R[3 + i] * t_wb[1] + R[6 + i] * t_wb[2];
  }
  const double Pb[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
  double Pc[3];
  for (int i = 0; i < 3; ++i) Pc[i] = R_cb[3 * i] * Pb[0] + R_cb[3 * i + 1] * Pb[1] + R_cb[3 * i + 2] * Pb[2] + t_cb[i];
  const double iz = 1.0 / Pc[2];
  const double u = (fx * Pc[0] + cx * Pc[2]) * iz, v = (fy * Pc[1] + cy * Pc[2]) * iz;
  const double r0 = w * (u_m - u), r1 = w * (v_m - v);
  const double ws = w * sqrt(calib_rho1(loss_kind, loss_a, r0 * r0 + r1 * r1));
  // ws Jpi (2x3): rows (jx0, 0, jx2), (0, jy1, jy2)
  const double jx0 = ws * fx * iz, jx2 = -ws * fx * Pc[0] * iz * iz;
  const double jy1 = ws * fy * iz, jy2 = -ws * fy * Pc[1] * iz * iz;
  const double Jp[6] = {jx0, 0.0, jx2, 0.0, jy1, jy2};
  for (int k = 0; k < 2; ++k) {
    const double m0 = Jp[3 * k], m1 = Jp[3 * k + 1], m2 = Jp[3 * k + 2];
    // -(m [P_c]x): (m [v]x)_j = (m x v) components with the sign of a row vector times a skew matrix
    E[6 * k + 0] = theta_free ? -(m1 * Pc[2] - m2 * Pc[1]) : 0.0;
    E[6 * k + 1] = theta_free ? -(m2 * Pc[0] - m0 * Pc[2]) : 0.0;
    E[6 * k + 2] = theta_free ? -(m0 * Pc[1] - m1 * Pc[0]) : 0.0;
    for (int j = 0; j < 3; ++j) E[6 * k + 3 + j] = p_free ? (m0 * R_cb[j] + m1 * R_cb[3 + j] + m2 * R_cb[6 + j]) : 0.0;
  }
}

}  // namespace bsg
