// Frame localisation (bsgpu_localize_frames): the robust refinement of ONE baselink pose against constant world points, i.e. the
// one-pose BSGPU_F_REPROJ problem, as VisualOdometry::LocalizeFrame (bs_models/src/visual_odometry.cpp:217-300) hands it to [EXT]
// beam_cv::PoseRefinement::RefinePose (:240-248), and the screening average of ComputeAverageReprojection (:1247-1272).
//
// Host- and device-compilable, in the style of lm_decide.h: localize_kernel (k_loc.hip) runs flm_solve with one workgroup per frame
// and a block-wide reduction as its evaluator; tests/plan/test_frame_lm.cpp runs the same flm_solve on the CPU with a serial one and
// compares it with the oracle.  Everything a frame needs besides the sums of its observations (the trust-region loop, the 6x6
// Cholesky, the covariance) is scalar code every lane runs redundantly on the broadcast sums, so no lane ever waits on another
// except inside the evaluator's reduction.
//
// The loop restates LmState (lm_state.h: [EXT] ceres TrustRegionMinimizer + LevenbergMarquardtStrategy, Jacobi scaling) for a
// problem whose whole normal system is 6x6: each evaluation with Jacobians yields the cost, the 21 distinct entries of the
// loss-corrected J^T J and J^T r; the step is the Cholesky solution of the Jacobi-scaled system damped by the clamped diagonal over
// the radius; the model cost change is -(g.s + s^T H s / 2) in scaled coordinates.  Tangent order [p (3), theta (3)]: position first,
// orientation on BSGPU_MANIFOLD_QUAT_RIGHT (q (x) AngleAxisToQuaternion(theta)).  Tolerance norms are ambient, over (q, p), as in
// the oracle and the device solve (SC_STEP_NORM2, SC_X_NORM2, SC_GRAD_MAX).  max_solver_time_in_seconds is not looked at.
#pragma once
#include <cmath>

#include "../../include/bsgpu.h"
#include "bsgpu_internal.h"
#include "lm_decide.h"

#if defined(__HIPCC__)
#define BSG_FLM_FN __host__ __device__ __forceinline__
#else
#define BSG_FLM_FN inline
#endif

namespace bsg {

// the sums one evaluation produces: [0] cost (1/2 sum rho), [1..21] J^T J upper triangle row by row, [22..27] J^T r
constexpr int kFlmSums = 28;
struct FlmSums { double v[kFlmSums]; };

// frame results: the status values of include/bsgpu.h bsgpu_localize_frames
enum { FLM_REFINED = 0, FLM_TOO_FEW = 1, FLM_UNUSABLE = 2, FLM_SINGULAR = 3 };
struct FlmResult { double q[4], p[3], cost; int iterations, status; double cov[36]; };

// the reprojection factor's per-pose math (reproj_body.h, bsgpu_device.h), restated for host and device
BSG_FLM_FN void flm_quat_to_rot(const double q[4], double R[9]) {
  const double tx = 2.0 * q[1], ty = 2.0 * q[2], tz = 2.0 * q[3];
  const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
  const double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
  const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}
// x (x) AngleAxisToQuaternion(d): fuse's Orientation3DLocalParameterization::Plus (bs_constraints/src/jacobians.cpp:24-35)
BSG_FLM_FN void flm_quat_plus(const double x[4], const double d[3], double out[4]) {
  const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  double b[4];
  if (th2 > 0.0) {
    const double th = sqrt(th2), half = th * 0.5;
    const double k = sin(half) / th;
    b[0] = cos(half); b[1] = d[0] * k; b[2] = d[1] * k; b[3] = d[2] * k;
  } else {
    b[0] = 1.0; b[1] = d[0] * 0.5; b[2] = d[1] * 0.5; b[3] = d[2] * 0.5;
  }
  out[0] = x[0] * b[0] - x[1] * b[1] - x[2] * b[2] - x[3] * b[3];
  out[1] = x[0] * b[1] + x[1] * b[0] + x[2] * b[3] - x[3] * b[2];
  out[2] = x[0] * b[2] - x[1] * b[3] + x[2] * b[0] + x[3] * b[1];
  out[3] = x[0] * b[3] + x[1] * b[2] - x[2] * b[1] + x[3] * b[0];
}
// the Plus of flm_solve and flm_grad_norms unless a caller passes another (loam.h does: one without library sines)
struct FlmQuatPlus {
  BSG_FLM_FN void operator()(const double x[4], const double d[3], double out[4]) const { flm_quat_plus(x, d, out); }
};
// ceres::LossFunction::Evaluate: rho(s), *rho1 = rho'(s) (bsgpu_device.h loss_eval)
BSG_FLM_FN double flm_loss(int kind, double a, double s, double* rho1) {
  if (kind == BSGPU_LOSS_CAUCHY) {
    const double b = a * a, c = 1.0 / b;
    const double sum = 1.0 + s * c, inv = 1.0 / sum;
    *rho1 = fmax(2.2250738585072014e-308, inv);
    return b * log(sum);
  } else if (kind == BSGPU_LOSS_HUBER) {
    const double b = a * a;
    if (s > b) {
      const double r = sqrt(s);
      *rho1 = fmax(2.2250738585072014e-308, a / r);
      return 2.0 * a * r - b;
    }
  }
  *rho1 = 1.0;
  return s;
}

// P_c = R_cb (R^T P - R^T t) + t_cb (euclidean_reprojection_function.h; reproj_body.h)
BSG_FLM_FN void flm_camera_point(const DevCamera& cam, const double R[9], const double t[3], const double P[3], double Pb[3], double Pc[3]) {
  double a[3], b[3];
  for (int i = 0; i < 3; ++i) {
    a[i] = R[i] * P[0] + R[3 + i] * P[1] + R[6 + i] * P[2];
    b[i] = R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2];
  }
  for (int i = 0; i < 3; ++i) Pb[i] = a[i] - b[i];
  for (int i = 0; i < 3; ++i) Pc[i] = cam.R[3 * i] * Pb[0] + cam.R[3 * i + 1] * Pb[1] + cam.R[3 * i + 2] * Pb[2] + cam.t[i];
}

// one observation's share of an evaluation: cost, and with Jacobians J^T J and J^T r of its loss-corrected 2x6 tangent Jacobian
// (the pose half of reproj_body.h: d/dp = +M R^T, d/dtheta = -M [P_b]x, M = w sqrt(rho') Jpi R_cb)
BSG_FLM_FN void flm_obs_accum(const DevCamera& cam, const double R[9], const double t[3], const double P[3], double zx, double zy,
                              double w, int loss_kind, double loss_a, bool with_J, FlmSums& s) {
  double Pb[3], Pc[3];
  flm_camera_point(cam, R, t, P, Pb, Pc);
  const double iz = 1.0 / Pc[2];
  const double u = (cam.fx * Pc[0] + cam.cx * Pc[2]) * iz;
  const double v = (cam.fy * Pc[1] + cam.cy * Pc[2]) * iz;
  const double r0 = w * (zx - u), r1 = w * (zy - v);
  double rho1;
  const double rho = flm_loss(loss_kind, loss_a, r0 * r0 + r1 * r1, &rho1);
  s.v[0] += 0.5 * rho;
  if (!with_J) return;
  const double sc = sqrt(rho1);
  const double rc[2] = {r0 * sc, r1 * sc};
  const double jx0 = cam.fx * iz, jx2 = -cam.fx * Pc[0] * iz * iz;
  const double jy1 = cam.fy * iz, jy2 = -cam.fy * Pc[1] * iz * iz;
  const double ws = w * sc;
  double M[6];
  for (int j = 0; j < 3; ++j) {
    M[j] = ws * (jx0 * cam.R[j] + jx2 * cam.R[6 + j]);
    M[3 + j] = ws * (jy1 * cam.R[3 + j] + jy2 * cam.R[6 + j]);
  }
  double J[12];
  for (int i = 0; i < 2; ++i) {
    const double m0 = M[3 * i], m1 = M[3 * i + 1], m2 = M[3 * i + 2];
    for (int j = 0; j < 3; ++j) J[6 * i + j] = m0 * R[3 * j] + m1 * R[3 * j + 1] + m2 * R[3 * j + 2];
    J[6 * i + 3] = -(m1 * Pb[2] - m2 * Pb[1]);
    J[6 * i + 4] = -(m2 * Pb[0] - m0 * Pb[2]);
    J[6 * i + 5] = -(m0 * Pb[1] - m1 * Pb[0]);
  }
  int k = 1;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) s.v[k++] += J[i] * J[j] + J[6 + i] * J[6 + j];
  for (int i = 0; i < 6; ++i) s.v[22 + i] += J[i] * rc[0] + J[6 + i] * rc[1];
}

// ComputeAverageReprojection's term of one pair (visual_odometry.cpp:1247-1272): |z - pi(P_c)| when the point projects into the
// image (P_c.z > 0 and 0 <= u < width, 0 <= v < height; width or height <= 0: no bounds check), else nothing
BSG_FLM_FN double flm_pixel_error(const DevCamera& cam, const double R[9], const double t[3], const double P[3], double zx, double zy,
                                  int width, int height) {
  double Pb[3], Pc[3];
  flm_camera_point(cam, R, t, P, Pb, Pc);
  if (!(Pc[2] > 0.0)) return 0.0;
  const double iz = 1.0 / Pc[2];
  const double u = (cam.fx * Pc[0] + cam.cx * Pc[2]) * iz;
  const double v = (cam.fy * Pc[1] + cam.cy * Pc[2]) * iz;
  if (width > 0 && height > 0 && !(u >= 0.0 && u < (double)width && v >= 0.0 && v < (double)height)) return 0.0;
  const double du = zx - u, dv = zy - v;
  return sqrt(du * du + dv * dv);
}

// the packed upper triangle of FlmSums -> full 6x6 row-major
BSG_FLM_FN void flm_unpack(const FlmSums& s, double H[36], double g[6]) {
  int k = 1;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { H[6 * i + j] = s.v[k]; H[6 * j + i] = s.v[k]; ++k; }
  for (int i = 0; i < 6; ++i) g[i] = s.v[22 + i];
}
// lower Cholesky factor of a 6x6 in place; false on a pivot that is not positive or not finite (SC_CHOL_FAIL)
BSG_FLM_FN bool flm_chol6(double A[36]) {
  for (int j = 0; j < 6; ++j) {
    double d = A[6 * j + j];
    for (int p = 0; p < j; ++p) d -= A[6 * j + p] * A[6 * j + p];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    d = sqrt(d);
    A[6 * j + j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[6 * i + j];
      for (int p = 0; p < j; ++p) s -= A[6 * i + p] * A[6 * j + p];
      A[6 * i + j] = s / d;
    }
  }
  return true;
}
BSG_FLM_FN void flm_chol6_solve(const double L[36], double b[6]) {
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
    for (int p = 0; p < i; ++p) s -= L[6 * i + p] * b[p];
    b[i] = s / L[6 * i + i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = b[i];
    for (int p = i + 1; p < 6; ++p) s -= L[6 * p + i] * b[p];
    b[i] = s / L[6 * i + i];
  }
}
// |x - Plus(x, -g)| over the ambient (q, p): max and sum of squares (SC_GRAD_MAX, SC_GRAD_NORM2)
template <class Plus = FlmQuatPlus>
BSG_FLM_FN void flm_grad_norms(const double q[4], const double p[3], const double g[6], double* gmax, double* gn2, Plus plus = Plus()) {
  const double ng[3] = {-g[3], -g[4], -g[5]};
  double qm[4];
  plus(q, ng, qm);
  double mx = 0.0, s2 = 0.0;
  for (int i = 0; i < 4; ++i) { const double d = q[i] - qm[i]; s2 += d * d; mx = fmax(mx, fabs(d)); }
  for (int i = 0; i < 3; ++i) { const double d = g[i]; s2 += d * d; mx = fmax(mx, fabs(d)); }
  *gmax = mx; *gn2 = s2;
}

// The trust-region loop of one frame.  ev(q, p, with_J, sums) evaluates every observation of the frame at (q, p) and must hand
// every caller the same sums.  On return res holds the pose reached, its cost, the iteration count (LmState: the iterations
// recorded, i.e. not the one a tolerance or the invalid-step limit ends), the status and, for FLM_REFINED, the covariance
// (J^T J)^-1 of [p, theta] at that pose (NaN otherwise).  trace (optional, max_num_iterations entries): the fate of each recorded
// iteration, FLM_STEP_*.  plus: the orientation's Plus, flm_quat_plus unless the caller needs another.
enum { FLM_STEP_INVALID = 0, FLM_STEP_REJECTED = 1, FLM_STEP_ACCEPTED = 2 };
template <class Eval, class Plus = FlmQuatPlus>
BSG_FLM_FN void flm_solve(const bsgpu_options& o, const double q0[4], const double p0[3], Eval& ev, FlmResult& res, int* trace = nullptr,
                          Plus plus = Plus()) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double q[4] = {q0[0], q0[1], q0[2], q0[3]}, p[3] = {p0[0], p0[1], p0[2]};
  FlmSums s;
  ev(q, p, true, s);
  double x_cost = s.v[0];
  double H[36], g[6], scale[6], diag[6];
  flm_unpack(s, H, g);
  int iteration = 0, recorded = 0, status = FLM_REFINED;
  bool failed = !std::isfinite(x_cost);
  for (int i = 0; i < 6; ++i) scale[i] = o.jacobi_scaling ? 1.0 / (1.0 + sqrt(H[7 * i])) : 1.0;
  double gmax, gn2;
  flm_grad_norms(q, p, g, &gmax, &gn2, plus);
  double x_norm = 0.0;
  for (int i = 0; i < 4; ++i) x_norm += q[i] * q[i];
  for (int i = 0; i < 3; ++i) x_norm += p[i] * p[i];
  x_norm = sqrt(x_norm);
  double radius = o.initial_trust_region_radius, decrease_factor = 2.0;
  bool successful = true, reuse_diag = false;
  int n_invalid = 0;
  while (!failed) {
    recorded = iteration;
    if (iteration >= o.max_num_iterations) break;
    if (successful && gmax <= o.gradient_tolerance) break;
    if (radius <= o.min_trust_region_radius) break;
    ++iteration;
    if (!reuse_diag)
      for (int i = 0; i < 6; ++i) diag[i] = fmin(fmax(scale[i] * scale[i] * H[7 * i], o.min_lm_diagonal), o.max_lm_diagonal);
    reuse_diag = true;
    // (S H S + D / radius) y = S g, step = -y (scaled coordinates)
    double A[36], y[6];
    for (int i = 0; i < 6; ++i) {
      for (int j = 0; j < 6; ++j) A[6 * i + j] = scale[i] * H[6 * i + j] * scale[j];
      A[7 * i] += diag[i] / radius;
      y[i] = scale[i] * g[i];
    }
    double mcc = 0.0;
    bool valid = flm_chol6(A);
    if (valid) {
      flm_chol6_solve(A, y);
      for (int i = 0; i < 6; ++i) y[i] = -y[i];
      double gs = 0.0, sHs = 0.0;
      for (int i = 0; i < 6; ++i) {
        gs += scale[i] * g[i] * y[i];
        double hy = 0.0;
        for (int j = 0; j < 6; ++j) hy += scale[i] * H[6 * i + j] * scale[j] * y[j];
        sHs += y[i] * hy;
      }
      mcc = -(gs + sHs / 2.0);
      valid = std::isfinite(mcc) && mcc > 0.0;
    }
    if (!valid) {
      if (++n_invalid >= o.max_num_consecutive_invalid_steps) { failed = true; break; }
      radius *= 0.5;
      successful = false;
      if (trace) trace[iteration - 1] = FLM_STEP_INVALID;
      continue;
    }
    n_invalid = 0;
    double qc[4], pc[3];
    const double dth[3] = {y[3] * scale[3], y[4] * scale[4], y[5] * scale[5]};
    plus(q, dth, qc);
    for (int i = 0; i < 3; ++i) pc[i] = p[i] + y[i] * scale[i];
    ev(qc, pc, false, s);
    double cand_cost = s.v[0];
    if (!std::isfinite(cand_cost)) cand_cost = 1.7976931348623157e308;
    double sn2 = 0.0;
    for (int i = 0; i < 4; ++i) { const double d = q[i] - qc[i]; sn2 += d * d; }
    for (int i = 0; i < 3; ++i) { const double d = p[i] - pc[i]; sn2 += d * d; }
    if (sqrt(sn2) <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) break;
    const double cost_change = x_cost - cand_cost;
    if (fabs(cost_change) <= o.function_tolerance * x_cost) break;
    const double rd = cost_change / mcc;
    if (rd > o.min_relative_decrease) {
      for (int i = 0; i < 4; ++i) q[i] = qc[i];
      for (int i = 0; i < 3; ++i) p[i] = pc[i];
      ev(q, p, true, s);
      x_cost = s.v[0];
      flm_unpack(s, H, g);
      flm_grad_norms(q, p, g, &gmax, &gn2, plus);
      x_norm = 0.0;
      for (int i = 0; i < 4; ++i) x_norm += q[i] * q[i];
      for (int i = 0; i < 3; ++i) x_norm += p[i] * p[i];
      x_norm = sqrt(x_norm);
      radius = fmin(o.max_trust_region_radius, radius / fmax(1.0 / 3.0, 1.0 - lm_cube(2.0 * rd - 1.0)));
      decrease_factor = 2.0;
      reuse_diag = false;
      successful = true;
      if (trace) trace[iteration - 1] = FLM_STEP_ACCEPTED;
    } else {
      radius = radius / decrease_factor;
      decrease_factor *= 2.0;
      successful = false;
      if (trace) trace[iteration - 1] = FLM_STEP_REJECTED;
    }
  }
  for (int i = 0; i < 4; ++i) { res.q[i] = q[i]; failed = failed || !std::isfinite(q[i]); }
  for (int i = 0; i < 3; ++i) { res.p[i] = p[i]; failed = failed || !std::isfinite(p[i]); }
  res.cost = x_cost;
  res.iterations = recorded;
  for (int i = 0; i < 36; ++i) res.cov[i] = NAN;
  if (failed) status = FLM_UNUSABLE;
  else if (!flm_chol6(H)) status = FLM_SINGULAR;
  else {
    for (int j = 0; j < 6; ++j) {
      double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      e[j] = 1.0;
      flm_chol6_solve(H, e);
      for (int i = 0; i < 6; ++i) res.cov[6 * i + j] = e[i];
    }
  }
  res.status = status;
}

// VisualOdometry::LocalizeFrame's gate (visual_odometry.cpp:217-248): below min_points observations nothing is solved, the pose is
// returned as given with its cost there (FLM_TOO_FEW)
template <class Eval>
BSG_FLM_FN void flm_localize(const bsgpu_options& o, int n_obs, int min_points, const double q0[4], const double p0[3], Eval& ev, FlmResult& res,
                                  int* trace = nullptr) {
  if (n_obs >= min_points) { flm_solve(o, q0, p0, ev, res, trace); return; }
  FlmSums s;
  ev(q0, p0, false, s);
  for (int i = 0; i < 4; ++i) res.q[i] = q0[i];
  for (int i = 0; i < 3; ++i) res.p[i] = p0[i];
  res.cost = s.v[0];
  res.iterations = 0;
  for (int i = 0; i < 36; ++i) res.cov[i] = NAN;
  res.status = FLM_TOO_FEW;
}

}  // namespace bsg
