// One interval of bsgpu_preintegrate (k_preint.hip): bs_common::PreIntegrator restated
// (bs_common/src/bs_common/preintegrator.cpp) —
//   Increment  :26-89   covariance propagation A P A^T + B Q B^T on the 9-d error state (q, p, v), bias random walk,
//                        bias Jacobians (order of the updates matters), mid-point state integration
//   Integrate  :91-115  consecutive samples up to t_end, then the remainder with the last sample
//   ComputeSqrtInvCov :117-143  norm guards, sqrt information = cov^-1 .llt().matrixU(), fallback weight
// writing the constant payload of BSGPU_F_IMU_DELTA (include/bsgpu.h): dt, dq, dp, dv, the five bias Jacobians, the bias
// linearisation point and A = info_weight * sqrt_inv_cov.
//
// Host- and device-compilable, in the style of p3p.h: plain C++, nothing from HIP but the qualifiers.  preintegrate_kernel gives an
// interval to a lane; tests/plan/test_preint.cpp runs the same function on the CPU.
//
// The coefficients of Rodrigues' formula and of the right Jacobian, with th = |w|,
//      A = sin th / th,   B = (1 - cos th) / th^2,   C = (th - sin th) / th^3,
// are evaluated without cancellation (pre_so3_coeffs): B through the half angle, C by its series below th = 0.5.  The closed forms
// of B and C lose th^-2 and 6 th^-2 ulps (100 % at th = 1e-8, 1e-9 entrywise in the right Jacobian at th = 1e-6), and a
// stationary or slowly turning IMU has |w - b_g| dt exactly there; switching to the limits only below 1e-8 / 1e-10, as the
// reference's helpers do, leaves that whole range wrong.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define BSG_PRE_FN __host__ __device__ __forceinline__
#else
#define BSG_PRE_FN inline
#endif

namespace bsg {

constexpr int kPreintOut = 287;   // doubles per interval: consts of BSGPU_F_IMU_DELTA

struct M3 { double m[9]; };
BSG_PRE_FN M3 m3_zero() { M3 r; for (int i = 0; i < 9; ++i) r.m[i] = 0.0; return r; }
BSG_PRE_FN M3 m3_eye() { M3 r = m3_zero(); r.m[0] = r.m[4] = r.m[8] = 1.0; return r; }
BSG_PRE_FN M3 m3_mul(const M3& a, const M3& b) {
  M3 r;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
  return r;
}
BSG_PRE_FN M3 m3_t(const M3& a) { M3 r; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r.m[3 * i + j] = a.m[3 * j + i]; return r; }
BSG_PRE_FN M3 m3_axpy(double s, const M3& a, const M3& b) { M3 r; for (int i = 0; i < 9; ++i) r.m[i] = s * a.m[i] + b.m[i]; return r; }
BSG_PRE_FN M3 m3_skew(const double v[3]) { M3 r = m3_zero(); r.m[1] = -v[2]; r.m[2] = v[1]; r.m[3] = v[2]; r.m[5] = -v[0]; r.m[6] = -v[1]; r.m[7] = v[0]; return r; }
// quat_to_rot / quat_mul of bsgpu_device.h (Eigen::Quaternion::toRotationMatrix, no normalisation), which the host cannot include
BSG_PRE_FN M3 pre_quat_to_rot(const double q[4]) {
  const double tx = 2.0 * q[1], ty = 2.0 * q[2], tz = 2.0 * q[3];
  const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
  const double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
  const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
  M3 R;
  R.m[0] = 1.0 - (tyy + tzz); R.m[1] = txy - twz;         R.m[2] = txz + twy;
  R.m[3] = txy + twz;         R.m[4] = 1.0 - (txx + tzz); R.m[5] = tyz - twx;
  R.m[6] = txz - twy;         R.m[7] = tyz + twx;         R.m[8] = 1.0 - (txx + tyy);
  return R;
}
BSG_PRE_FN void pre_quat_mul(const double a[4], const double b[4], double o[4]) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3 to a few ulps for every th >= 0.
//   B = 2 sin^2(th/2) / th^2: no subtraction.
//   C: seven terms of sum (-1)^k th^2k / (2k+3)! below th = 0.5 (first dropped term 0.5^14 / 17! = 1.7e-19, against 1/6); above, the
//   closed form loses 6 / th^2 <= 24 ulps of C, which enters the Jacobian through th^2 C <= 0.05: below one ulp of its unit diagonal.
BSG_PRE_FN void pre_so3_coeffs(double th, double& A, double& B, double& C) {
  if (!(th > 0.0)) { A = 1.0; B = 0.5; C = 1.0 / 6.0; return; }
  const double sn = sin(th), sh = sin(0.5 * th) / th;
  A = sn / th;
  B = 2.0 * sh * sh;
  if (th < 0.5) {
    const double u = th * th;
    C = 1.0 / 6.0 + u * (-1.0 / 120.0 + u * (1.0 / 5040.0 + u * (-1.0 / 362880.0 + u * (1.0 / 39916800.0 +
        u * (-1.0 / 6227020800.0 + u * (1.0 / 1307674368000.0))))));
  } else {
    C = (th - sn) / (th * th * th);
  }
}
// [EXT] beam::LieAlgebraToR (Rodrigues)
BSG_PRE_FN M3 so3_exp(const double w[3]) {
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const M3 K = m3_skew(w), K2 = m3_mul(K, K);
  double a, b, c;
  pre_so3_coeffs(th, a, b, c);
  M3 r = m3_eye();
  for (int i = 0; i < 9; ++i) r.m[i] += a * K.m[i] + b * K2.m[i];
  return r;
}
// [EXT] beam::RightJacobianOfSO3
BSG_PRE_FN M3 so3_jr(const double w[3]) {
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const M3 K = m3_skew(w), K2 = m3_mul(K, K);
  double a, b, c;
  pre_so3_coeffs(th, a, b, c);
  M3 r = m3_eye();
  for (int i = 0; i < 9; ++i) r.m[i] += -b * K.m[i] + c * K2.m[i];
  return r;
}
BSG_PRE_FN void quat_from_aa_unit(const double w[3], double q[4]) {
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  if (th < 1e-12) {
    q[0] = 1.0; q[1] = 0.5 * w[0]; q[2] = 0.5 * w[1]; q[3] = 0.5 * w[2];
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] /= n;
  } else {
    const double s = sin(0.5 * th) / th;
    q[0] = cos(0.5 * th); q[1] = s * w[0]; q[2] = s * w[1]; q[3] = s * w[2];
  }
}

// in-place lower Cholesky of an n x n SPD matrix (row-major, pitch n); false on a non-positive pivot
template <int N> BSG_PRE_FN bool chol_lower(double* A) {
  for (int j = 0; j < N; ++j) {
    double d = A[j * N + j];
    for (int k = 0; k < j; ++k) d -= A[j * N + k] * A[j * N + k];
    if (!(d > 0.0)) return false;
    const double l = sqrt(d);
    A[j * N + j] = l;
    for (int i = j + 1; i < N; ++i) {
      double s = A[i * N + j];
      for (int k = 0; k < j; ++k) s -= A[i * N + k] * A[j * N + k];
      A[i * N + j] = s / l;
    }
  }
  return true;
}

// Interval of the samples [s0, s1) of (ts, wm, am) up to the time te, at the bias linearisation point (bg, ba).
// covs: cov_w, cov_a, cov_bg, cov_ba, 4 x 9 row-major.  o: kPreintOut doubles.
BSG_PRE_FN void preintegrate_interval(int s0, int s1, const double* __restrict__ ts, const double* __restrict__ wm,
                                      const double* __restrict__ am, double te, const double* __restrict__ bg_in,
                                      const double* __restrict__ ba_in, const double* __restrict__ covs, double info_weight,
                                      double* __restrict__ o) {
  const double bg[3] = {bg_in[0], bg_in[1], bg_in[2]}, ba[3] = {ba_in[0], ba_in[1], ba_in[2]};
  double dt_tot = 0.0, q[4] = {1, 0, 0, 0}, p[3] = {0, 0, 0}, v[3] = {0, 0, 0};
  double cov[15 * 15];
  for (int i = 0; i < 225; ++i) cov[i] = 0.0;
  M3 dq_dbg = m3_zero(), dp_dbg = m3_zero(), dp_dba = m3_zero(), dv_dbg = m3_zero(), dv_dba = m3_zero();
  M3 Cw, Ca, Cbg, Cba;
  for (int i = 0; i < 9; ++i) { Cw.m[i] = covs[i]; Ca.m[i] = covs[9 + i]; Cbg.m[i] = covs[18 + i]; Cba.m[i] = covs[27 + i]; }

  auto increment = [&](double dt, const double* wraw, const double* araw) {   // preintegrator.cpp:26-89
    const double w[3] = {wraw[0] - bg[0], wraw[1] - bg[1], wraw[2] - bg[2]}, a[3] = {araw[0] - ba[0], araw[1] - ba[1], araw[2] - ba[2]};
    const double wdt[3] = {w[0] * dt, w[1] * dt, w[2] * dt}, whalf[3] = {0.5 * wdt[0], 0.5 * wdt[1], 0.5 * wdt[2]};
    const M3 R_full = so3_exp(wdt), Jr = so3_jr(wdt), Sa = m3_skew(a);
    const M3 Rdq = pre_quat_to_rot(q);
    const M3 RS = m3_mul(Rdq, Sa);
    // A (9x9) and B (9x6) of the error-state propagation; error-state order q(0) p(3) v(6)
    double A[81], B[54];
    for (int i = 0; i < 81; ++i) A[i] = 0.0;
    for (int i = 0; i < 54; ++i) B[i] = 0.0;
    for (int i = 0; i < 9; ++i) A[10 * i] = 1.0;
    const M3 Rt = m3_t(R_full);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
      A[(0 + i) * 9 + j] = Rt.m[3 * i + j];
      A[(6 + i) * 9 + j] = -dt * RS.m[3 * i + j];
      A[(3 + i) * 9 + j] = -0.5 * dt * dt * RS.m[3 * i + j];
      A[(3 + i) * 9 + 6 + j] = (i == j) ? dt : 0.0;
      B[(0 + i) * 6 + j] = dt * Jr.m[3 * i + j];
      B[(6 + i) * 6 + 3 + j] = dt * Rdq.m[3 * i + j];
      B[(3 + i) * 6 + 3 + j] = 0.5 * dt * dt * Rdq.m[3 * i + j];
    }
    const double inv_dt = 1.0 / fmax(dt, 1.0e-7);
    // P9 <- A P9 A^T + B Q B^T,  Q = blkdiag(cov_w, cov_a) / dt
    double AP[81], P9[81];
    for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) { double s = 0.0; for (int k = 0; k < 9; ++k) s += A[i * 9 + k] * cov[k * 15 + j]; AP[i * 9 + j] = s; }
    for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) { double s = 0.0; for (int k = 0; k < 9; ++k) s += AP[i * 9 + k] * A[j * 9 + k]; P9[i * 9 + j] = s; }
    double BQ[54];
    for (int i = 0; i < 9; ++i) for (int j = 0; j < 6; ++j) {
      double s = 0.0;
      const M3& Qb = j < 3 ? Cw : Ca;
      const int off = j < 3 ? 0 : 3;
      for (int k = 0; k < 3; ++k) s += B[i * 6 + off + k] * (Qb.m[3 * k + (j - off)] * inv_dt);
      BQ[i * 6 + j] = s;
    }
    for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) { double s = 0.0; for (int k = 0; k < 6; ++k) s += BQ[i * 6 + k] * B[j * 6 + k]; cov[i * 15 + j] = P9[i * 9 + j] + s; }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { cov[(9 + i) * 15 + 9 + j] += dt * Cbg.m[3 * i + j]; cov[(12 + i) * 15 + 12 + j] += dt * Cba.m[3 * i + j]; }
    // bias Jacobians (:69-80, this order)
    const M3 RSdq = m3_mul(RS, dq_dbg);
    dp_dbg = m3_axpy(-0.5 * dt * dt, RSdq, m3_axpy(dt, dv_dbg, dp_dbg));
    dp_dba = m3_axpy(-0.5 * dt * dt, Rdq, m3_axpy(dt, dv_dba, dp_dba));
    dv_dbg = m3_axpy(-dt, RSdq, dv_dbg);
    dv_dba = m3_axpy(-dt, Rdq, dv_dba);
    dq_dbg = m3_axpy(-dt, Jr, m3_mul(Rt, dq_dbg));
    // state (:82-88)
    double qh[4], qm[4], qf[4], qn[4];
    quat_from_aa_unit(whalf, qh);
    pre_quat_mul(q, qh, qm);
    const M3 Rm = pre_quat_to_rot(qm);
    const double amid[3] = {Rm.m[0] * a[0] + Rm.m[1] * a[1] + Rm.m[2] * a[2], Rm.m[3] * a[0] + Rm.m[4] * a[1] + Rm.m[5] * a[2],
                            Rm.m[6] * a[0] + Rm.m[7] * a[1] + Rm.m[8] * a[2]};
    dt_tot += dt;
    for (int i = 0; i < 3; ++i) p[i] += dt * v[i] + 0.5 * dt * dt * amid[i];
    for (int i = 0; i < 3; ++i) v[i] += dt * amid[i];
    quat_from_aa_unit(wdt, qf);
    pre_quat_mul(q, qf, qn);
    const double nn = sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
    for (int i = 0; i < 4; ++i) q[i] = qn[i] / nn;
  };

  for (int s = s0; s + 1 < s1; ++s) {                       // :96-102
    if (ts[s + 1] > te + 1e-12) break;
    increment(ts[s + 1] - ts[s], wm + 3 * s, am + 3 * s);
  }
  if (s1 > s0) {                                            // :104-108 remainder with the last sample
    const double dt = te - ts[s1 - 1];
    if (dt > 1e-12) increment(dt, wm + 3 * (s1 - 1), am + 3 * (s1 - 1));
  }
  // ComputeSqrtInvCov (:117-143)
  double n9 = 0.0, n6 = 0.0;
  for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) n9 += cov[i * 15 + j] * cov[i * 15 + j];
  for (int i = 9; i < 15; ++i) for (int j = 9; j < 15; ++j) n6 += cov[i * 15 + j] * cov[i * 15 + j];
  if (sqrt(n9) < 1e-5) for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) cov[i * 15 + j] = (i == j) ? 1e-5 : 0.0;
  if (sqrt(n6) < 1e-9) for (int i = 9; i < 15; ++i) for (int j = 9; j < 15; ++j) cov[i * 15 + j] = (i == j) ? 1e-9 : 0.0;
  // info = cov^-1 through cov = L L^T;  U = chol(info)^T  (cov.inverse().llt().matrixU())
  double L[225], Li[225];
  for (int i = 0; i < 225; ++i) L[i] = cov[i];
  bool ok = chol_lower<15>(L);
  double U[225];
  for (int i = 0; i < 225; ++i) U[i] = 0.0;
  if (ok) {
    for (int i = 0; i < 225; ++i) Li[i] = 0.0;
    for (int c = 0; c < 15; ++c)                      // Li = L^-1 (lower)
      for (int i = c; i < 15; ++i) {
        double s = (i == c) ? 1.0 : 0.0;
        for (int k = c; k < i; ++k) s -= L[i * 15 + k] * Li[k * 15 + c];
        Li[i * 15 + c] = s / L[i * 15 + i];
      }
    double info[225];
    for (int i = 0; i < 15; ++i) for (int j = 0; j < 15; ++j) { double s = 0.0; for (int k = (i > j ? i : j); k < 15; ++k) s += Li[k * 15 + i] * Li[k * 15 + j]; info[i * 15 + j] = s; }
    ok = chol_lower<15>(info);
    if (ok) for (int i = 0; i < 15; ++i) for (int j = 0; j <= i; ++j) { U[j * 15 + i] = info[i * 15 + j]; if (!std::isfinite(info[i * 15 + j])) ok = false; }
  }
  if (!ok) for (int i = 0; i < 225; ++i) U[i] = (i % 16 == 0) ? 1e-4 : 0.0;    // invalid_inv_cov_weight_ * I
  o[0] = dt_tot;
  for (int i = 0; i < 4; ++i) o[1 + i] = q[i];
  for (int i = 0; i < 3; ++i) { o[5 + i] = p[i]; o[8 + i] = v[i]; }
  for (int i = 0; i < 9; ++i) { o[11 + i] = dq_dbg.m[i]; o[20 + i] = dp_dbg.m[i]; o[29 + i] = dp_dba.m[i]; o[38 + i] = dv_dbg.m[i]; o[47 + i] = dv_dba.m[i]; }
  for (int i = 0; i < 3; ++i) { o[56 + i] = bg[i]; o[59 + i] = ba[i]; }
  for (int i = 0; i < 225; ++i) o[62 + i] = info_weight * U[i];
}

// The same interval without covariance and information — Integrate(te, bg, ba, jacobian, no covariance, no information), what
// imu::EstimateParameters asks of its frames (inertial_align.h).  Increment's state update and its dq_dbg update with the arithmetic
// of preintegrate_interval's `increment`; nothing of the 15 x 15 covariance, its two Cholesky factorisations or the other four
// bias Jacobians.  s_bridge >= 0: one increment of ts[s0] - t_bridge with the sample s_bridge runs first (skipped, like the
// remainder, when it is not longer than 1e-12), so that the delta starts at t_bridge instead of at its first sample.
constexpr int kPreintDelta = 20;   // dt, dq[4], dp[3], dv[3], dq_dbg[9]
BSG_PRE_FN void preintegrate_delta(int s0, int s1, const double* __restrict__ ts, const double* __restrict__ wm,
                                   const double* __restrict__ am, double te, const double* __restrict__ bg_in,
                                   const double* __restrict__ ba_in, int s_bridge, double t_bridge, double* __restrict__ o) {
  const double bg[3] = {bg_in[0], bg_in[1], bg_in[2]}, ba[3] = {ba_in[0], ba_in[1], ba_in[2]};
  double dt_tot = 0.0, q[4] = {1, 0, 0, 0}, p[3] = {0, 0, 0}, v[3] = {0, 0, 0};
  M3 dq_dbg = m3_zero();

  auto increment = [&](double dt, const double* wraw, const double* araw) {   // preintegrator.cpp:26-36, :78-88
    const double w[3] = {wraw[0] - bg[0], wraw[1] - bg[1], wraw[2] - bg[2]}, a[3] = {araw[0] - ba[0], araw[1] - ba[1], araw[2] - ba[2]};
    const double wdt[3] = {w[0] * dt, w[1] * dt, w[2] * dt}, whalf[3] = {0.5 * wdt[0], 0.5 * wdt[1], 0.5 * wdt[2]};
    const M3 R_full = so3_exp(wdt), Jr = so3_jr(wdt);
    const M3 Rt = m3_t(R_full);
    dq_dbg = m3_axpy(-dt, Jr, m3_mul(Rt, dq_dbg));
    double qh[4], qm[4], qf[4], qn[4];
    quat_from_aa_unit(whalf, qh);
    pre_quat_mul(q, qh, qm);
    const M3 Rm = pre_quat_to_rot(qm);
    const double amid[3] = {Rm.m[0] * a[0] + Rm.m[1] * a[1] + Rm.m[2] * a[2], Rm.m[3] * a[0] + Rm.m[4] * a[1] + Rm.m[5] * a[2],
                            Rm.m[6] * a[0] + Rm.m[7] * a[1] + Rm.m[8] * a[2]};
    dt_tot += dt;
    for (int i = 0; i < 3; ++i) p[i] += dt * v[i] + 0.5 * dt * dt * amid[i];
    for (int i = 0; i < 3; ++i) v[i] += dt * amid[i];
    quat_from_aa_unit(wdt, qf);
    pre_quat_mul(q, qf, qn);
    const double nn = sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
    for (int i = 0; i < 4; ++i) q[i] = qn[i] / nn;
  };

  if (s_bridge >= 0 && s1 > s0) {
    const double dt = ts[s0] - t_bridge;
    if (dt > 1e-12) increment(dt, wm + 3 * s_bridge, am + 3 * s_bridge);
  }
  for (int s = s0; s + 1 < s1; ++s) {                       // :96-102
    if (ts[s + 1] > te + 1e-12) break;
    increment(ts[s + 1] - ts[s], wm + 3 * s, am + 3 * s);
  }
  if (s1 > s0) {                                            // :104-108 remainder with the last sample
    const double dt = te - ts[s1 - 1];
    if (dt > 1e-12) increment(dt, wm + 3 * (s1 - 1), am + 3 * (s1 - 1));
  }
  o[0] = dt_tot;
  for (int i = 0; i < 4; ++i) o[1 + i] = q[i];
  for (int i = 0; i < 3; ++i) { o[5 + i] = p[i]; o[8 + i] = v[i]; }
  for (int i = 0; i < 9; ++i) o[11 + i] = dq_dbg.m[i];
}

}  // namespace bsg
