// The Unicycle3D kinematic constraint (BSGPU_F_UNICYCLE): bs_constraints::Unicycle3DStateKinematicConstraint
// (src/motion/unicycle_3d_state_kinematic_constraint.cpp:11-31,73-77), evaluated by Ceres as
// AutoDiffCostFunction<Unicycle3DStateCostFunctor, 15, 3,4,3,3,3, 3,4,3,3,3>
// (motion/unicycle_3d_state_cost_functor.h:65-125) around the prediction of motion/unicycle_3d_predict.h:49-196.
//
// Host- and device-compilable, in the style of frame_lm.h: unicycle_body (k_small.hip) runs it a wave per factor, one raw tangent
// column per lane; tests/plan/unicycle_body_capi.cpp exposes the same functions on the CPU for tests/test_unicycle_body.py.
//
//   e = [ p2 - p^ ; wrap(rpy(q2) - rpy^) ; v2 - v^ ; w2 - w^ ; a2 - a^ ]      r = A e
//   p^ = p1 + R(roll1, pitch1, yaw1) (v1 dt + a1 dt^2 / 2),  rpy^ = wrap(rpy(q1) + T(roll1, pitch1) w1 dt),  v^ = v1 + a1 dt,
//   w^ = w1, a^ = a1
// The tangent Jacobian is the ambient one (what AutoDiff gives, wrap and the pitch clamp with derivative 0 included) times the
// 4x3 PlusJacobian of each orientation block, not the Lie derivative: the two differ for |q| != 1.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define BSG_UNI_FN __host__ __device__ __forceinline__
#else
#define BSG_UNI_FN inline
#endif

namespace bsg {

constexpr double kUniPi = 3.14159265358979323846;

// [EXT] fuse_core::wrapAngle2D: to [-pi, pi); derivative 1
BSG_UNI_FN double uni_wrap(double a) {
  const double two_pi = 2.0 * kUniPi;
  return a - two_pi * floor((a + kUniPi) / two_pi);
}

// [EXT] fuse_core::getRoll / getPitch / getYaw on the stored (w, x, y, z), not renormalised; d: their 3x4 derivative (row-major)
BSG_UNI_FN void uni_rpy(const double q[4], double rpy[3]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  rpy[0] = atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y));
  const double s = 2.0 * (w * y - z * x);
  rpy[1] = fabs(s) >= 1.0 ? (s >= 0.0 ? 1.0 : -1.0) * (kUniPi / 2.0) : asin(s);
  rpy[2] = atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z));
}
BSG_UNI_FN void uni_rpy_jac(const double q[4], double d[12]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  {  // atan2(S, C): (C dS - S dC) / (S^2 + C^2)
    const double S = 2.0 * (w * x + y * z), C = 1.0 - 2.0 * (x * x + y * y), k = 1.0 / (S * S + C * C);
    const double dS[4] = {2.0 * x, 2.0 * w, 2.0 * z, 2.0 * y}, dC[4] = {0.0, -4.0 * x, -4.0 * y, 0.0};
    for (int j = 0; j < 4; ++j) d[j] = k * (C * dS[j] - S * dC[j]);
  }
  {
    const double s = 2.0 * (w * y - z * x);
    const double k = fabs(s) >= 1.0 ? 0.0 : 1.0 / sqrt(1.0 - s * s);
    d[4] = k * 2.0 * y; d[5] = -k * 2.0 * z; d[6] = k * 2.0 * w; d[7] = -k * 2.0 * x;
  }
  {
    const double S = 2.0 * (w * z + x * y), C = 1.0 - 2.0 * (y * y + z * z), k = 1.0 / (S * S + C * C);
    const double dS[4] = {2.0 * z, 2.0 * y, 2.0 * x, 2.0 * w}, dC[4] = {0.0, 0.0, -4.0 * y, -4.0 * z};
    for (int j = 0; j < 4; ++j) d[8 + j] = k * (C * dS[j] - S * dC[j]);
  }
}
// d rpy / d theta_i: the 3x4 derivative times column i of the PlusJacobian of x (x) AngleAxisToQuaternion(theta)
BSG_UNI_FN void uni_rpy_tangent(const double q[4], int i, double g[3]) {
  // column i of the PlusJacobian over 1/2: rows w, x, y, z of [-x -y -z; w -z y; z w -x; -y x w]
  // (weights, not selects of q[.]: a select of two loads becomes a load at a computed index, and q then lives in scratch on the device)
  const double e0 = i == 0 ? 1.0 : 0.0, e1 = i == 1 ? 1.0 : 0.0, e2 = i == 2 ? 1.0 : 0.0;
  const double P0 = -(e0 * q[1] + e1 * q[2] + e2 * q[3]);
  const double P1 = e0 * q[0] - e1 * q[3] + e2 * q[2];
  const double P2 = e0 * q[3] + e1 * q[0] - e2 * q[1];
  const double P3 = -e0 * q[2] + e1 * q[1] + e2 * q[0];
  double d[12];
  uni_rpy_jac(q, d);
  for (int r = 0; r < 3; ++r) g[r] = 0.5 * (d[4 * r] * P0 + d[4 * r + 1] * P1 + d[4 * r + 2] * P2 + d[4 * r + 3] * P3);
}

// what the Jacobian columns need of the first state, kept from the residual
struct UniLin {
  double sr, cr, sp, cp, cpi, tp, sy, cy;
  double u[3];      // v1 + a1 dt / 2: p^ = p1 + dt R u
  double w1[3];
  double dt;
};

// the unweighted error e (15) of the blocks' ambient values, in the reference's order of operations
BSG_UNI_FN void uni_error(const double p1[3], const double q1[4], const double v1[3], const double w1[3], const double a1[3],
                          const double p2[3], const double q2[4], const double v2[3], const double w2[3], const double a2[3],
                          const double dt, double e[15], UniLin* L) {
  double rpy1[3], rpy2[3];
  uni_rpy(q1, rpy1);
  uni_rpy(q2, rpy2);
  const double sp = sin(rpy1[1]), cp = cos(rpy1[1]), cpi = 1.0 / cp, tp = sp * cpi;
  const double sr = sin(rpy1[0]), cr = cos(rpy1[0]);
  const double sy = sin(rpy1[2]), cy = cos(rpy1[2]);
  const double VX = v1[0], VY = v1[1], VZ = v1[2], AX = a1[0], AY = a1[1], AZ = a1[2];
  const double VR = w1[0], VP = w1[1], VYAW = w1[2];
  const double X_VX = cy * cp * dt, X_VY = (cy * sp * sr - sy * cr) * dt, X_VZ = (cy * sp * cr + sy * sr) * dt;
  const double X_AX = 0.5 * X_VX * dt, X_AY = 0.5 * X_VY * dt, X_AZ = 0.5 * X_VZ * dt;
  const double Y_VX = sy * cp * dt, Y_VY = (sy * sp * sr + cy * cr) * dt, Y_VZ = (sy * sp * cr - cy * sr) * dt;
  const double Y_AX = 0.5 * Y_VX * dt, Y_AY = 0.5 * Y_VY * dt, Y_AZ = 0.5 * Y_VZ * dt;
  const double Z_VX = -sp * dt, Z_VY = cp * sr * dt, Z_VZ = cp * cr * dt;
  const double Z_AX = (0.5 * Z_VX) * dt, Z_AY = (0.5 * Z_VY) * dt, Z_AZ = (0.5 * Z_VZ) * dt;
  const double ROLL_VR = dt, ROLL_VP = sr * tp * dt, ROLL_VY = cr * tp * dt;
  const double PITCH_VP = cr * dt, PITCH_VY = -sr * dt;
  const double YAW_VP = sr * cpi * dt, YAW_VY = cr * cpi * dt;
  const double px = p1[0] + VX * X_VX + VY * X_VY + VZ * X_VZ + AX * X_AX + AY * X_AY + AZ * X_AZ;
  const double py = p1[1] + VX * Y_VX + VY * Y_VY + VZ * Y_VZ + AX * Y_AX + AY * Y_AY + AZ * Y_AZ;
  const double pz = p1[2] + VX * Z_VX + VY * Z_VY + VZ * Z_VZ + AX * Z_AX + AY * Z_AY + AZ * Z_AZ;
  const double roll = uni_wrap(rpy1[0] + VR * ROLL_VR + VP * ROLL_VP + VYAW * ROLL_VY);
  const double pitch = uni_wrap(rpy1[1] + VP * PITCH_VP + VYAW * PITCH_VY);
  const double yaw = uni_wrap(rpy1[2] + VP * YAW_VP + VYAW * YAW_VY);
  e[0] = p2[0] - px; e[1] = p2[1] - py; e[2] = p2[2] - pz;
  e[3] = uni_wrap(rpy2[0] - roll); e[4] = uni_wrap(rpy2[1] - pitch); e[5] = uni_wrap(rpy2[2] - yaw);
  e[6] = v2[0] - (VX + AX * dt); e[7] = v2[1] - (VY + AY * dt); e[8] = v2[2] - (VZ + AZ * dt);
  e[9] = w2[0] - VR; e[10] = w2[1] - VP; e[11] = w2[2] - VYAW;
  e[12] = a2[0] - AX; e[13] = a2[1] - AY; e[14] = a2[2] - AZ;
  if (L) {
    L->sr = sr; L->cr = cr; L->sp = sp; L->cp = cp; L->cpi = cpi; L->tp = tp; L->sy = sy; L->cy = cy;
    for (int k = 0; k < 3; ++k) { L->u[k] = v1[k] + 0.5 * a1[k] * dt; L->w1[k] = w1[k]; }
    L->dt = dt;
  }
}

// raw tangent column k (< 30) of d e / d delta: block k / 3 of (p1, q1, v1, w1, a1, p2, q2, v2, w2, a2), component k % 3
BSG_UNI_FN void uni_column(const UniLin& L, const double q1[4], const double q2[4], const int k, double col[15]) {
  for (int m = 0; m < 15; ++m) col[m] = 0.0;
  const int b = k / 3, i = k % 3;
  const double sr = L.sr, cr = L.cr, sp = L.sp, cp = L.cp, cpi = L.cpi, tp = L.tp, sy = L.sy, cy = L.cy, dt = L.dt;
  // R(roll, pitch, yaw) column i (the transfer terms X_V*, Y_V*, Z_V* over dt)
  const double Ri[3] = {i == 0 ? cy * cp : i == 1 ? cy * sp * sr - sy * cr : cy * sp * cr + sy * sr,
                        i == 0 ? sy * cp : i == 1 ? sy * sp * sr + cy * cr : sy * sp * cr - cy * sr,
                        i == 0 ? -sp : i == 1 ? cp * sr : cp * cr};
  switch (b) {
    case 0: col[i] = -1.0; break;
    case 1: {
      double g[3];
      uni_rpy_tangent(q1, i, g);
      const double* u = L.u;
      // d p^ / d (roll, pitch, yaw) = dt dR/d(.) u
      const double dPr[3] = {dt * ((cy * sp * cr + sy * sr) * u[1] + (-cy * sp * sr + sy * cr) * u[2]),
                             dt * ((sy * sp * cr - cy * sr) * u[1] + (-sy * sp * sr - cy * cr) * u[2]),
                             dt * (cp * cr * u[1] - cp * sr * u[2])};
      const double dPp[3] = {dt * (-cy * sp * u[0] + cy * cp * sr * u[1] + cy * cp * cr * u[2]),
                             dt * (-sy * sp * u[0] + sy * cp * sr * u[1] + sy * cp * cr * u[2]),
                             dt * (-cp * u[0] - sp * sr * u[1] - sp * cr * u[2])};
      const double dPy[3] = {dt * (-sy * cp * u[0] + (-sy * sp * sr - cy * cr) * u[1] + (-sy * sp * cr + cy * sr) * u[2]),
                             dt * (cy * cp * u[0] + (cy * sp * sr - sy * cr) * u[1] + (cy * sp * cr + sy * sr) * u[2]), 0.0};
      for (int m = 0; m < 3; ++m) col[m] = -(dPr[m] * g[0] + dPp[m] * g[1] + dPy[m] * g[2]);
      // d rpy^ / d (roll, pitch, yaw)
      const double VP = L.w1[1], VY = L.w1[2];
      const double a = (VP * cr - VY * sr) * dt, c = (VP * sr + VY * cr) * dt;
      col[3] = -((1.0 + a * tp) * g[0] + c * cpi * cpi * g[1]);
      col[4] = -(-c * g[0] + g[1]);
      col[5] = -(a * cpi * g[0] + c * tp * cpi * g[1] + g[2]);
    } break;
    case 2:
      for (int m = 0; m < 3; ++m) col[m] = -Ri[m] * dt;
      col[6 + i] = -1.0;
      break;
    case 3:
      // d rpy^ / d (VR, VP, VY), column i
      col[3] = -(i == 0 ? dt : i == 1 ? sr * tp * dt : cr * tp * dt);
      col[4] = -(i == 0 ? 0.0 : i == 1 ? cr * dt : -sr * dt);
      col[5] = -(i == 0 ? 0.0 : i == 1 ? sr * cpi * dt : cr * cpi * dt);
      col[9 + i] = -1.0;
      break;
    case 4:
      for (int m = 0; m < 3; ++m) col[m] = -0.5 * (Ri[m] * dt) * dt;
      col[6 + i] = -dt;
      col[12 + i] = -1.0;
      break;
    case 5: col[i] = 1.0; break;
    case 6: uni_rpy_tangent(q2, i, col + 3); break;
    case 7: col[6 + i] = 1.0; break;
    case 8: col[9 + i] = 1.0; break;
    default: col[12 + i] = 1.0; break;
  }
}

}  // namespace bsg
