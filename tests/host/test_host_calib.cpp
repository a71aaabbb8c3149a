// Online calibration in a GpuGraph: four key frames held by tight pose priors, 30 landmarks, every observation a
// bs_constraints::EuclideanReprojectionConstraintOnlineCalib naming one extrinsic pair (bs_variables::Orientation3D / Position3D) that
// starts off its true value under the calibration prior of VisualMap::AddCameraCalibration (bs_models/src/lib/vision/visual_map.cpp:610-618:
// AbsolutePose3DConstraint, covariance 1e-5 I).  Built by tests/test_host_online_calib.py against either back-end.
//   "free": the pair is released (setHoldConstant(false)) before it is added — the optimised extrinsic is read back from the graph, as
//           VisualOdometry::onGraphUpdate does (bs_models/src/visual_odometry.cpp:352-361);
//   "held": the default, holdConstant() == true — it must not move.
#include <cstdio>
#include <cmath>
#include <cstring>
#include <random>

#include "../../beam_slam_amd/host/fixed_lag_smoother.h"

using namespace bs_math;

static void quat_rot(const double* q, double R[9]) {   // Eigen's toRotationMatrix, row-major
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

int main(int argc, char** argv) {
  const bool release = argc > 1 && std::strcmp(argv[1], "free") == 0;
  std::mt19937 rng(5);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> N(0.0, 1.0);
  Mat<3, 3> K = Mat<3, 3>::Identity(); K(0, 0) = 458.654; K(1, 1) = 457.296; K(0, 2) = 367.215; K(1, 2) = 248.375;
  const int n_kf = 4, n_lm = 30;
  bs_optimizers::GpuGraph graph;
  // the true extrinsic T_BASELINK_CAM and where the graph starts it
  const double a_t = 0.04;
  const double q_bc_true[4] = {std::cos(a_t / 2), 0.0, std::sin(a_t / 2), 0.0}, p_bc_true[3] = {0.05, -0.02, 0.03};
  auto ext_q = bs_variables::Orientation3D::make_shared("cam", "baselink");
  auto ext_p = bs_variables::Position3D::make_shared("cam", "baselink");
  const double a_0 = 0.06;
  ext_q->data()[0] = std::cos(a_0 / 2); ext_q->data()[1] = 0.0; ext_q->data()[2] = std::sin(a_0 / 2); ext_q->data()[3] = 0.0;
  ext_p->data()[0] = 0.07; ext_p->data()[1] = -0.04; ext_p->data()[2] = 0.05;
  if (release) { ext_q->setHoldConstant(false); ext_p->setHoldConstant(false); }
  graph.addVariable(ext_q); graph.addVariable(ext_p);
  Mat<6, 6> cov_calib = Mat<6, 6>::Identity(); for (int i = 0; i < 6; ++i) cov_calib(i, i) = 1e-5;
  const double* q0 = ext_q->data(); const double* p0 = ext_p->data();
  graph.addConstraint(std::make_shared<bs_constraints::AbsolutePose3DConstraint>(
      "calibration", *ext_p, *ext_q, bs_constraints::Vector7d{p0[0], p0[1], p0[2], q0[0], q0[1], q0[2], q0[3]}, cov_calib));
  // key frames that turn about two axes (the pair's translation is seen through their rotation), held at the truth
  std::vector<fuse_variables::Orientation3DStamped::SharedPtr> qs;
  std::vector<fuse_variables::Position3DStamped::SharedPtr> ps;
  Mat<6, 6> cov6 = Mat<6, 6>::Identity(); for (int i = 0; i < 6; ++i) cov6(i, i) = 1e-8;
  for (int k = 0; k < n_kf; ++k) {
    auto q = fuse_variables::Orientation3DStamped::make_shared(fuse_core::Time(1.0 + 0.1 * k));
    auto p = fuse_variables::Position3DStamped::make_shared(fuse_core::Time(1.0 + 0.1 * k));
    const double az = 0.5 * k, ay = 0.1 * k;   // q = qz(az) * qy(ay)
    const double cz = std::cos(az / 2), sz = std::sin(az / 2), cy = std::cos(ay / 2), sy = std::sin(ay / 2);
    q->data()[0] = cz * cy; q->data()[1] = -sz * sy; q->data()[2] = cz * sy; q->data()[3] = sz * cy;
    p->data()[0] = 0.3 * k; p->data()[1] = 0.05 * k * k; p->data()[2] = 0.02 * k;
    graph.addVariable(q); graph.addVariable(p);
    const double* qd = q->data(); const double* pd = p->data();
    graph.addConstraint(std::make_shared<fuse_constraints::AbsolutePose3DStampedConstraint>(
        "prior", *p, *q, bs_constraints::Vector7d{pd[0], pd[1], pd[2], qd[0], qd[1], qd[2], qd[3]}, cov6));
    qs.push_back(q); ps.push_back(p);
  }
  double R_bc[9];
  quat_rot(q_bc_true, R_bc);
  int n_obs = 0;
  for (int l = 0; l < n_lm; ++l) {
    // a point in front of key frame 0's camera, in the world
    const double z = 4.0 + 6.0 * U(rng), x = (U(rng) - 0.5) * 0.6 * z, y = (U(rng) - 0.5) * 0.4 * z;
    double R0[9];
    quat_rot(qs[0]->data(), R0);
    double Pb[3], Pw[3];
    for (int i = 0; i < 3; ++i) Pb[i] = R_bc[3 * i] * x + R_bc[3 * i + 1] * y + R_bc[3 * i + 2] * z + p_bc_true[i];
    for (int i = 0; i < 3; ++i) Pw[i] = R0[3 * i] * Pb[0] + R0[3 * i + 1] * Pb[1] + R0[3 * i + 2] * Pb[2] + ps[0]->data()[i];
    auto lm = bs_variables::Point3DLandmark::make_shared((uint64_t)(100 + l));
    lm->x() = Pw[0] + 0.05 * N(rng); lm->y() = Pw[1] + 0.05 * N(rng); lm->z() = Pw[2] + 0.05 * N(rng);
    graph.addVariable(lm);
    for (int k = 0; k < n_kf; ++k) {
      double Rk[9], d[3], pb[3], pc[3];
      quat_rot(qs[k]->data(), Rk);
      for (int i = 0; i < 3; ++i) d[i] = Pw[i] - ps[k]->data()[i];
      for (int i = 0; i < 3; ++i) pb[i] = Rk[i] * d[0] + Rk[3 + i] * d[1] + Rk[6 + i] * d[2] - p_bc_true[i];
      for (int i = 0; i < 3; ++i) pc[i] = R_bc[i] * pb[0] + R_bc[3 + i] * pb[1] + R_bc[6 + i] * pb[2];
      if (pc[2] < 1.0) continue;
      const std::array<double, 2> uv = {K(0, 0) * pc[0] / pc[2] + K(0, 2), K(1, 1) * pc[1] / pc[2] + K(1, 2)};
      auto c = std::make_shared<bs_constraints::EuclideanReprojectionConstraintOnlineCalib>("vo", *qs[k], *ps[k], *lm, *ext_q, *ext_p, K, uv, 1.0);
      c->loss(std::make_shared<fuse_loss::CauchyLoss>(5.0));
      graph.addConstraint(c);
      ++n_obs;
    }
  }
  std::printf("OBS %d\n", n_obs);
  std::printf("TRUE %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", q_bc_true[0], q_bc_true[1], q_bc_true[2], q_bc_true[3], p_bc_true[0], p_bc_true[1], p_bc_true[2]);
  std::printf("X0 %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", q0[0], q0[1], q0[2], q0[3], p0[0], p0[1], p0[2]);
  auto summary = graph.optimize();
  if (!summary.IsSolutionUsable()) { std::printf("solve not usable: %s\n", summary.message.c_str()); return 1; }
  const fuse_core::Variable& q1 = graph.getVariable(ext_q->uuid());
  const fuse_core::Variable& p1 = graph.getVariable(ext_p->uuid());
  std::printf("X %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", q1.data()[0], q1.data()[1], q1.data()[2], q1.data()[3], p1.data()[0], p1.data()[1], p1.data()[2]);
  std::printf("cost %.17g %.17g\n", summary.initial_cost, summary.final_cost);
  std::printf("HOST CALIB DONE\n");
  return 0;
}
