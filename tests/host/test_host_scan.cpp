// bs_models::scan_registration::ScanMatcher (beam_slam_amd/host/scan_matcher.h): the motion-threshold gate, the batched call, the
// composition of T_LIDARREF_LIDARTGT and RegistrationValidation around one bsgpu_register_scans call.  Built three ways by
// tests/test_host_scan_matcher.py: against libbsgpu.so; with -DSCAN_STANDIN, where the stand-in below answers the C-ABI call pair by
// pair with icp.h on one core; and with -DSCAN_NO_BACKEND, where nothing defines the entry point.
#include <cmath>
#include <cstdio>

#include "../../beam_slam_amd/host/scan_matcher.h"

#ifdef SCAN_STANDIN
#include "icp.h"
extern "C" int bsgpu_register_scans(int, int32_t n_pairs, const int32_t* ref_start, const double* ref_points, const int32_t* tgt_start,
                                    const double* tgt_points, const double* T_init, double max_corr, int32_t max_iter, double t_eps,
                                    double fit_eps, double rotation_threshold, double rel_mse_eps, double* T_refest_ref, double* T_ref_tgt,
                                    double* mse, int32_t* n_corr, int32_t* n_iters, int32_t* status) {
  const bsg::IcpParams P{max_iter, t_eps, fit_eps, rotation_threshold, rel_mse_eps};
  for (int p = 0; p < n_pairs; ++p)
    if (!bsg::icp_register_serial(ref_start[p + 1] - ref_start[p], ref_points + 3 * (size_t)ref_start[p], tgt_start[p + 1] - tgt_start[p],
                                  tgt_points + 3 * (size_t)tgt_start[p], T_init ? T_init + 12 * p : nullptr, max_corr, P,
                                  (double)BSGPU_ICP_MAX_CELLS, T_refest_ref + 12 * p, T_ref_tgt + 12 * p, mse + p, n_corr + p, n_iters + p,
                                  status + p))
      return BSGPU_ERR_UNSUPPORTED;
  return BSGPU_OK;
}
#endif

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using namespace bs_models::scan_registration;

static Mat4 pose(double rx, double ry, double rz, double x, double y, double z) {
  const bs_math::Mat3 R = bs_math::so3Exp({rx, ry, rz});
  Mat4 T = Mat4::Identity();
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T(i, j) = R(i, j);
  T(0, 3) = x; T(1, 3) = y; T(2, 3) = z;
  return T;
}
static void print(const char* tag, int k, const Mat4& T) {
  std::printf("%s %d", tag, k);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) std::printf(" %.17g", T(i, j));
  std::printf("\n");
}

int main() {
#if !defined(SCAN_STANDIN) && !defined(SCAN_NO_BACKEND)
  // a strong reference: the header's is weak, and a linker that drops libraries nothing needs would leave the entry point unbound
  CHECK(bsgpu_abi_version() == 1);
#endif
  // ---- PassedMotionThresholds: its three returns (scan_registration_base.cpp:200-206) and the translation ceiling --------------------
  const Mat4 still = pose(0, 0, 0.001, 0.01, 0, 0), turned = pose(0, 0, 0.2, 0.01, 0, 0), moved = pose(0, 0, 0.001, 1.0, 0, 0),
             far = pose(0, 0, 0, 11.0, 0, 0);
  {
    ScanMatcher none(0, {}, {0.0, 0.0, 10.0}), trans(0, {}, {0.5, 0.0, 10.0}), rot(0, {}, {0.0, 5.0, 10.0}), both(0, {}, {0.5, 5.0, 10.0}),
        no_ceiling(0, {}, {0.0, 0.0, 0.0});
    CHECK(none.PassedMotionThresholds(still) && !none.PassedMotionThresholds(far) && no_ceiling.PassedMotionThresholds(far));
    CHECK(!trans.PassedMotionThresholds(still) && !trans.PassedMotionThresholds(turned) && trans.PassedMotionThresholds(moved));   // rotation not looked at
    CHECK(!rot.PassedMotionThresholds(still) && rot.PassedMotionThresholds(turned) && !rot.PassedMotionThresholds(moved));        // translation not looked at
    CHECK(!both.PassedMotionThresholds(still) && both.PassedMotionThresholds(turned) && both.PassedMotionThresholds(moved));      // either
    CHECK(std::fabs(RotationAngle(turned) - 0.2) < 1e-15 && std::fabs(RotationAngle(pose(3.0, 0, 0, 0, 0, 0)) - 3.0) < 1e-12);
  }
  // ---- RegistrationValidation on a hand-made metric list ---------------------------------------------------------------------------
  {
    RegistrationValidation v;
    CHECK(v.Validate(RegistrationMetrics{0.1, 0.2, -10.0}));
    CHECK(!v.Validate(RegistrationMetrics{0.1, 0.6, -10.0}));               // initial branch: t > 0.5
    CHECK(!v.Validate(RegistrationMetrics{0.6, 0.2, -10.0}));               //                 r > 3.14 / 6
    CHECK(!v.Validate(RegistrationMetrics{0.1, 0.2, -3.0}));                //                 entropy > -4
    RegistrationValidation w;
    for (int i = 0; i < 15; ++i) CHECK(w.Validate(RegistrationMetrics{0.10 + 0.001 * (i % 3), 0.20 + 0.002 * (i % 2), -10.0}));
    CHECK(w.metrics().size() == 15);
    CHECK(w.Validate(RegistrationMetrics{0.101, 0.201, -10.0}));            // windowed branch: inside mean +- 2 sigma; the sums start at 0
    CHECK(w.metrics().size() == 15);
    CHECK(!w.Validate(RegistrationMetrics{0.2, 0.201, -10.0}));             // rotation far above the window's mean + 2 sigma
    CHECK(!w.Validate(RegistrationMetrics{0.101, 0.05, -10.0}));            // translation below mean - 2 sigma
    Cov6 c = ScanMatcher::DefaultCovariance();
    CHECK(std::fabs(ShannonEntropyFromPoseCovariance(c) - 0.5 * (6.0 * std::log(2.0 * M_PI * std::exp(1.0)) + 6.0 * std::log(1e-3))) < 1e-12);
    c(0, 1) = c(1, 0) = 5e-4;                                               // det = (1e-6 - 2.5e-7) 1e-12
    CHECK(std::fabs(ShannonEntropyFromPoseCovariance(c) - 0.5 * (6.0 * std::log(2.0 * M_PI * std::exp(1.0)) + std::log(7.5e-19))) < 1e-12);
  }
  // ---- MatchScans: a box seen from two lidar poses, the target's pose estimate 10 cm and half a degree off -----------------------------
  std::vector<double> world;
  uint64_t lcg = 12345;
  const auto uni = [&] { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992.0 - 0.5; };
  const double box[3] = {20.0, 14.0, 5.0};
  for (int i = 0; i < 1500; ++i) {
    double p[3] = {uni() * box[0], uni() * box[1], uni() * box[2]};
    const int face = i % 6;
    p[face / 2] = (face % 2 ? 0.5 : -0.5) * box[face / 2];
    world.insert(world.end(), p, p + 3);
  }
  const auto seen_from = [&](const Mat4& T_WORLD_LIDAR, int first, int step) {
    const Mat4 Ti = InvertTransform(T_WORLD_LIDAR);
    std::vector<double> cloud;
    for (size_t i = first; i < world.size() / 3; i += step)
      for (int a = 0; a < 3; ++a) cloud.push_back(Ti(a, 0) * world[3 * i] + Ti(a, 1) * world[3 * i + 1] + Ti(a, 2) * world[3 * i + 2] + Ti(a, 3));
    return cloud;
  };
  const Mat4 T_ref = pose(0, 0, 0.3, 1.0, -0.5, 0.1), T_ref2 = pose(0, 0.01, 0.28, 1.1, -0.4, 0.1), T_tgt = pose(0.01, -0.02, 0.34, 1.25, -0.65, 0.15);
  ScanPose ref, ref2, ref_far, tgt;
  ref.T_REFFRAME_LIDAR = T_ref; ref.cloud = seen_from(T_ref, 0, 1);
  ref2.T_REFFRAME_LIDAR = T_ref2; ref2.cloud = seen_from(T_ref2, 0, 1);
  ref_far.T_REFFRAME_LIDAR = pose(0, 0, 0, 20.0, 0, 0); ref_far.cloud = ref.cloud;
  tgt.T_REFFRAME_LIDAR = T_tgt * pose(0.004, -0.003, 0.008, 0.08, -0.05, 0.03);   // the estimate; the cloud is seen from the true pose
  tgt.cloud = seen_from(T_tgt, 0, 1);
  ScanMatcher matcher;
  const std::vector<ScanMatch> res = matcher.MatchScansBatch({&ref, &ref_far, &ref2}, tgt);
  CHECK(res.size() == 3 && !res[1].passed_motion && !res[1].matched && res[1].status == -1);
  const ScanPose* refs[3] = {&ref, &ref_far, &ref2};
  for (int k = 0; k < 3; ++k) {
    const ScanMatch& m = res[k];
    std::printf("STATUS %d %d %d %d %d %d %d %d %.17g\n", k, m.matched ? 1 : 0, m.passed_motion ? 1 : 0, m.converged ? 1 : 0, m.validated ? 1 : 0,
                m.status, m.n_iters, m.n_corr, m.mse);
    if (!m.converged) continue;
    print("TINIT", k, InvertTransform(refs[k]->T_REFFRAME_LIDAR) * tgt.T_REFFRAME_LIDAR);
    print("TEST", k, m.T_RefEst_Ref);
    print("TOUT", k, m.T_LIDARREF_LIDARTGT);
    print("TRUE", k, InvertTransform(refs[k]->T_REFFRAME_LIDAR) * T_tgt);
  }
#ifdef SCAN_NO_BACKEND
  CHECK(!res[0].matched && res[0].passed_motion && res[0].status == -1 && matcher.validation().metrics().empty());
#else
  CHECK(res[0].matched && res[2].matched && matcher.validation().metrics().size() == 2);
#endif
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("HOST SCAN MATCHER DONE\n");
  return 0;
}
