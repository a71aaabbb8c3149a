// bs_models::FrameLocalizer (beam_slam_amd/host/frame_localizer.h): LocalizeFrame's gate, fallback, pose conversions and covariance
// order around one bsgpu_localize_frames call.  Built twice by tests/test_host_frame_localizer.py: against libbsgpu.so, and against the
// CPU oracle (tests/host/oracle_backend.h), where the stand-in below answers bsgpu_localize_frames frame by frame with the oracle's
// solve of the one-pose BSGPU_F_REPROJ problem and its covariance blocks.
#include <cmath>
#include <cstdio>
#include <random>

#include "../../beam_slam_amd/host/frame_localizer.h"

using namespace bs_math;
using bs_models::FrameInput;

static bsgpu_camera g_cam;

#ifdef bsgpu_solve   // the oracle back-end: bsgpu_* names are the oracle's
extern "C" int bsgpu_localize_frames(bsgpu_ctx*, int32_t n_frames, const int32_t* obs_start, const double* pixels, const double* points,
                                     const int32_t*, const int32_t*, const double* q_init, const double* p_init, int32_t loss_kind,
                                     double loss_a, double sqrt_info, int32_t truncate_pixels, int32_t min_points, int32_t, int32_t,
                                     const bsgpu_options* options, double* q_out, double* p_out, double* cov_out, double* avg_reproj,
                                     double* final_cost, int32_t* iterations, int32_t* status) {
  for (int f = 0; f < n_frames; ++f) {
    const int o0 = obs_start[f], n = obs_start[f + 1] - o0;
    for (int i = 0; i < 4; ++i) q_out[4 * f + i] = q_init[4 * f + i];
    for (int i = 0; i < 3; ++i) p_out[3 * f + i] = p_init[3 * f + i];
    for (int i = 0; i < 36; ++i) cov_out[36 * f + i] = NAN;
    if (avg_reproj) avg_reproj[f] = 0.0;
    if (n < min_points) { status[f] = 1; continue; }
    std::vector<double> v(q_init + 4 * f, q_init + 4 * f + 4);
    v.insert(v.end(), p_init + 3 * f, p_init + 3 * f + 3);
    v.insert(v.end(), points + 3 * o0, points + 3 * (o0 + n));
    const int nb = 2 + n;
    std::vector<int32_t> off(nb), idx;
    std::vector<uint8_t> size(nb, 3), man(nb, BSGPU_MANIFOLD_EUCLIDEAN), cst(nb, 1);
    std::vector<double> consts;
    off[0] = 0; size[0] = 4; man[0] = BSGPU_MANIFOLD_QUAT_RIGHT; cst[0] = 0; off[1] = 4; cst[1] = 0;
    for (int i = 0; i < n; ++i) {
      off[2 + i] = 7 + 3 * i;
      idx.insert(idx.end(), {0, 1, 2 + i, 0});
      const double* z = pixels + 2 * (o0 + i);
      consts.insert(consts.end(), {truncate_pixels ? std::trunc(z[0]) : z[0], truncate_pixels ? std::trunc(z[1]) : z[1], sqrt_info});
    }
    std::vector<int32_t> lk(n, loss_kind);
    std::vector<double> la(n, loss_a);
    bsgpu_ctx* c = bsgpu_create(0);
    bsgpu_summary s;
    int rc = bsgpu_set_blocks(c, nb, v.data(), off.data(), size.data(), man.data(), cst.data());
    if (rc == BSGPU_OK) rc = bsgpu_set_cameras(c, 1, &g_cam);
    if (rc == BSGPU_OK) rc = bsgpu_add_factors(c, BSGPU_F_REPROJ, n, idx.data(), consts.data(), lk.data(), la.data());
    if (rc == BSGPU_OK) rc = bsgpu_solve(c, options, &s);
    if (rc == BSGPU_OK) rc = bsgpu_get_blocks(c, v.data(), (int64_t)v.size());
    if (rc != BSGPU_OK || !s.is_solution_usable) { status[f] = 2; bsgpu_destroy(c); continue; }
    for (int i = 0; i < 4; ++i) q_out[4 * f + i] = v[i];
    for (int i = 0; i < 3; ++i) p_out[3 * f + i] = v[4 + i];
    if (final_cost) final_cost[f] = s.final_cost;
    if (iterations) iterations[f] = s.num_iterations;
    status[f] = 0;
    const int blk[2] = {1, 0};   // [p, q]
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) {
        double m[9];
        if (bsgpu_covariance(c, blk[a], blk[b], m) != BSGPU_OK) { status[f] = 3; continue; }
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) cov_out[36 * f + 6 * (3 * a + i) + 3 * b + j] = m[3 * i + j];
      }
    bsgpu_destroy(c);
  }
  return BSGPU_OK;
}
#endif

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
  std::mt19937 rng(11);
  std::normal_distribution<double> N(0.0, 1.0);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  // camera z forward / baselink x forward, offset from the baselink
  Mat<4, 4> T_cb = Mat<4, 4>::Identity();
  const double R0[9] = {0, -1, 0, 0, 0, -1, 1, 0, 0};
  for (int i = 0; i < 9; ++i) T_cb(i / 3, i % 3) = R0[i];
  T_cb(0, 3) = 0.05; T_cb(1, 3) = -0.02; T_cb(2, 3) = 0.1;
  g_cam.fx = 458.654; g_cam.fy = 457.296; g_cam.cx = 367.215; g_cam.cy = 248.375;
  for (int i = 0; i < 9; ++i) g_cam.R_cam_baselink[i] = T_cb(i / 3, i % 3);
  for (int i = 0; i < 3; ++i) g_cam.t_cam_baselink[i] = T_cb(i, 3);
  const Mat<4, 4> T_true = bs_models::PoseToTransform(bs_math::quatNormalized({0.9, 0.1, -0.2, 0.3}), {1.0, -2.0, 0.5});
  auto frame = [&](int n) {
    FrameInput f;
    const Mat<4, 4> T_wc = T_true * bs_models::InvertTransform(T_cb);
    for (int i = 0; i < n; ++i) {
      const double z = 2.0 + 10.0 * U(rng), u = 752.0 * U(rng), v = 480.0 * U(rng);
      const double Pc[3] = {(u - g_cam.cx) / g_cam.fx * z, (v - g_cam.cy) / g_cam.fy * z, z};
      Vec3 P;
      for (int r = 0; r < 3; ++r) P[r] = T_wc(r, 0) * Pc[0] + T_wc(r, 1) * Pc[1] + T_wc(r, 2) * Pc[2] + T_wc(r, 3);
      f.points.push_back(P);
      f.pixels.push_back({u + 0.5 * N(rng), v + 0.5 * N(rng)});
    }
    f.T_WORLD_BASELINK_init = T_true * bs_models::PoseToTransform(bs_math::quatFromAngleAxis({0.02, -0.03, 0.01}), {0.1, -0.05, 0.08});
    return f;
  };
  bsgpu_ctx* ctx = bsgpu_create(0);
  CHECK(ctx && bsgpu_set_cameras(ctx, 1, &g_cam) == BSGPU_OK);
  bs_models::FrameLocalizerParams prm;
  prm.truncate_pixels = false;
  prm.image_width = 752; prm.image_height = 480;
  bs_models::FrameLocalizer loc(ctx, 0, T_cb, prm);
  const std::vector<FrameInput> frames = {frame(150), frame(19), frame(60)};
  const auto out = loc.Localize(frames);
  // 0: refined — close to the truth, (x, y, z, r, p, y) covariance, T_CAMERA_WORLD the inverse of T_WORLD_BASELINK T_cam_baselink^-1
  CHECK(out[0].status == 0 && out[0].localized);
  double dp = 0.0;
  for (int i = 0; i < 3; ++i) dp = std::max(dp, std::fabs(out[0].T_WORLD_BASELINK(i, 3) - T_true(i, 3)));
  CHECK(dp < 0.05);
  const Mat<4, 4> I4 = out[0].T_CAMERA_WORLD * out[0].T_WORLD_BASELINK * bs_models::InvertTransform(T_cb);
  CHECK((I4 - Mat<4, 4>::Identity()).norm() < 1e-12);
  CHECK(out[0].covariance.allFinite() && out[0].covariance(0, 0) > 0 && out[0].covariance(5, 5) > 0);
  CHECK(out[0].avg_reprojection >= 0.0 && out[0].avg_reprojection < 2.0);   // (the oracle stand-in reports 0)
  // position block first: a position variance is larger than an attitude variance at this geometry (metres vs radians at 2-12 m)
  CHECK(out[0].covariance(0, 0) > out[0].covariance(3, 3));
  const Mat<6, 6> sw = bs_models::SwapRotationTranslation(out[0].covariance);
  CHECK(sw(3, 3) == out[0].covariance(0, 0) && sw(0, 4) == out[0].covariance(3, 1));
  CHECK((bs_models::SwapRotationTranslation(sw) - out[0].covariance).norm() == 0.0);
  // 1: below required_points_to_refine — the initial pose and invalid_localization_covariance_weight * I
  CHECK(out[1].status == 1 && !out[1].localized);
  CHECK((out[1].T_WORLD_BASELINK - frames[1].T_WORLD_BASELINK_init).norm() == 0.0);
  CHECK((out[1].covariance - 0.1 * Mat<6, 6>::Identity()).norm() == 0.0);
  CHECK(out[2].status == 0 && out[2].localized);
  // a validator that refuses: the fallback again, and it was handed T_init_refined, the covariance and the average
  int seen = 0;
  const auto rej = loc.Localize({frames[2]}, [&](const Mat<4, 4>& T_ir, const Mat<6, 6>& c, double avg) {
    ++seen;
    CHECK((T_ir - bs_models::InvertTransform(frames[2].T_WORLD_BASELINK_init) * out[2].T_WORLD_BASELINK).norm() < 1e-12);
    CHECK((c - out[2].covariance).norm() == 0.0 && avg == out[2].avg_reprojection);
    return false;
  });
  CHECK(seen == 1 && rej[0].status == 0 && !rej[0].localized);
  CHECK((rej[0].T_WORLD_BASELINK - frames[2].T_WORLD_BASELINK_init).norm() == 0.0);
  CHECK((rej[0].covariance - 0.1 * Mat<6, 6>::Identity()).norm() == 0.0);
  std::printf("POSE %.17g %.17g %.17g\n", out[0].T_WORLD_BASELINK(0, 3), out[0].T_WORLD_BASELINK(1, 3), out[0].T_WORLD_BASELINK(2, 3));
  for (int i = 0; i < 36; ++i) std::printf("COV %d %.17g\n", i, out[0].covariance.a[i]);
  bsgpu_destroy(ctx);
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("HOST FRAME LOCALIZER DONE\n");
  return 0;
}
