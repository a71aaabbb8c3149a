// bs_models::KeyframeRansacLocalizer (beam_slam_amd/host/keyframe_ransac_localizer.h): the id intersection, its order, the pixel
// truncation and "no pose" around one bsgpu_absolute_pose_ransac call.  Built twice by tests/test_host_keyframe_localizer.py: against
// libbsgpu.so, and with -DP3P_STANDIN, where the stand-in below answers the C-ABI call frame by frame with p3p.h's serial loop
// (p3p_ransac_serial) and records the pixels it was handed.
#include <cmath>
#include <cstdio>
#include <random>
#include <set>

#include "../../beam_slam_amd/host/keyframe_ransac_localizer.h"

// the camera both builds use: C2's pinhole, baselink x forward / z up -> camera z forward / y down, offset from the baselink
static const double kK[4] = {458.654, 457.296, 367.215, 248.375};
static const double kRcb[9] = {0.0, -1.0, 0.0, 0.0, 0.0, -1.0, 1.0, 0.0, 0.0};
static const double kTcb[3] = {0.05, -0.02, 0.1};

#ifdef P3P_STANDIN
#include "p3p.h"
static std::vector<double> g_seen_pix;
extern "C" int bsgpu_absolute_pose_ransac(bsgpu_ctx*, int32_t n_frames, const int32_t* obs_start, const double* pixels, const double* points,
                                          const int32_t*, double prob, double threshold_px, int32_t max_iters, uint64_t seed,
                                          int32_t truncate_pixels, uint8_t* mask, double* q_out, double* p_out, double* T_cam_world,
                                          int32_t* n_inliers, int32_t* n_iters, int32_t* best_sample, int32_t* status) {
  g_seen_pix.assign(pixels, pixels + 2 * obs_start[n_frames]);
  for (int k = 0; k < n_frames; ++k) {
    const int o0 = obs_start[k], n = obs_start[k + 1] - o0;
    double T[12];
    int ni, it, bs[3];
    bsg::p3p_ransac_serial(n, pixels + 2 * o0, points + 3 * o0, kK, prob, threshold_px, max_iters, seed, (uint64_t)k, truncate_pixels,
                           mask + o0, T, &ni, &it, bs, status + k);
    for (int e = 0; e < 4; ++e) q_out[4 * k + e] = NAN;
    for (int e = 0; e < 3; ++e) p_out[3 * k + e] = NAN;
    if (status[k] == bsg::P3P_OK) bsg::p3p_baselink_pose(T, kRcb, kTcb, q_out + 4 * k, p_out + 3 * k);
    if (T_cam_world) for (int e = 0; e < 12; ++e) T_cam_world[12 * k + e] = T[e];
    if (n_inliers) n_inliers[k] = ni;
    if (n_iters) n_iters[k] = it;
    if (best_sample) for (int j = 0; j < 3; ++j) best_sample[3 * k + j] = bs[j];
  }
  return BSGPU_OK;
}
#endif

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
  std::mt19937 rng(23);
  auto U = [&](double a, double b) { return a + (b - a) * (double)(rng() >> 5) / 134217728.0; };
  // two keyframes: T_WORLD_BASELINK = (yaw, p); P_c = R_cb R_wb^T (P - p) + t_cb
  const double yaw[2] = {0.2, -0.35}, pos[2][3] = {{1.0, 0.5, 0.2}, {2.0, -0.4, 0.1}};
  auto project = [&](int k, const std::array<double, 3>& P, double* uv) {
    const double c = std::cos(yaw[k]), s = std::sin(yaw[k]);
    const double d[3] = {P[0] - pos[k][0], P[1] - pos[k][1], P[2] - pos[k][2]};
    const double b[3] = {c * d[0] + s * d[1], -s * d[0] + c * d[1], d[2]};
    double pc[3];
    for (int i = 0; i < 3; ++i) pc[i] = kRcb[3 * i] * b[0] + kRcb[3 * i + 1] * b[1] + kRcb[3 * i + 2] * b[2] + kTcb[i];
    uv[0] = kK[0] * pc[0] / pc[2] + kK[2]; uv[1] = kK[1] * pc[1] / pc[2] + kK[3];
    return pc[2];
  };
  bs_models::LandmarkPoints landmarks;
  bs_models::KeyframePixels kf[2], few, none;
  std::set<uint64_t> common[2], gross[2];
  for (int i = 0; i < 160; ++i) {
    const uint64_t id = 500 + 3 * (uint64_t)((i * 37) % 160);   // inserted out of order
    const std::array<double, 3> P = {U(6.0, 16.0), U(-5.0, 5.0), U(-2.5, 3.0)};
    if (i % 8 != 5) landmarks[id] = P;                          // an eighth of the tracks has no landmark yet
    for (int k = 0; k < 2; ++k) {
      double uv[2];
      const double z = project(k, P, uv);
      if (!(z > 1.0) || uv[0] < 0 || uv[0] >= 752 || uv[1] < 0 || uv[1] >= 480) continue;
      if (i % 7 == 2 + k) continue;                             // not measured in this keyframe
      kf[k][id] = {uv[0], uv[1]};
      if (i % 8 == 5) continue;
      common[k].insert(id);
      if (i % 4 == k + 2) { kf[k][id] = {std::fmod(uv[0] + 300.0, 752.0), std::fmod(uv[1] + 200.0, 480.0)}; gross[k].insert(id); }   // a mismatch far away
    }
  }
  kf[0][7] = {10.0, 10.0};                                      // an id the landmark map does not know
  int m = 0;
  for (const uint64_t id : common[0]) { if (gross[0].count(id)) continue; if (m++ == 3) break; few[id] = kf[0][id]; }
  bsgpu_ctx* ctx = nullptr;
#ifndef P3P_STANDIN
  ctx = bsgpu_create(0);
  CHECK(ctx != nullptr);
  bsgpu_camera cam;
  cam.fx = kK[0]; cam.fy = kK[1]; cam.cx = kK[2]; cam.cy = kK[3];
  for (int i = 0; i < 9; ++i) cam.R_cam_baselink[i] = kRcb[i];
  for (int i = 0; i < 3; ++i) cam.t_cam_baselink[i] = kTcb[i];
  CHECK(bsgpu_set_cameras(ctx, 1, &cam) == BSGPU_OK);
#endif
  bs_models::KeyframeRansacLocalizerParams prm;
  prm.seed = 11;
  bs_models::KeyframeRansacLocalizer loc(ctx, 0, prm);
  const auto out = loc.Localize(landmarks, {&kf[0], &kf[1], &few, &none});
  CHECK(out.size() == 4);
  for (int k = 0; k < 2; ++k) {
    const bs_models::KeyframePose& r = out[k];
    CHECK(r.status == BSGPU_RANSAC_OK && r.has_pose);
    CHECK(r.ids_in_frame == std::vector<uint64_t>(common[k].begin(), common[k].end()));   // the intersection, ascending
    CHECK(common[k].size() > 60 && gross[k].size() > 10);
    CHECK(r.n_iters == 100);                                    // the fixed loop of the reference's call
    std::set<uint64_t> inl(r.inlier_ids.begin(), r.inlier_ids.end());
    CHECK(inl.size() == r.inlier_ids.size() && (int32_t)inl.size() == r.n_inliers);
    for (const uint64_t id : gross[k]) CHECK(inl.count(id) == 0);
    for (const uint64_t id : r.inlier_ids) CHECK(common[k].count(id) == 1);
    CHECK(r.n_inliers >= (int32_t)(0.9 * (double)(common[k].size() - gross[k].size())));
    // whole pixels, 5 px: the pose is the keyframe's to a few centimetres and a fraction of a degree
    const double c = std::cos(yaw[k]), s = std::sin(yaw[k]);
    CHECK(std::fabs(r.T_WORLD_BASELINK(0, 0) - c) < 0.02 && std::fabs(r.T_WORLD_BASELINK(1, 0) - s) < 0.02);
    CHECK(std::fabs(r.T_WORLD_BASELINK(2, 2) - 1.0) < 0.02 && r.T_WORLD_BASELINK(3, 3) == 1.0);
    for (int i = 0; i < 3; ++i) CHECK(std::fabs(r.T_WORLD_BASELINK(i, 3) - pos[k][i]) < 0.3);
  }
  // three pairs, and none: no pose, nothing invented
  CHECK(out[2].status == BSGPU_RANSAC_TOO_FEW && !out[2].has_pose && out[2].ids_in_frame.size() == 3 && out[2].inlier_ids.empty());
  CHECK(out[3].status == BSGPU_RANSAC_TOO_FEW && !out[3].has_pose && out[3].ids_in_frame.empty() && out[3].n_iters == 0);
  CHECK(out[2].T_WORLD_BASELINK(0, 0) == 1.0 && out[2].T_WORLD_BASELINK(0, 3) == 0.0);
#ifdef P3P_STANDIN
  // what reached the back-end: whole pixels, in id order
  CHECK(g_seen_pix.size() == 2 * (common[0].size() + common[1].size() + 3));
  size_t i = 0;
  for (const uint64_t id : common[0]) {
    CHECK(g_seen_pix[2 * i] == std::trunc(kf[0][id][0]) && g_seen_pix[2 * i + 1] == std::trunc(kf[0][id][1]));
    CHECK(kf[0][id][0] != std::trunc(kf[0][id][0]));
    ++i;
  }
  // without truncation the exact pixels pass, and the noise-free inliers are exactly the ids that are not mismatches
  prm.truncate_pixels = false;
  const auto exact = bs_models::KeyframeRansacLocalizer(ctx, 0, prm).Localize(landmarks, {&kf[0]});
  CHECK(g_seen_pix[0] == kf[0][*common[0].begin()][0]);
  std::set<uint64_t> want;
  for (const uint64_t id : common[0]) if (!gross[0].count(id)) want.insert(id);
  CHECK(std::set<uint64_t>(exact[0].inlier_ids.begin(), exact[0].inlier_ids.end()) == want);
  for (int a = 0; a < 3; ++a) CHECK(std::fabs(exact[0].T_WORLD_BASELINK(a, 3) - pos[0][a]) < 1e-6);
#else
  bsgpu_destroy(ctx);
#endif
  for (int k = 0; k < 2; ++k) {
    std::printf("IDS %d", k);
    for (const uint64_t id : out[k].ids_in_frame) std::printf(" %llu", (unsigned long long)id);
    std::printf("\nINLIERS %d", k);
    for (const uint64_t id : out[k].inlier_ids) std::printf(" %llu", (unsigned long long)id);
    std::printf("\n");
  }
  std::printf("STATUS %d %d %d %d\n", out[0].status, out[1].status, out[2].status, out[3].status);
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("HOST KEYFRAME LOCALIZER DONE\n");
  return 0;
}
