// CPU context for scripts/time_relative_pose_ransac.py: wall time of seven_point.h's serial loop (sp7_ransac_serial) on one core.
// Input file: "<n_frames> <prob> <threshold_px> <max_iters> <seed> <reps>", then per set "<n> <fx fy cx cy>" and n lines "<u_first v_first u_last v_last>".
// Output: one line per repetition, "MS <milliseconds for all frames>", then "ITERS <n_iters of every frame>".
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "seven_point.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_frames, max_iters, reps;
  double prob, thr;
  uint64_t seed;
  if (std::fscanf(f, "%d %lf %lf %d %" SCNu64 " %d", &n_frames, &prob, &thr, &max_iters, &seed, &reps) != 6) return 3;
  struct Frame { int n; double K[4]; std::vector<double> p0, p1; };
  std::vector<Frame> frames(n_frames);
  for (Frame& s : frames) {
    if (std::fscanf(f, "%d %lf %lf %lf %lf", &s.n, s.K, s.K + 1, s.K + 2, s.K + 3) != 5) return 3;
    s.p0.resize(2 * s.n); s.p1.resize(2 * s.n);
    for (int i = 0; i < s.n; ++i)
      if (std::fscanf(f, "%lf %lf %lf %lf", &s.p0[2 * i], &s.p0[2 * i + 1], &s.p1[2 * i], &s.p1[2 * i + 1]) != 4) return 3;
  }
  std::fclose(f);
  std::vector<int> iters(n_frames);
  for (int r = 0; r <= reps; ++r) {   // (repetition 0 warms the caches and is not reported)
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < n_frames; ++k) {
      Frame& s = frames[k];
      std::vector<uint8_t> mask(s.n + 1), valid(s.n + 1);
      std::vector<double> pts(3 * (size_t)s.n + 3);
      double T[12], ratio;
      int ni, bs[7], st, pv;
      bsg::sp7_ransac_serial(s.n, s.p0.data(), s.p1.data(), s.K, prob, thr, max_iters, seed, (uint64_t)k, 0, 10.0, 0.8, mask.data(), T,
                             pts.data(), valid.data(), &ratio, &pv, &ni, &iters[k], bs, &st);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r > 0) std::printf("MS %.6f\n", ms);
  }
  std::printf("ITERS");
  for (int v : iters) std::printf(" %d", v);
  std::printf("\n");
  return 0;
}
