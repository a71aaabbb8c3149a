// CPU context for scripts/time_essential_ransac.py: wall time of five_point.h's serial loop (fpr_ransac_serial) on one core.
// Input file: "<n_sets> <prob> <threshold_px> <max_iters> <seed> <reps>", then per set "<n> <fx fy cx cy>" and n lines "<u1 v1 u2 v2>".
// Output: one line per repetition, "MS <milliseconds for all sets>", then "ITERS <n_iters of every set>".
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "five_point.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_sets, max_iters, reps;
  double prob, thr;
  uint64_t seed;
  if (std::fscanf(f, "%d %lf %lf %d %" SCNu64 " %d", &n_sets, &prob, &thr, &max_iters, &seed, &reps) != 6) return 3;
  struct Set { int n; double K[4]; std::vector<double> p1, p2; };
  std::vector<Set> sets(n_sets);
  for (Set& s : sets) {
    if (std::fscanf(f, "%d %lf %lf %lf %lf", &s.n, s.K, s.K + 1, s.K + 2, s.K + 3) != 5) return 3;
    s.p1.resize(2 * s.n); s.p2.resize(2 * s.n);
    for (int i = 0; i < s.n; ++i)
      if (std::fscanf(f, "%lf %lf %lf %lf", &s.p1[2 * i], &s.p1[2 * i + 1], &s.p2[2 * i], &s.p2[2 * i + 1]) != 4) return 3;
  }
  std::fclose(f);
  std::vector<int> iters(n_sets);
  for (int r = 0; r <= reps; ++r) {   // (repetition 0 warms the caches and is not reported)
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < n_sets; ++k) {
      Set& s = sets[k];
      std::vector<double> xn(4 * (size_t)s.n + 4);
      std::vector<uint8_t> mask(s.n + 1);
      double E[9];
      int ni, bs[5], st;
      bsg::fpr_ransac_serial(s.n, s.p1.data(), s.p2.data(), s.K, prob, thr, max_iters, seed, (uint64_t)k, xn.data(), mask.data(), E, &ni,
                             &iters[k], bs, &st);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r > 0) std::printf("MS %.6f\n", ms);
  }
  std::printf("ITERS");
  for (int v : iters) std::printf(" %d", v);
  std::printf("\n");
  return 0;
}
