// Driver of beam_slam_amd/csrc/five_point.h on the CPU for tests/test_five_point.py: reads commands from a file and prints what the
// header computes.
//   SOLVE  <20 doubles: 5 x (x1 y1 x2 y2), normalised>                      -> SOL <case> <nsol>, then E <case> <9 doubles> each
//   SAMPLE <seed> <set> <sample> <n>                                        -> IDX <case> <5 ints>
//   RANSAC <n> <prob> <threshold_px> <max_iters> <seed> <set> <fx fy cx cy> -> RES <case> <status> <n_inliers> <n_iters> <5 ints>,
//          followed by n lines <u1 v1 u2 v2>                                   EBEST <case> <9 doubles>, MASK <case> <n 0/1 digits>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "five_point.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char cmd[16];
  int count = 0;
  while (std::fscanf(f, "%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "SOLVE")) {
      double m[20], E[9 * bsg::kFprMaxSol];
      for (double& v : m) if (std::fscanf(f, "%lf", &v) != 1) return 3;
      const int ns = bsg::fpr_five_point(m, E);
      std::printf("SOL %d %d\n", count, ns);
      for (int h = 0; h < ns; ++h) {
        std::printf("E %d", count);
        for (int e = 0; e < 9; ++e) std::printf(" %.17g", E[9 * h + e]);
        std::printf("\n");
      }
    } else if (!std::strcmp(cmd, "SAMPLE")) {
      uint64_t seed, set, s;
      int n, idx[5];
      if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %d", &seed, &set, &s, &n) != 4) return 3;
      bsg::fpr_sample(seed, set, s, n, idx);
      std::printf("IDX %d %d %d %d %d %d\n", count, idx[0], idx[1], idx[2], idx[3], idx[4]);
    } else if (!std::strcmp(cmd, "RANSAC")) {
      int n, max_iters;
      double prob, thr, K[4];
      uint64_t seed, set;
      if (std::fscanf(f, "%d %lf %lf %d %" SCNu64 " %" SCNu64 " %lf %lf %lf %lf", &n, &prob, &thr, &max_iters, &seed, &set, K, K + 1, K + 2,
                      K + 3) != 10) return 3;
      std::vector<double> p1(2 * n), p2(2 * n), xn(4 * n + 4);
      for (int i = 0; i < n; ++i)
        if (std::fscanf(f, "%lf %lf %lf %lf", &p1[2 * i], &p1[2 * i + 1], &p2[2 * i], &p2[2 * i + 1]) != 4) return 3;
      std::vector<uint8_t> mask(n + 1);
      double E[9];
      int ninl, nit, bs[5], status;
      bsg::fpr_ransac_serial(n, p1.data(), p2.data(), K, prob, thr, max_iters, seed, set, xn.data(), mask.data(), E, &ninl, &nit, bs, &status);
      std::printf("RES %d %d %d %d %d %d %d %d %d\n", count, status, ninl, nit, bs[0], bs[1], bs[2], bs[3], bs[4]);
      std::printf("EBEST %d", count);
      for (double v : E) std::printf(" %.17g", v);
      std::printf("\nMASK %d ", count);
      for (int i = 0; i < n; ++i) std::printf("%d", (int)mask[i]);
      std::printf("\n");
    } else {
      return 4;
    }
    ++count;
  }
  std::fclose(f);
  std::printf("DONE %d\n", count);
  return 0;
}
