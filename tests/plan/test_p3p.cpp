// Driver of beam_slam_amd/csrc/p3p.h on the CPU for tests/test_p3p.py: reads commands from a file and prints what the header
// computes.
//   SOLVE  <fx fy cx cy> <6 doubles: 3 pixels> <9 doubles: 3 world points>   -> SOL <case> <nsol>, then T <case> <12 doubles> each
//   SAMPLE <seed> <frame> <sample> <n>                                       -> IDX <case> <3 ints>
//   RANSAC <n> <prob> <threshold_px> <max_iters> <seed> <frame> <truncate> <fx fy cx cy>, followed by n lines <u v X Y Z>
//          -> RES <case> <status> <n_inliers> <n_iters> <3 ints>, TBEST <case> <12 doubles>, MASK <case> <n 0/1 digits>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "p3p.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char cmd[16];
  int count = 0;
  while (std::fscanf(f, "%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "SOLVE")) {
      double K[4], px[6], P[9], T[12 * bsg::kP3pMaxSol];
      for (double& v : K) if (std::fscanf(f, "%lf", &v) != 1) return 3;
      for (double& v : px) if (std::fscanf(f, "%lf", &v) != 1) return 3;
      for (double& v : P) if (std::fscanf(f, "%lf", &v) != 1) return 3;
      const int ns = bsg::p3p_solve(px, P, K, T);
      std::printf("SOL %d %d\n", count, ns);
      for (int h = 0; h < ns; ++h) {
        std::printf("T %d", count);
        for (int e = 0; e < 12; ++e) std::printf(" %.17g", T[12 * h + e]);
        std::printf("\n");
      }
    } else if (!std::strcmp(cmd, "SAMPLE")) {
      uint64_t seed, frame, s;
      int n, idx[3];
      if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %d", &seed, &frame, &s, &n) != 4) return 3;
      bsg::p3p_sample(seed, frame, s, n, idx[0], idx[1], idx[2]);
      std::printf("IDX %d %d %d %d\n", count, idx[0], idx[1], idx[2]);
    } else if (!std::strcmp(cmd, "RANSAC")) {
      int n, max_iters, truncate;
      double prob, thr, K[4];
      uint64_t seed, frame;
      if (std::fscanf(f, "%d %lf %lf %d %" SCNu64 " %" SCNu64 " %d %lf %lf %lf %lf", &n, &prob, &thr, &max_iters, &seed, &frame, &truncate, K,
                      K + 1, K + 2, K + 3) != 11) return 3;
      std::vector<double> px(2 * (size_t)n + 2), P(3 * (size_t)n + 3);
      for (int i = 0; i < n; ++i)
        if (std::fscanf(f, "%lf %lf %lf %lf %lf", &px[2 * i], &px[2 * i + 1], &P[3 * i], &P[3 * i + 1], &P[3 * i + 2]) != 5) return 3;
      std::vector<uint8_t> mask(n + 1);
      double T[12];
      int ninl, nit, bs[3], status;
      bsg::p3p_ransac_serial(n, px.data(), P.data(), K, prob, thr, max_iters, seed, frame, truncate, mask.data(), T, &ninl, &nit, bs, &status);
      std::printf("RES %d %d %d %d %d %d %d\n", count, status, ninl, nit, bs[0], bs[1], bs[2]);
      std::printf("TBEST %d", count);
      for (double v : T) std::printf(" %.17g", v);
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
