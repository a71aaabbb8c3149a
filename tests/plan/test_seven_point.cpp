// Driver of beam_slam_amd/csrc/seven_point.h on the CPU for tests/test_seven_point.py: reads commands from a file and prints what the
// header computes.
//   SOLVE  <28 doubles: 7 x (x_first y_first x_last y_last), normalised>   -> SOL <case> <nsol>, then per solution E <case> <9 doubles>
//                                                                             and four times T <case> <12 doubles>
//   SAMPLE <seed> <set> <sample> <n>                                       -> IDX <case> <7 ints>
//   RANSAC <n> <prob> <threshold_px> <max_iters> <seed> <set> <truncate> <validate_px> <min_ratio> <fx fy cx cy>, followed by n lines
//          <u_first v_first u_last v_last>
//          -> RES <case> <status> <n_inliers> <n_iters> <pair_valid> <7 ints>, RATIO <case> <double>, TBEST <case> <12 doubles>,
//             MASK <case> <n 0/1 digits>, VALID <case> <n 0/1 digits>, PTS <case> <3 n doubles>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "seven_point.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char cmd[16];
  int count = 0;
  while (std::fscanf(f, "%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "SOLVE")) {
      double m[28], E[9 * bsg::kSp7MaxSol], T[12 * bsg::kSp7MaxHyp];
      for (double& v : m) if (std::fscanf(f, "%lf", &v) != 1) return 3;
      const int ns = bsg::sp7_solve(m, E, T);
      std::printf("SOL %d %d\n", count, ns);
      for (int k = 0; k < ns; ++k) {
        std::printf("E %d", count);
        for (int e = 0; e < 9; ++e) std::printf(" %.17g", E[9 * k + e]);
        std::printf("\n");
        for (int d = 0; d < 4; ++d) {
          std::printf("T %d", count);
          for (int e = 0; e < 12; ++e) std::printf(" %.17g", T[12 * (4 * k + d) + e]);
          std::printf("\n");
        }
      }
    } else if (!std::strcmp(cmd, "SAMPLE")) {
      uint64_t seed, set, s;
      int n, idx[7];
      if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %d", &seed, &set, &s, &n) != 4) return 3;
      bsg::sp7_sample(seed, set, s, n, idx);
      std::printf("IDX %d", count);
      for (int v : idx) std::printf(" %d", v);
      std::printf("\n");
    } else if (!std::strcmp(cmd, "RANSAC")) {
      int n, max_iters, truncate;
      double prob, thr, val, ratio_min, K[4];
      uint64_t seed, set;
      if (std::fscanf(f, "%d %lf %lf %d %" SCNu64 " %" SCNu64 " %d %lf %lf %lf %lf %lf %lf", &n, &prob, &thr, &max_iters, &seed, &set,
                      &truncate, &val, &ratio_min, K, K + 1, K + 2, K + 3) != 13) return 3;
      std::vector<double> p0(2 * (size_t)n + 2), p1(2 * (size_t)n + 2), pts(3 * (size_t)n + 3);
      for (int i = 0; i < n; ++i)
        if (std::fscanf(f, "%lf %lf %lf %lf", &p0[2 * i], &p0[2 * i + 1], &p1[2 * i], &p1[2 * i + 1]) != 4) return 3;
      std::vector<uint8_t> mask(n + 1), valid(n + 1);
      double T[12], ratio;
      int ninl, nit, bs[7], status, pair_valid;
      bsg::sp7_ransac_serial(n, p0.data(), p1.data(), K, prob, thr, max_iters, seed, set, truncate, val, ratio_min, mask.data(), T,
                             pts.data(), valid.data(), &ratio, &pair_valid, &ninl, &nit, bs, &status);
      std::printf("RES %d %d %d %d %d", count, status, ninl, nit, pair_valid);
      for (int v : bs) std::printf(" %d", v);
      std::printf("\nRATIO %d %.17g\nTBEST %d", count, ratio, count);
      for (double v : T) std::printf(" %.17g", v);
      std::printf("\nMASK %d ", count);
      for (int i = 0; i < n; ++i) std::printf("%d", (int)mask[i]);
      std::printf("\nVALID %d ", count);
      for (int i = 0; i < n; ++i) std::printf("%d", (int)valid[i]);
      std::printf("\nPTS %d", count);
      for (int i = 0; i < 3 * n; ++i) std::printf(" %.17g", pts[i]);
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
