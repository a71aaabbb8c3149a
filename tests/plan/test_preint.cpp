// Driver of beam_slam_amd/csrc/preint_core.h on the CPU for tests/test_preint_hp.py: reads commands from a file and prints what the
// header computes, one bsgpu_preintegrate call per command.
//   PREINT <n_intervals> <n_samples> <info_weight>, followed by <36 doubles: cov_w cov_a cov_bg cov_ba, 3 x 3 row-major each>,
//          <n_intervals + 1 ints: sample_start>, n_samples lines <t w[3] a[3]>, n_intervals lines <t_end bg[3] ba[3]>
//          -> n_intervals lines OUT <case> <interval> <287 doubles>
#include <cstdio>
#include <cstring>
#include <vector>

#include "preint_core.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char cmd[16];
  int count = 0;
  while (std::fscanf(f, "%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "PREINT")) {
      int n, ns;
      double weight, covs[36];
      if (std::fscanf(f, "%d %d %lf", &n, &ns, &weight) != 3 || n < 0 || ns < 0) return 3;
      for (double& v : covs) if (std::fscanf(f, "%lf", &v) != 1) return 3;
      std::vector<int> start(n + 1);
      for (int& v : start) if (std::fscanf(f, "%d", &v) != 1) return 3;
      std::vector<double> ts(ns + 1), wm(3 * ns + 3), am(3 * ns + 3), te(n + 1), bg(3 * n + 3), ba(3 * n + 3);
      for (int s = 0; s < ns; ++s)
        if (std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf", &ts[s], &wm[3 * s], &wm[3 * s + 1], &wm[3 * s + 2], &am[3 * s], &am[3 * s + 1],
                        &am[3 * s + 2]) != 7) return 3;
      for (int i = 0; i < n; ++i)
        if (std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf", &te[i], &bg[3 * i], &bg[3 * i + 1], &bg[3 * i + 2], &ba[3 * i], &ba[3 * i + 1],
                        &ba[3 * i + 2]) != 7) return 3;
      std::vector<double> out(bsg::kPreintOut);
      for (int i = 0; i < n; ++i) {
        if (start[i] < 0 || start[i + 1] < start[i] || start[i + 1] > ns) return 3;
        bsg::preintegrate_interval(start[i], start[i + 1], ts.data(), wm.data(), am.data(), te[i], &bg[3 * i], &ba[3 * i], covs, weight,
                                   out.data());
        std::printf("OUT %d %d", count, i);
        for (double v : out) std::printf(" %.17g", v);
        std::printf("\n");
      }
    } else {
      return 4;
    }
    ++count;
  }
  std::fclose(f);
  std::printf("DONE %d\n", count);
  return 0;
}
