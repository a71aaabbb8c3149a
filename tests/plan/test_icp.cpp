// Driver of beam_slam_amd/csrc/icp.h on the CPU for tests/test_icp.py: reads commands from a binary file of doubles (integers as
// doubles too) and prints what the header computes.  Every array has its exact size, so that a sanitizer sees any access past one.
//   1 <n_src> <n_tgt> <has_init> <max_corr> <max_iter> <t_eps> <fit_eps> <rotation_threshold> <rel_mse_eps> <max_cells>
//     <S: 3 n_src> <Q: 3 n_tgt> <T_init: 12 if has_init>
//       -> REG <command> <ok> <status> <n_iters> <n_corr> <mse> <T[12]> <T_ref_tgt[12]>           icp_register_serial
//   2 <n_src> <n_tgt> <h> <S> <Q>
//       -> NN <command> <n_src indices, -1: none within h>                                         icp_grid_build_serial, icp_nearest
#include <cstdio>
#include <vector>

#include "icp.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  int count = 0;
  double kind;
  while (rd(&kind, 1)) {
    if (kind == 1.0) {
      double h[10];
      if (!rd(h, 10) || h[0] < 0 || h[1] < 0) return 3;
      const int ns = (int)h[0], nt = (int)h[1];
      std::vector<double> S(3 * (size_t)ns), Q(3 * (size_t)nt), Ti(h[2] != 0.0 ? 12 : 0);
      if (!rd(S.data(), S.size()) || !rd(Q.data(), Q.size()) || !rd(Ti.data(), Ti.size())) return 3;
      const bsg::IcpParams P{(int)h[4], h[5], h[6], h[7], h[8]};
      std::vector<double> T(12), Trt(12);
      double mse = 0.0;
      int n_corr = 0, n_iters = 0, status = 0;
      const bool ok = bsg::icp_register_serial(ns, S.data(), nt, Q.data(), Ti.empty() ? nullptr : Ti.data(), h[3], P, h[9], T.data(), Trt.data(),
                                               &mse, &n_corr, &n_iters, &status);
      std::printf("REG %d %d %d %d %d %.17g", count, ok ? 1 : 0, status, n_iters, n_corr, mse);
      for (double v : T) std::printf(" %.17g", ok ? v : 0.0);
      for (double v : Trt) std::printf(" %.17g", ok ? v : 0.0);
      std::printf("\n");
    } else if (kind == 2.0) {
      double h[3];
      if (!rd(h, 3) || h[0] < 0 || h[1] < 0) return 3;
      const int ns = (int)h[0], nt = (int)h[1];
      std::vector<double> S(3 * (size_t)ns), Q(3 * (size_t)nt);
      if (!rd(S.data(), S.size()) || !rd(Q.data(), Q.size())) return 3;
      bsg::IcpSerialGrid G;
      if (!bsg::icp_grid_build_serial(nt, Q.data(), h[2], 1e9, &G)) return 5;
      std::printf("NN %d", count);
      for (int i = 0; i < ns; ++i) {
        double d2, q[3], idx;
        const bool kept = bsg::icp_nearest(G.g, G.cell_end.data(), G.rec.data(), &S[3 * (size_t)i], h[2] * h[2], &d2, q, &idx);
        std::printf(" %d", kept ? (int)idx : -1);
      }
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
