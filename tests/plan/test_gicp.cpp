// Driver of beam_slam_amd/csrc/gicp.h on the CPU for tests/test_gicp.py: reads commands from a binary file of doubles (integers as
// doubles too) and prints what the header computes.  Every array has its exact size, so that a sanitizer sees any access past one.
//   1 <n_src> <n_tgt> <has_init> <k> <gicp_epsilon> <max_corr> <max_iter> <r_eps> <t_eps> <max_inner> <inner_eps> <grid_cell> <max_cells>
//     <want_cov> <S: 3 n_src> <Q: 3 n_tgt> <T_init: 12 if has_init>
//       -> REG <command> <ok> <status> <n_iters> <n_inner> <n_corr> <cost> <T[12]> <T_ref_tgt[12]> [<ref_cov: 6 n_src> <tgt_cov: 6 n_tgt>]
//                                                                                                   gicp_register_serial
//   2 <n> <k> <h> <P: 3 n>
//       -> KNN <command> <n k indices: the k nearest of every point in its own cloud>              icp_grid_build_serial, gicp_knn
//   3 <n_src> <n_tgt> <h> <max_corr> <S> <Q>
//       -> NN <command> <n_src indices, -1: none below max_corr>                                   icp_grid_build_serial, gicp_nearest
#include <cstdio>
#include <vector>

#include "gicp.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  int count = 0;
  double kind;
  while (rd(&kind, 1)) {
    if (kind == 1.0) {
      double h[14];
      if (!rd(h, 14) || h[0] < 0 || h[1] < 0) return 3;
      const int ns = (int)h[0], nt = (int)h[1];
      const bool want_cov = h[13] != 0.0;
      std::vector<double> S(3 * (size_t)ns), Q(3 * (size_t)nt), Ti(h[2] != 0.0 ? 12 : 0);
      if (!rd(S.data(), S.size()) || !rd(Q.data(), Q.size()) || !rd(Ti.data(), Ti.size())) return 3;
      const bsg::GicpParams P{(int)h[3], h[4], h[5], (int)h[6], h[7], h[8], (int)h[9], h[10]};
      std::vector<double> T(12), Trt(12), rc(want_cov ? 6 * (size_t)ns : 0), tc(want_cov ? 6 * (size_t)nt : 0);
      double cost = 0.0;
      int n_corr = 0, n_iters = 0, n_inner = 0, status = 0;
      const bool ok = bsg::gicp_register_serial(ns, S.data(), nt, Q.data(), Ti.empty() ? nullptr : Ti.data(), P, h[11], h[12], T.data(), Trt.data(),
                                                &cost, &n_corr, &n_iters, &n_inner, &status, want_cov ? rc.data() : nullptr,
                                                want_cov ? tc.data() : nullptr);
      std::printf("REG %d %d %d %d %d %d %.17g", count, ok ? 1 : 0, status, n_iters, n_inner, n_corr, cost);
      for (double v : T) std::printf(" %.17g", ok ? v : 0.0);
      for (double v : Trt) std::printf(" %.17g", ok ? v : 0.0);
      for (double v : rc) std::printf(" %.17g", ok ? v : 0.0);
      for (double v : tc) std::printf(" %.17g", ok ? v : 0.0);
      std::printf("\n");
    } else if (kind == 2.0) {
      double h[3];
      if (!rd(h, 3) || h[0] < 0 || h[1] < 1 || h[1] > h[0]) return 3;
      const int n = (int)h[0], k = (int)h[1];
      std::vector<double> P(3 * (size_t)n), ld((size_t)k), li((size_t)k);
      if (!rd(P.data(), P.size())) return 3;
      bsg::IcpSerialGrid G;
      if (!bsg::icp_grid_build_serial(n, P.data(), h[2], 1e9, &G)) return 5;
      std::printf("KNN %d", count);
      for (int i = 0; i < n; ++i) {
        bsg::gicp_knn(G.g, G.cell_end.data(), G.rec.data(), &P[3 * (size_t)i], k, ld.data(), li.data(), 1);
        for (int j = 0; j < k; ++j) std::printf(" %d", (int)li[j]);
      }
      std::printf("\n");
    } else if (kind == 3.0) {
      double h[4];
      if (!rd(h, 4) || h[0] < 0 || h[1] < 0) return 3;
      const int ns = (int)h[0], nt = (int)h[1];
      std::vector<double> S(3 * (size_t)ns), Q(3 * (size_t)nt);
      if (!rd(S.data(), S.size()) || !rd(Q.data(), Q.size())) return 3;
      bsg::IcpSerialGrid G;
      if (!bsg::icp_grid_build_serial(nt, Q.data(), h[2], 1e9, &G)) return 5;
      std::printf("NN %d", count);
      for (int i = 0; i < ns; ++i) {
        double d2, q[3], idx;
        const bool kept = bsg::gicp_nearest(G.g, G.cell_end.data(), G.rec.data(), &S[3 * (size_t)i], h[3] * h[3], &d2, q, &idx);
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
