// Driver of beam_slam_amd/csrc/loam.h on the CPU for tests/test_loam.py: reads commands from a binary file of doubles (integers as
// doubles too) and prints what the header computes.  Every array has its exact size, so that a sanitizer sees any access past one.
//   1 <n_ref_edge> <n_ref_surf> <n_tgt_edge> <n_tgt_surf> <has_init> <max_corr> <min_measurements> <max_outer> <conv_translation_m>
//     <conv_rotation_deg> <loss_kind> <loss_a> <grid_cell> <max_cells> <max_num_iterations> <function_tolerance> <gradient_tolerance>
//     <parameter_tolerance> <ref edges> <ref surfaces> <tgt edges> <tgt surfaces> <T_init: 12 if has_init>
//       -> REG <command> <ok> <status> <n_iters> <n_inner> <n_edge> <n_surf> <cost> <T_refest_ref[12]> <T_ref_tgt[12]> <cov[36]>
//                                                                                                   loam_register_serial
//   2 <k: 2 edge rule, 3 surface rule> <n_ref> <n_query> <h> <max_corr> <ref> <queries>
//       -> NN <command> <per query: kept, then the k neighbour indices (-1: the cloud has no such point)>
//                                                                                                   grid_build_serial, grid_knn, loam_keep_*
#include <cstdio>
#include <cstring>
#include <vector>

#include "loam.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  int count = 0;
  double kind;
  while (rd(&kind, 1)) {
    if (kind == 1.0) {
      double h[18];
      if (!rd(h, 18) || h[0] < 0 || h[1] < 0 || h[2] < 0 || h[3] < 0) return 3;
      const int n[4] = {(int)h[0], (int)h[1], (int)h[2], (int)h[3]};
      std::vector<double> c[4], Ti(h[4] != 0.0 ? 12 : 0);
      for (int k = 0; k < 4; ++k) {
        c[k].resize(3 * (size_t)n[k]);
        if (!rd(c[k].data(), c[k].size())) return 3;
      }
      if (!rd(Ti.data(), Ti.size())) return 3;
      bsg::LoamParams P;
      std::memset(&P, 0, sizeof(P));
      P.mc2 = h[5] * h[5]; P.min_measurements = (int)h[6]; P.max_outer = (int)h[7];
      P.conv_translation = h[8]; P.cos_rotation = bsg::loam_cos_bound(h[9]);
      P.loss_kind = (int)h[10]; P.loss_a = h[11];
      // Ceres' defaults (bsgpu_options_default) under the four fields of the command
      P.inner.jacobi_scaling = 1; P.inner.max_num_consecutive_invalid_steps = 5;
      P.inner.initial_trust_region_radius = 1e4; P.inner.max_trust_region_radius = 1e16; P.inner.min_trust_region_radius = 1e-32;
      P.inner.min_relative_decrease = 1e-3; P.inner.min_lm_diagonal = 1e-6; P.inner.max_lm_diagonal = 1e32;
      P.inner.max_num_iterations = (int)h[14]; P.inner.function_tolerance = h[15]; P.inner.gradient_tolerance = h[16];
      P.inner.parameter_tolerance = h[17];
      std::vector<double> T(12), Trt(12);
      bsg::LoamResult res;
      std::memset(&res, 0, sizeof(res));
      const bool ok = bsg::loam_register_serial(n[0], c[0].data(), n[1], c[1].data(), n[2], c[2].data(), n[3], c[3].data(),
                                                Ti.empty() ? nullptr : Ti.data(), P, h[12], h[13], T.data(), Trt.data(), &res);
      std::printf("REG %d %d %d %d %d %d %d %.17g", count, ok ? 1 : 0, res.status, res.n_iters, res.n_inner, res.n_edge, res.n_surf, res.cost);
      for (double v : T) std::printf(" %.17g", ok ? v : 0.0);
      for (double v : Trt) std::printf(" %.17g", ok ? v : 0.0);
      for (int i = 0; i < 36; ++i) std::printf(" %.17g", ok ? res.cov[i] : 0.0);
      std::printf("\n");
    } else if (kind == 2.0) {
      double h[5];
      if (!rd(h, 5) || (h[0] != 2.0 && h[0] != 3.0) || h[1] < 0 || h[2] < 0) return 3;
      const int k = (int)h[0], nr = (int)h[1], nq = (int)h[2];
      std::vector<double> R(3 * (size_t)nr), Q(3 * (size_t)nq), ld((size_t)k), li((size_t)k);
      if (!rd(R.data(), R.size()) || !rd(Q.data(), Q.size())) return 3;
      bsg::SerialGrid G;
      if (!bsg::grid_build_serial(nr, R.data(), h[3], 1e9, &G)) return 5;
      std::printf("NN %d", count);
      for (int i = 0; i < nq; ++i) {
        int corr[3] = {-1, -1, -1};
        bsg::grid_knn(G.g, G.cell_end.data(), G.rec.data(), &Q[3 * (size_t)i], k, ld.data(), li.data(), 1);
        const bool kept = k == 2 ? bsg::loam_keep_edge(R.data(), ld.data(), li.data(), 1, h[4] * h[4], corr)
                                 : bsg::loam_keep_surface(R.data(), ld.data(), li.data(), 1, h[4] * h[4], corr);
        std::printf(" %d", kept ? 1 : 0);
        for (int j = 0; j < k; ++j) std::printf(" %d", std::isfinite(li[j]) ? (int)li[j] : -1);
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
