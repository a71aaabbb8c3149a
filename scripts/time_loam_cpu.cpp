// CPU context for scripts/time_register_loam.py: wall time of loam.h's serial loop (loam_register_serial: both grids, the
// correspondences and the Levenberg-Marquardt iterations, pair after pair) on one core.  Input: <reps> then a binary file of doubles
// holding the pairs in the format of tests/plan/test_loam.cpp's command 1.  Output: reps lines MS <milliseconds for all pairs>, then
// ITERS <outer/inner per pair> and STATUS <per pair>.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "loam.h"

struct Pair { std::vector<double> c[4], Ti; bsg::LoamParams P; double grid_cell, max_cells; };

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int reps = std::atoi(argv[1]);
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  std::vector<Pair> pairs;
  double kind;
  while (rd(&kind, 1)) {
    double h[18];
    if (kind != 1.0 || !rd(h, 18)) return 3;
    Pair p;
    for (int k = 0; k < 4; ++k) {
      if (h[k] < 0) return 3;
      p.c[k].resize(3 * (size_t)h[k]);
      if (!rd(p.c[k].data(), p.c[k].size())) return 3;
    }
    p.Ti.resize(h[4] != 0.0 ? 12 : 0);
    if (!rd(p.Ti.data(), p.Ti.size())) return 3;
    std::memset(&p.P, 0, sizeof(p.P));
    p.P.mc2 = h[5] * h[5]; p.P.min_measurements = (int)h[6]; p.P.max_outer = (int)h[7];
    p.P.conv_translation = h[8]; p.P.cos_rotation = bsg::loam_cos_bound(h[9]);
    p.P.loss_kind = (int)h[10]; p.P.loss_a = h[11];
    p.P.inner.jacobi_scaling = 1; p.P.inner.max_num_consecutive_invalid_steps = 5;
    p.P.inner.initial_trust_region_radius = 1e4; p.P.inner.max_trust_region_radius = 1e16; p.P.inner.min_trust_region_radius = 1e-32;
    p.P.inner.min_relative_decrease = 1e-3; p.P.inner.min_lm_diagonal = 1e-6; p.P.inner.max_lm_diagonal = 1e32;
    p.P.inner.max_num_iterations = (int)h[14]; p.P.inner.function_tolerance = h[15]; p.P.inner.gradient_tolerance = h[16];
    p.P.inner.parameter_tolerance = h[17];
    p.grid_cell = h[12]; p.max_cells = h[13];
    pairs.push_back(p);
  }
  std::fclose(f);
  std::vector<bsg::LoamResult> res(pairs.size());
  for (int r = 0; r < reps + 1; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t k = 0; k < pairs.size(); ++k) {
      const Pair& p = pairs[k];
      double T[12], Trt[12];
      if (!bsg::loam_register_serial((int)(p.c[0].size() / 3), p.c[0].data(), (int)(p.c[1].size() / 3), p.c[1].data(), (int)(p.c[2].size() / 3),
                                     p.c[2].data(), (int)(p.c[3].size() / 3), p.c[3].data(), p.Ti.empty() ? nullptr : p.Ti.data(), p.P, p.grid_cell,
                                     p.max_cells, T, Trt, &res[k]))
        return 5;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r > 0) std::printf("MS %.6f\n", ms);
  }
  std::printf("ITERS");
  for (const bsg::LoamResult& r : res) std::printf(" %d/%d", r.n_iters, r.n_inner);
  std::printf("\nSTATUS");
  for (const bsg::LoamResult& r : res) std::printf(" %d", r.status);
  std::printf("\n");
  return 0;
}
