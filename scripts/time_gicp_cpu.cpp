// CPU context for scripts/time_register_gicp.py: wall time of gicp.h's serial loop (gicp_register_serial: both grids, the covariances
// and the iterations, pair after pair) on one core.  Input: <reps> then a binary file of doubles holding the pairs in the format of
// tests/plan/test_gicp.cpp's command 1.  Output: reps lines MS <milliseconds for all pairs>, then ITERS <outer/inner per pair> and
// STATUS <per pair>.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gicp.h"

struct Pair { std::vector<double> S, Q, Ti; bsg::GicpParams P; double grid_cell, max_cells; };

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int reps = std::atoi(argv[1]);
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  std::vector<Pair> pairs;
  double kind;
  while (rd(&kind, 1)) {
    double h[14];
    if (kind != 1.0 || !rd(h, 14) || h[0] < 0 || h[1] < 0) return 3;
    Pair p;
    p.S.resize(3 * (size_t)h[0]); p.Q.resize(3 * (size_t)h[1]); p.Ti.resize(h[2] != 0.0 ? 12 : 0);
    if (!rd(p.S.data(), p.S.size()) || !rd(p.Q.data(), p.Q.size()) || !rd(p.Ti.data(), p.Ti.size())) return 3;
    p.P = bsg::GicpParams{(int)h[3], h[4], h[5], (int)h[6], h[7], h[8], (int)h[9], h[10]};
    p.grid_cell = h[11]; p.max_cells = h[12];
    pairs.push_back(p);
  }
  std::fclose(f);
  std::vector<int> iters(pairs.size()), inner(pairs.size()), status(pairs.size());
  for (int r = 0; r < reps + 1; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t k = 0; k < pairs.size(); ++k) {
      const Pair& p = pairs[k];
      double T[12], Trt[12], cost;
      int n_corr;
      if (!bsg::gicp_register_serial((int)(p.S.size() / 3), p.S.data(), (int)(p.Q.size() / 3), p.Q.data(), p.Ti.empty() ? nullptr : p.Ti.data(), p.P,
                                     p.grid_cell, p.max_cells, T, Trt, &cost, &n_corr, &iters[k], &inner[k], &status[k], nullptr, nullptr))
        return 5;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r > 0) std::printf("MS %.6f\n", ms);
  }
  std::printf("ITERS");
  for (size_t k = 0; k < pairs.size(); ++k) std::printf(" %d/%d", iters[k], inner[k]);
  std::printf("\nSTATUS");
  for (int v : status) std::printf(" %d", v);
  std::printf("\n");
  return 0;
}
