// Driver of beam_slam_amd/csrc/point_grid.h's summation template on the CPU for tests/test_point_grid.py: reads commands from a binary
// file of doubles (integers as doubles too) and prints what the header computes.
//   <n> <rec: 17 or 28> <terms: rec per point>
//       -> SUM <command> <rec sums>                                                                 grid_chunked_sums<rec>
#include <cstdio>
#include <vector>

#include "point_grid.h"

template <int REC>
static void sums(int n, const std::vector<double>& terms, int count) {
  double sum[REC];
  bsg::grid_chunked_sums<REC>(n, [&](int i, double* r) { for (int t = 0; t < REC; ++t) r[t] = terms[(size_t)i * REC + t]; }, sum);
  std::printf("SUM %d", count);
  for (double v : sum) std::printf(" %.17g", v);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  int count = 0;
  double h[2];
  while (rd(h, 1)) {
    if (!rd(h + 1, 1) || h[0] < 0 || (h[1] != 17.0 && h[1] != 28.0)) return 3;
    const int n = (int)h[0], rec = (int)h[1];
    std::vector<double> terms((size_t)n * rec);
    if (!rd(terms.data(), terms.size())) return 3;
    if (rec == 17) sums<17>(n, terms, count); else sums<28>(n, terms, count);
    ++count;
  }
  std::fclose(f);
  std::printf("DONE %d\n", count);
  return 0;
}
