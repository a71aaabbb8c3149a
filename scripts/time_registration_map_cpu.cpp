// CPU context for scripts/time_registration_map.py: wall time of registration_map.h's serial contract (registration_map_serial: the
// transform, the keys, std::stable_sort, the sequential centroids) on one core.  Input: <reps> then a binary file of doubles holding
// one call in the format of tests/plan/test_registration_map.cpp's command 1.  Output: reps lines MS <milliseconds>, then COUNTS <output
// points per map>.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "registration_map.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int reps = std::atoi(argv[1]);
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  double h[6];
  if (!rd(h, 6) || h[0] != 1.0 || h[1] < 0 || h[2] < 0 || h[3] < 0) return 3;
  const size_t n_maps = (size_t)h[1], n_scans = (size_t)h[2], n = (size_t)h[3];
  std::vector<double> msd(n_maps + 1), ssd(n_scans + 1), pts(3 * n), T(h[4] != 0.0 ? 12 * n_scans : 0);
  if (!rd(msd.data(), msd.size()) || !rd(ssd.data(), ssd.size()) || !rd(pts.data(), pts.size()) || !rd(T.data(), T.size())) return 3;
  std::fclose(f);
  std::vector<int32_t> ms(msd.begin(), msd.end()), ss(ssd.begin(), ssd.end());
  bsg::RegistrationMaps R;
  for (int r = 0; r < reps + 1; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!bsg::registration_map_serial((int)n_maps, ms.data(), ss.data(), pts.data(), T.empty() ? nullptr : T.data(), h[5], &R)) return 5;
    const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r > 0) std::printf("MS %.6f\n", t);
  }
  std::printf("COUNTS");
  for (size_t m = 0; m < n_maps; ++m) std::printf(" %d", R.start[m + 1] - R.start[m]);
  std::printf("\n");
  return 0;
}
