// Driver of beam_slam_amd/csrc/registration_map.h on the CPU for tests/test_registration_map.py: reads commands from a binary file of
// doubles (integers as doubles too) and prints what the header computes.  Every array has its exact size, so that a sanitizer sees any
// access past one.
//   1 <n_maps> <n_scans> <n_points> <has_T> <voxel_size> <map_scan_start: n_maps + 1> <scan_start: n_scans + 1> <points: 3 n_points>
//     <T: 12 n_scans if has_T>
//       -> MAP <command> <ok> <n_out> <map_start: n_maps + 1> <count: n_out> <points: 3 n_out, the bits in hexadecimal>
//          ok 0: a coordinate out of range                                                                   registration_map_serial
#include <cstdio>
#include <cstring>
#include <vector>

#include "registration_map.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  int count = 0;
  double kind;
  while (rd(&kind, 1)) {
    if (kind != 1.0) return 4;
    double h[5];
    if (!rd(h, 5) || h[0] < 0 || h[1] < 0 || h[2] < 0) return 3;
    const size_t n_maps = (size_t)h[0], n_scans = (size_t)h[1], n = (size_t)h[2];
    std::vector<double> msd(n_maps + 1), ssd(n_scans + 1), pts(3 * n), T(h[3] != 0.0 ? 12 * n_scans : 0);
    if (!rd(msd.data(), msd.size()) || !rd(ssd.data(), ssd.size()) || !rd(pts.data(), pts.size()) || !rd(T.data(), T.size())) return 3;
    std::vector<int32_t> ms(msd.begin(), msd.end()), ss(ssd.begin(), ssd.end());
    if (ms[0] != 0 || ss[0] != 0 || (size_t)ms[n_maps] != n_scans || (size_t)ss[n_scans] != n) return 3;
    bsg::RegistrationMaps R;
    const bool ok = bsg::registration_map_serial((int)n_maps, ms.data(), ss.data(), pts.data(), h[3] != 0.0 ? T.data() : nullptr, h[4], &R);
    if (!ok) {
      std::printf("MAP %d 0\n", count);
    } else {
      std::printf("MAP %d 1 %zu", count, R.count.size());
      for (int32_t s : R.start) std::printf(" %d", s);
      for (int32_t c : R.count) std::printf(" %d", c);
      for (double x : R.points) {
        unsigned long long bits;
        std::memcpy(&bits, &x, 8);
        std::printf(" %016llx", bits);
      }
      std::printf("\n");
    }
    ++count;
  }
  std::fclose(f);
  std::printf("DONE %d\n", count);
  return 0;
}
