// CPU context for scripts/time_extract_loam.py: wall time of loam_features.h's serial loop (loam_extract_serial: rings, unreliable marks,
// curvature and the picks, scan after scan) on one core.  Input: <reps> then a binary file of doubles holding the scans in the format of
// tests/plan/test_loam_features.cpp's command 1.  Output: reps lines MS <milliseconds for all scans>, then COUNTS <SHARP/LESS_SHARP/FLAT/
// LESS_FLAT per scan>.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "loam_features.h"

struct Scan { std::vector<double> pts, bound; std::vector<int32_t> ring; bool has_ring; bsg::LoamFeatParams P; };

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int reps = std::atoi(argv[1]);
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  std::vector<Scan> scans;
  double kind;
  while (rd(&kind, 1)) {
    double h[11];
    if (kind != 1.0 || !rd(h, 11) || h[0] < 0 || h[2] < 1 || h[2] > bsg::kLoamMaxRings) return 3;
    Scan s;
    s.pts.resize(3 * (size_t)h[0]);
    s.has_ring = h[1] != 0.0;
    std::vector<double> ringd(s.has_ring ? (size_t)h[0] : 0);
    if (!rd(s.pts.data(), s.pts.size()) || !rd(ringd.data(), ringd.size())) return 3;
    for (double r : ringd) s.ring.push_back((int32_t)r);
    s.P.beams = (int)h[2]; s.P.axis = (int)h[4]; s.P.regions = (int)h[5]; s.P.c = (int)h[6];
    s.P.max_sharp = (int)h[7]; s.P.max_less_sharp = (int)h[8]; s.P.max_flat = (int)h[9]; s.P.threshold = h[10];
    s.bound.resize((size_t)s.P.beams + 1);
    bsg::loam_feat_bounds(s.P.beams, h[3], s.bound.data());
    scans.push_back(s);
  }
  std::fclose(f);
  std::vector<bsg::LoamFeatures> res(scans.size());
  for (int r = 0; r < reps + 1; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t k = 0; k < scans.size(); ++k) {
      const Scan& s = scans[k];
      if (!bsg::loam_extract_serial((int)(s.pts.size() / 3), s.pts.data(), s.has_ring ? s.ring.data() : nullptr, s.P, s.bound.data(), &res[k])) return 5;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r > 0) std::printf("MS %.6f\n", ms);
  }
  std::printf("COUNTS");
  for (const bsg::LoamFeatures& r : res) std::printf(" %zu/%zu/%zu/%zu", r.sharp.size(), r.less_sharp.size(), r.flat.size(), r.less_flat.size());
  std::printf("\n");
  return 0;
}
