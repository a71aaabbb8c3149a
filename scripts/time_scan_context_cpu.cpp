// CPU context for scripts/time_scan_context.py: wall time of scan_context.h's serial loops (sc_describe_serial, then sc_match_serial on
// its descriptors: one set, the first <n_queries> aggregates against the rest) on one core.  Input: <reps> <file> <n_queries> <K>
// <search_ratio> <dist_thres>, the file holding one describe command in the format of tests/plan/test_scan_context.cpp's command 1.
// Output: reps lines MS <describe milliseconds> <match milliseconds>, then BEST <best_cand per query> and KEPT <n_binned of aggregate 0>.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scan_context.h"

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  const int reps = std::atoi(argv[1]), nq = std::atoi(argv[3]), K = std::atoi(argv[4]);
  const double ratio = std::atof(argv[5]), thres = std::atof(argv[6]);
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  auto rdi = [&](std::vector<int32_t>& v) {
    std::vector<double> t(v.size());
    if (!rd(t.data(), t.size())) return false;
    for (size_t i = 0; i < v.size(); ++i) v[i] = (int32_t)t[i];
    return true;
  };
  double h[7];
  if (!rd(h, 7) || h[0] != 1.0 || h[1] < 0 || h[2] < nq || h[3] < 0) return 3;
  const int ns = (int)h[1], na = (int)h[2], nm = (int)h[3];
  std::vector<int32_t> ss((size_t)ns + 1), ms((size_t)na + 1), mscan((size_t)nm);
  if (!rdi(ss)) return 3;
  std::vector<double> pts(3 * (size_t)ss[ns]), T(h[4] != 0.0 ? 12 * (size_t)nm : 0);
  if (!rd(pts.data(), pts.size()) || !rdi(ms) || !rdi(mscan) || !rd(T.data(), T.size())) return 3;
  std::fclose(f);
  std::vector<double> desc((size_t)bsg::kScBins * na), bd((size_t)nq);
  std::vector<int32_t> nb((size_t)na), bc((size_t)nq), bs((size_t)nq);
  const int32_t qs[2] = {0, nq}, cs[2] = {0, na - nq};
  for (int r = 0; r < reps + 1; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    bsg::sc_describe_serial(ss.data(), pts.data(), na, ms.data(), mscan.data(), T.empty() ? nullptr : T.data(), h[5], h[6], desc.data(), nullptr, nullptr,
                            nb.data());
    const auto t1 = std::chrono::steady_clock::now();
    bsg::sc_match_serial(1, qs, desc.data(), cs, desc.data() + (size_t)bsg::kScBins * nq, K, ratio, thres, bc.data(), bd.data(), bs.data(), nullptr,
                         nullptr, nullptr);
    const auto t2 = std::chrono::steady_clock::now();
    if (r > 0)
      std::printf("MS %.6f %.6f\n", std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count());
  }
  std::printf("BEST");
  for (int v : bc) std::printf(" %d", v);
  std::printf("\nKEPT %d\n", na > 0 ? nb[0] : 0);
  return 0;
}
