// Driver of beam_slam_amd/csrc/scan_context.h on the CPU for tests/test_scan_context.py: reads commands from a binary file of doubles
// (integers as doubles too) and prints what the header computes.  Every array has its exact size, so that a sanitizer sees any access
// past one.
//   1 <n_scans> <n_aggregates> <n_members> <has_T> <lidar_height> <max_radius> <scan_start: n_scans + 1> <points: 3 per point>
//     <member_start: n_aggregates + 1> <member_scan: n_members> <member_T: 12 n_members if has_T>
//       -> DESC <command> <n_binned: A> <desc: 1200 A> <ring_key: 20 A> <sector_key: 60 A>             sc_describe_serial
//   2 <n_sets> <K> <search_ratio> <dist_thres> <query_start: n_sets + 1> <cand_start: n_sets + 1> <query_desc> <cand_desc>
//       -> MATCH <command> <Q> <P> <best_cand: Q> <best_dist: Q> <best_shift: Q> <yaw: Q> <dist_all: P> <shift_all: P>   sc_match_serial
//   3 <n> <max_radius> <xy: 2 n>
//       -> BIN <command> <n bins, ring * 60 + sector, -1: dropped>                                     sc_bin
#include <cstdio>
#include <vector>

#include "scan_context.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&](double* v, size_t n) { return n == 0 || std::fread(v, sizeof(double), n, f) == n; };
  auto rdi = [&](std::vector<int32_t>& v) {
    std::vector<double> t(v.size());
    if (!rd(t.data(), t.size())) return false;
    for (size_t i = 0; i < v.size(); ++i) v[i] = (int32_t)t[i];
    return true;
  };
  int count = 0;
  double kind;
  while (rd(&kind, 1)) {
    if (kind == 1.0) {
      double h[6];
      if (!rd(h, 6) || h[0] < 0 || h[1] < 0 || h[2] < 0) return 3;
      const int ns = (int)h[0], na = (int)h[1], nm = (int)h[2];
      std::vector<int32_t> ss((size_t)ns + 1), ms((size_t)na + 1), mscan((size_t)nm);
      if (!rdi(ss)) return 3;
      std::vector<double> pts(3 * (size_t)ss[ns]), T(h[3] != 0.0 ? 12 * (size_t)nm : 0);
      if (!rd(pts.data(), pts.size()) || !rdi(ms) || !rdi(mscan) || !rd(T.data(), T.size())) return 3;
      std::vector<double> desc((size_t)bsg::kScBins * na), rk((size_t)bsg::kScRings * na), sk((size_t)bsg::kScSectors * na);
      std::vector<int32_t> nb((size_t)na);
      bsg::sc_describe_serial(ss.data(), pts.data(), na, ms.data(), mscan.data(), T.empty() ? nullptr : T.data(), h[4], h[5], desc.data(), rk.data(),
                              sk.data(), nb.data());
      std::printf("DESC %d", count);
      for (int v : nb) std::printf(" %d", v);
      for (double v : desc) std::printf(" %.17g", v);
      for (double v : rk) std::printf(" %.17g", v);
      for (double v : sk) std::printf(" %.17g", v);
      std::printf("\n");
    } else if (kind == 2.0) {
      double h[4];
      if (!rd(h, 4) || h[0] < 0) return 3;
      const int n_sets = (int)h[0];
      std::vector<int32_t> qs((size_t)n_sets + 1), cs((size_t)n_sets + 1);
      if (!rdi(qs) || !rdi(cs)) return 3;
      const size_t nq = (size_t)qs[n_sets], nc = (size_t)cs[n_sets];
      std::vector<double> qd(bsg::kScBins * nq), cd(bsg::kScBins * nc);
      if (!rd(qd.data(), qd.size()) || !rd(cd.data(), cd.size())) return 3;
      size_t np = 0;
      for (int s = 0; s < n_sets; ++s) np += (size_t)(qs[s + 1] - qs[s]) * (size_t)(cs[s + 1] - cs[s]);
      std::vector<int32_t> bc(nq), bs(nq), sa(np);
      std::vector<double> bd(nq), yaw(nq), da(np);
      bsg::sc_match_serial(n_sets, qs.data(), qd.data(), cs.data(), cd.data(), (int)h[1], h[2], h[3], bc.data(), bd.data(), bs.data(), yaw.data(),
                           da.data(), sa.data());
      std::printf("MATCH %d %zu %zu", count, nq, np);
      for (int v : bc) std::printf(" %d", v);
      for (double v : bd) std::printf(" %.17g", v);
      for (int v : bs) std::printf(" %d", v);
      for (double v : yaw) std::printf(" %.17g", v);
      for (double v : da) std::printf(" %.17g", v);
      for (int v : sa) std::printf(" %d", v);
      std::printf("\n");
    } else if (kind == 3.0) {
      double h[2];
      if (!rd(h, 2) || h[0] < 0) return 3;
      std::vector<double> xy(2 * (size_t)h[0]);
      if (!rd(xy.data(), xy.size())) return 3;
      std::printf("BIN %d", count);
      for (size_t i = 0; i < xy.size(); i += 2) std::printf(" %d", bsg::sc_bin(xy[i], xy[i + 1], h[1]));
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
