// CPU context for scripts/time_inertial_alignment.py: wall time of inertial_align.h's serial loop (one lane, path after path) on one
// core.  Input: <n_paths> <n_frames> <n_samples> <bridge_gap> <apply_scale> <reps>, <n_paths + 1 ints: frame_start>, <2 n_paths ints:
// imu_range>, n_frames lines <t q[4] p[3]>, n_samples lines <t w[3] a[3]>.  Output: reps lines MS <milliseconds>, then STATUS <per path>.
#include <chrono>
#include <cstdio>
#include <vector>

#include "inertial_align.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int np, nf, ns, bridge, apply, reps;
  if (std::fscanf(f, "%d %d %d %d %d %d", &np, &nf, &ns, &bridge, &apply, &reps) != 6 || np < 0 || nf < 0 || ns < 0) return 3;
  std::vector<int> fstart(np + 1), range(2 * np);
  for (int& v : fstart) if (std::fscanf(f, "%d", &v) != 1) return 3;
  for (int& v : range) if (std::fscanf(f, "%d", &v) != 1) return 3;
  std::vector<double> tf(nf), qf(4 * nf), pf(3 * nf), t(ns), w(3 * ns), a(3 * ns);
  auto rd = [&](double* v, int n) { for (int i = 0; i < n; ++i) if (std::fscanf(f, "%lf", v + i) != 1) return false; return true; };
  for (int i = 0; i < nf; ++i) if (!rd(&tf[i], 1) || !rd(&qf[4 * i], 4) || !rd(&pf[3 * i], 3)) return 3;
  for (int i = 0; i < ns; ++i) if (!rd(&t[i], 1) || !rd(&w[3 * i], 3) || !rd(&a[3 * i], 3)) return 3;
  std::fclose(f);
  if (fstart[0] != 0 || fstart[np] != nf) return 3;
  for (int k = 0; k < np; ++k) if (fstart[k + 1] < fstart[k] || range[2 * k] < 0 || range[2 * k + 1] < range[2 * k] || range[2 * k + 1] > ns) return 3;
  std::vector<double> grav(3 * np), bg(3 * np), scale(np), exc(np), vel(3 * nf), qo(4 * nf), po(3 * nf), vo(3 * nf);
  std::vector<int> rank(np), status(np), own(nf + np);
  std::vector<double> fs((size_t)nf * bsg::kAlignFrameScratch), ps((size_t)np * bsg::kAlignPathScratch);
  double ws[bsg::kAlignWork];
  for (int r = 0; r < reps + 1; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < np; ++k)
      bsg::align_path_of_call(k, fstart.data(), tf.data(), qf.data(), pf.data(), range.data(), t.data(), w.data(), a.data(), bridge, 0.25, apply,
                              0.02, 1.0, 1e-10, grav.data(), bg.data(), scale.data(), exc.data(), rank.data(), vel.data(), qo.data(), po.data(),
                              vo.data(), status.data(), own.data(), fs.data(), ps.data(), ws, 0, 1, bsg::AlignSerial{});
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r > 0) std::printf("MS %.6f\n", ms);
  }
  std::printf("STATUS");
  for (int k = 0; k < np; ++k) std::printf(" %d", status[k]);
  std::printf("\n");
  return 0;
}
