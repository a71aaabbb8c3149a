// beam_slam_amd/csrc/dogleg.h on the CPU (tests/test_dogleg.py compiles and runs this, and compares with tests/dogleg_ref.py): for every
// input line "g2 gn2 ggn jv2 radius" the coefficients of the step, one line "case a b norm norm_is_measured" with 17 significant digits.
#include <cstdio>

#include "dogleg.h"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  bsg::DoglegVecs w;
  double radius = 0.0;
  while (std::fscanf(f, "%lf %lf %lf %lf %lf", &w.g2, &w.gn2, &w.ggn, &w.jv2, &radius) == 5) {
    const bsg::DoglegStep s = bsg::dl_coefficients(w, radius);
    std::printf("%d %.17g %.17g %.17g %d\n", s.kase, s.a, s.b, s.norm, s.norm_is_measured ? 1 : 0);
  }
  std::fclose(f);
  // the strategy's radius / mu updates
  double r = 8.0, mu = 1e-8;
  bsg::dl_step_accepted(0.1, 1.0, &r, &mu);   // rho < 0.25: halved; mu stays at its floor
  std::printf("%.17g %.17g\n", r, mu);
  r = 1.0; mu = 1e-3;
  bsg::dl_step_accepted(0.9, 2.0, &r, &mu);   // rho > 0.75: max(radius, 3 |step'|); mu / 5
  std::printf("%.17g %.17g\n", r, mu);
  bsg::dl_step_rejected(&r);
  bsg::dl_step_invalid(&mu);
  std::printf("%.17g %.17g\n", r, mu);
  mu = 0.1;
  const bool again = bsg::dl_retry(&mu);
  std::printf("%d %.17g\n", again ? 1 : 0, mu);
  return 0;
}
