// beam_slam_amd/csrc/unicycle_body.h on the CPU: a C entry point over the shared functions, loaded with ctypes by
// tests/test_unicycle_body.py and tests/unicycle_ref.py.  x: the 32 ambient values p1, q1, v1, w1, a1, p2, q2, v2, w2, a2.
#include "unicycle_body.h"

extern "C" void uni_eval(const double* x, double dt, double* e, double* J /* 15 x 30 row-major, or null */) {
  bsg::UniLin L;
  bsg::uni_error(x, x + 3, x + 7, x + 10, x + 13, x + 16, x + 19, x + 23, x + 26, x + 29, dt, e, &L);
  if (!J) return;
  for (int k = 0; k < 30; ++k) {
    double col[15];
    bsg::uni_column(L, x + 3, x + 19, k, col);
    for (int m = 0; m < 15; ++m) J[m * 30 + k] = col[m];
  }
}
