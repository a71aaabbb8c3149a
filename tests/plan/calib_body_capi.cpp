// beam_slam_amd/csrc/calib_body.h on the CPU: a C entry point over the shared functions, loaded with ctypes by tests/test_calib_body.py.
// K: fx, fy, cx, cy; uvw: u, v (pixel), w; E: [E row 0 (theta: 3, p: 3) | E row 1].
#include "calib_body.h"

extern "C" void calib_eval(const double* q_wb, const double* t_wb, const double* P, const double* q_bc, const double* p_bc, const double* K,
                           const double* uvw, int loss_kind, double loss_a, int theta_free, int p_free, double* E) {
  double R_cb[9], t_cb[3];
  bsg::calib_camera(q_bc, p_bc, R_cb, t_cb);
  bsg::calib_E(q_wb, t_wb, P, R_cb, t_cb, K[0], K[1], K[2], K[3], uvw[0], uvw[1], uvw[2], loss_kind, loss_a, theta_free != 0, p_free != 0, E);
}
