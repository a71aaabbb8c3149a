// Point-to-point ICP of one scan pair (bsgpu_register_scans, k_icp.hip): the reference's generic matcher in its shipped ICP
// configuration (config/matchers/icp.json), as include/bsgpu.h pins it.  libbeam's IcpMatcher and PCL's IterativeClosestPoint are not in
// the reference checkout: the correspondence rule, the Kabsch step and the order of the convergence criteria are RECALLED, not verified.
// Host- and device-compilable in the style of p3p.h and inertial_align.h: plain C++, nothing from HIP but the qualifiers.
//
// Shared by the kernels, the CPU test program (tests/plan/test_icp.cpp) and the one-core timing (scripts/time_icp_cpu.cpp):
//   icp_record, icp_point_record   the 17 sums' terms of one source point from its nearest target within max_corr (point_grid.h: grid_near)
//   icp_jacobi, icp_kabsch_rotation  the 3 x 3 singular value decomposition by Jacobi rotations; the Kabsch rotation
//   icp_step                   the 17 sums of an iteration -> the Kabsch step, T <- dT T, the convergence criteria
//   icp_register_serial        (host only) grid build, iterations and outputs of one pair on one core, in the kernels' order of addition
// The target's grid (cell edge max_corr), the (d^2, index) order of the correspondences and the fixed order of the sums over the source
// points are point_grid.h's, and so is the rule that keeps the device's doubles and the host's the same ("Bits" there): contraction
// off in every body, an fma only where it is written.
#pragma once
#include "point_grid.h"

namespace bsg {

// status of a pair: the first criterion that fired (the values of PCL's DefaultConvergenceCriteria::ConvergenceState, recalled)
enum { ICP_NOT_CONVERGED = 0, ICP_MAX_ITERATIONS = 1, ICP_TRANSFORM = 2, ICP_ABS_MSE = 3, ICP_REL_MSE = 4, ICP_TOO_FEW_CORRESPONDENCES = 5 };

constexpr int kIcpChunk = 128;        // source points per partial record: point_grid.h's chunk, under the name the tests have read since §8.11
static_assert(kIcpChunk == kGridChunk, "one chunk size");
constexpr int kIcpRec = 17;           // [count | sum s (3) | sum q (3) | sum s_a q_b (9, a-major) | sum d^2]
constexpr int kIcpMinCorr = 3;

struct IcpParams {
  int max_iter;
  double t_eps, fit_eps, rotation_threshold, rel_mse_eps;
};

// The terms of one source point under T from s = T S_i and its correspondence q at squared distance d2 — zeros when it has none
BSG_GRID_FN void icp_record(bool kept, const double* s, const double* q, double d2, double* r) {
  BSG_GRID_EXACT
  r[0] = kept ? 1.0 : 0.0;
  r[1] = kept ? s[0] : 0.0; r[2] = kept ? s[1] : 0.0; r[3] = kept ? s[2] : 0.0;
  r[4] = kept ? q[0] : 0.0; r[5] = kept ? q[1] : 0.0; r[6] = kept ? q[2] : 0.0;
  r[7] = kept ? s[0] * q[0] : 0.0; r[8] = kept ? s[0] * q[1] : 0.0; r[9] = kept ? s[0] * q[2] : 0.0;
  r[10] = kept ? s[1] * q[0] : 0.0; r[11] = kept ? s[1] * q[1] : 0.0; r[12] = kept ? s[1] * q[2] : 0.0;
  r[13] = kept ? s[2] * q[0] : 0.0; r[14] = kept ? s[2] * q[1] : 0.0; r[15] = kept ? s[2] * q[2] : 0.0;
  r[16] = kept ? d2 : 0.0;
}
// ICP's correspondence: the nearest target of s within max_corr (closed: d^2 <= h2) through the target's grid, whose cell edge is
// max_corr (grid_near).  q_out, idx_out: the nearest seen, whatever the threshold says.
BSG_GRID_FN bool icp_nearest(const PointGrid& g, const int* cell_end, const double* rec, const double* s, double h2, double* d2_out,
                             double* q_out, double* idx_out) {
  GridBest m;
  const bool kept = grid_near(g, cell_end, rec, s, h2, &m);
  *d2_out = m.d2; *idx_out = m.idx;
  q_out[0] = m.x; q_out[1] = m.y; q_out[2] = m.z;
  return kept;
}
BSG_GRID_FN void icp_point_record(const double* T, const double* S, const PointGrid& g, const int* cell_end, const double* rec, double h2,
                                  double* r) {
  double s[3], q[3], d2, idx;
  grid_apply(T, S, s);
  const bool kept = icp_nearest(g, cell_end, rec, s, h2, &d2, q, &idx);
  icp_record(kept, s, q, d2, r);
}

// ---- the 3 x 3 singular value decomposition: one-sided Jacobi (Hestenes), in registers ---------------------------------------------------
// One rotation of the columns P, Q of a (and of v) that makes them orthogonal; false: they already are, to rounding.
template <int P, int Q>
BSG_GRID_FN bool icp_jacobi(double a[3][3], double v[3][3]) {
  BSG_GRID_EXACT
  const double alpha = a[0][P] * a[0][P] + a[1][P] * a[1][P] + a[2][P] * a[2][P];
  const double beta = a[0][Q] * a[0][Q] + a[1][Q] * a[1][Q] + a[2][Q] * a[2][Q];
  const double gamma = a[0][P] * a[0][Q] + a[1][P] * a[1][Q] + a[2][P] * a[2][Q];
  if (!(fabs(gamma) > kGridEps * sqrt(alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = c * t;
  for (int k = 0; k < 3; ++k) {
    const double ap = a[k][P], aq = a[k][Q], vp = v[k][P], vq = v[k][Q];
    a[k][P] = c * ap - s * aq; a[k][Q] = s * ap + c * aq;
    v[k][P] = c * vp - s * vq; v[k][Q] = s * vp + c * vq;
  }
  return true;
}
// columns P < Q of a and v and their norms into falling order of the norm
template <int P, int Q>
BSG_GRID_FN void icp_order(double* sig, double a[3][3], double v[3][3]) {
  const bool sw = sig[Q] > sig[P];
  const double sp = sig[P], sq = sig[Q];
  sig[P] = sw ? sq : sp; sig[Q] = sw ? sp : sq;
  for (int k = 0; k < 3; ++k) {
    const double ap = a[k][P], aq = a[k][Q], vp = v[k][P], vq = v[k][Q];
    a[k][P] = sw ? aq : ap; a[k][Q] = sw ? ap : aq;
    v[k][P] = sw ? vq : vp; v[k][Q] = sw ? vp : vq;
  }
}
// The rotation R that minimises sum |R (s - cs) + cq - q|^2 for the cross-covariance H = sum (s - cs)(q - cq)^T = U S V^T:
// R = V diag(1, 1, det(V U^T)) U^T (Kabsch / Umeyama without scale).  H V = U S by rotations of H's columns; with the columns in
// falling order of their norms, u3 = u1 x u2 and v3 = v1 x v2 make both factors proper rotations, which IS the determinant fix: it
// flips the direction of the smallest singular value when det(V U^T) < 0.  A cross-covariance of rank < 2 (all kept points on a line)
// has no second direction: the step's rotation is then the identity.  R row-major.
BSG_GRID_FN void icp_kabsch_rotation(const double* H, double* R) {
  BSG_GRID_EXACT
  double a[3][3], v[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { a[i][j] = H[3 * i + j]; v[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 30; ++sweep) {
    const bool r01 = icp_jacobi<0, 1>(a, v), r02 = icp_jacobi<0, 2>(a, v), r12 = icp_jacobi<1, 2>(a, v);
    if (!(r01 || r02 || r12)) break;
  }
  double sig[3];
  for (int j = 0; j < 3; ++j) sig[j] = sqrt(a[0][j] * a[0][j] + a[1][j] * a[1][j] + a[2][j] * a[2][j]);
  icp_order<0, 1>(sig, a, v); icp_order<1, 2>(sig, a, v); icp_order<0, 1>(sig, a, v);
  const bool ok = sig[1] > 0.0 && sig[0] < std::numeric_limits<double>::infinity();
  const double i0 = 1.0 / sig[0], i1 = 1.0 / sig[1];
  const double u1[3] = {a[0][0] * i0, a[1][0] * i0, a[2][0] * i0}, u2[3] = {a[0][1] * i1, a[1][1] * i1, a[2][1] * i1};
  const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
  const double v1[3] = {v[0][0], v[1][0], v[2][0]}, v2[3] = {v[0][1], v[1][1], v[2][1]};
  const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = ok ? v1[i] * u1[j] + v2[i] * u2[j] + v3[i] * u3[j] : (i == j ? 1.0 : 0.0);
}

// Iteration k (1-based) from its 17 sums: returns the status that ends the pair, or ICP_NOT_CONVERGED to go on.  Fewer than 3
// correspondences: T stays.  Otherwise T <- dT T, then the criteria in PCL's order (recalled): k >= max_iter; the step's rotation
// cosine 1/2 (tr dR - 1) >= rotation_threshold and |dt|^2 <= t_eps; |mse - mse_prev| < fit_eps; the same relative to mse_prev.
// mse: the mean of the kept squared distances of THIS iteration (under T before the step; 0 when nothing was kept).
BSG_GRID_FN int icp_step(const double* sum, int k, const IcpParams& P, double* T, double* mse_prev, double* mse_out, int* n_corr) {
  BSG_GRID_EXACT
  const double n = sum[0];
  *n_corr = (int)n;
  const double mse = n > 0.0 ? sum[16] / n : 0.0;
  *mse_out = mse;
  if (n < (double)kIcpMinCorr) return ICP_TOO_FEW_CORRESPONDENCES;
  const double cs[3] = {sum[1] / n, sum[2] / n, sum[3] / n}, cq[3] = {sum[4] / n, sum[5] / n, sum[6] / n};
  double H[9], R[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) H[3 * a + b] = sum[7 + 3 * a + b] - sum[1 + a] * cq[b];
  icp_kabsch_rotation(H, R);
  double dt[3], Tn[12];
  for (int i = 0; i < 3; ++i) dt[i] = cq[i] - (R[3 * i] * cs[0] + R[3 * i + 1] * cs[1] + R[3 * i + 2] * cs[2]);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) Tn[4 * i + j] = R[3 * i] * T[j] + R[3 * i + 1] * T[4 + j] + R[3 * i + 2] * T[8 + j];
    Tn[4 * i + 3] = Tn[4 * i + 3] + dt[i];
  }
  for (int i = 0; i < 12; ++i) T[i] = Tn[i];
  const double cosine = 0.5 * (R[0] + R[4] + R[8] - 1.0), dt2 = dt[0] * dt[0] + dt[1] * dt[1] + dt[2] * dt[2];
  const double prev = *mse_prev, diff = fabs(mse - prev);
  *mse_prev = mse;
  if (k >= P.max_iter) return ICP_MAX_ITERATIONS;
  if (cosine >= P.rotation_threshold && dt2 <= P.t_eps) return ICP_TRANSFORM;
  if (diff < P.fit_eps) return ICP_ABS_MSE;
  if (diff / prev < P.rel_mse_eps) return ICP_REL_MSE;
  return ICP_NOT_CONVERGED;
}
// steps applied when iteration k ended the pair with `status`
BSG_GRID_FN int icp_iterations(int status, int k) { return status == ICP_TOO_FEW_CORRESPONDENCES ? k - 1 : k; }

// out = inv(T) Tinit (MatchScans' T_LIDARREF_LIDARTGT = InvertTransform(T_RefEst_Ref) * T_LidarRefEst_LidarTgt), all row-major 3 x 4
BSG_GRID_FN void icp_inverse_times(const double* T, const double* Ti, double* out) {
  BSG_GRID_EXACT
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) out[4 * i + j] = T[i] * Ti[j] + T[4 + i] * Ti[4 + j] + T[8 + i] * Ti[8 + j];
    out[4 * i + 3] = out[4 * i + 3] - (T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11]);
  }
}

// ---- one pair on one core (host) ---------------------------------------------------------------------------------------------------------
// (the serial grid under the names of the CPU drivers that were written when it lived in this file)
using IcpSerialGrid = SerialGrid;
inline bool icp_grid_build_serial(int n, const double* q, double h, double max_cells, IcpSerialGrid* G) { return grid_build_serial(n, q, h, max_cells, G); }

// bsgpu_register_scans for one pair.  false: the grid would exceed max_cells (the entry point's BSGPU_ERR_UNSUPPORTED).
inline bool icp_register_serial(int n_src, const double* S, int n_tgt, const double* Q, const double* T_init, double max_corr,
                                const IcpParams& P, double max_cells, double* T, double* T_ref_tgt, double* mse, int* n_corr,
                                int* n_iters, int* status) {
  BSG_GRID_EXACT
  static const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const double* Ti = T_init ? T_init : eye;
  std::vector<double> tq(3 * (size_t)n_tgt);
  for (int i = 0; i < n_tgt; ++i) grid_apply(Ti, Q + 3 * i, &tq[3 * (size_t)i]);
  SerialGrid G;
  if (!grid_build_serial(n_tgt, tq.data(), max_corr, max_cells, &G)) return false;
  const double h2 = max_corr * max_corr;
  for (int i = 0; i < 12; ++i) T[i] = eye[i];
  double mse_prev = std::numeric_limits<double>::infinity();
  *status = ICP_NOT_CONVERGED; *n_iters = 0; *n_corr = 0; *mse = 0.0;
  for (int k = 1; *status == ICP_NOT_CONVERGED; ++k) {
    double sum[kIcpRec];
    grid_chunked_sums<kIcpRec>(n_src, [&](int i, double* r) { icp_point_record(T, S + 3 * (size_t)i, G.g, G.cell_end.data(), G.rec.data(), h2, r); }, sum);
    *status = icp_step(sum, k, P, T, &mse_prev, mse, n_corr);
    *n_iters = icp_iterations(*status, k);
  }
  if (T_ref_tgt) icp_inverse_times(T, Ti, T_ref_tgt);
  return true;
}

}  // namespace bsg
