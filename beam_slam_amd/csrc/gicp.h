// Generalized ICP of one scan pair (bsgpu_register_scans_gicp, k_gicp.hip): the reference's GicpMatcher in its shipped configuration
// (config/matchers/gicp.json), as include/bsgpu.h pins it.  libbeam's GicpMatcher and PCL's GeneralizedIterativeClosestPoint are not
// in the reference checkout: the covariances, the correspondence rule, the objective and the outer criterion are RECALLED, not
// verified.  PCL minimises the objective with BFGS over (x, y, z, roll, pitch, yaw); this file minimises the same objective with
// Gauss-Newton steps, so PCL's iterates are NOT reproduced.  Host- and device-compilable in the style of icp.h, whose Jacobi rotation it
// reuses; the clouds' grids, both searches and the chunked sums are point_grid.h's.
//
//   gicp_covariance            PCL's computeCovariances for one point from its neighbour list
//   gicp_mahalanobis           M = (C'^Q_j + R C'^S_i R^T)^-1
//   gicp_terms                 the 28 sums' terms of one correspondence: 21 of H's upper triangle, 6 of g, 1 of F
//   gicp_solve, gicp_exp       the 6 x 6 Cholesky step; Rodrigues' formula without library sines
//   gicp_advance               one Gauss-Newton step of one pair from its sums, the inner and the outer criteria
//   gicp_register_serial       (host only) one pair on one core, in the kernels' order of addition
//
// Bits.  As in point_grid.h: contraction is off in every body, an fma appears only where it is written (grid_apply), the sums over
// the correspondences have its fixed order; the k neighbours of a point are summed in their (d^2, index) order.  No function of this file calls
// sin, cos or any other library function that is not correctly rounded on both sides.
#pragma once
#include "icp.h"
#include "point_grid.h"

namespace bsg {

enum { GICP_NOT_CONVERGED = 0, GICP_MAX_ITERATIONS = 1, GICP_TRANSFORM = 2, GICP_TOO_FEW_CORRESPONDENCES = 5, GICP_DEGENERATE = 6 };

constexpr int kGicpMaxK = 32;
constexpr int kGicpMaxInner = 64;
constexpr int kGicpMinCorr = 4;
constexpr int kGicpRec = 28;            // [H upper triangle, row-major (21) | g (6) | F]
constexpr double kGicpPivot = 1e-12;    // a Cholesky pivot <= this x its diagonal entry of H: DEGENERATE

struct GicpParams {
  int k;
  double epsilon, max_corr;
  int max_iter;
  double r_eps, t_eps;
  int max_inner;
  double inner_eps;
};

// What a pair carries from launch to launch (and gicp_register_serial from step to step).  stopped_at: the outer iteration whose
// inner loop has ended.
struct GicpState {
  double T[12], T0[12], cost;
  int n_corr, n_iters, n_inner, status, stopped_at;
};

// ---- the searches -----------------------------------------------------------------------------------------------------------------------
// GICP's two searches are point_grid.h's shell searches: the k nearest points of a cloud for a covariance, and the correspondence,
// the nearest target below max_corr (strict: d^2 < mc2).  q_out, idx_out: the nearest seen, whatever the threshold says.
BSG_GRID_FN void gicp_knn(const PointGrid& g, const int* cell_end, const double* rec, const double* x, int k, double* ld, double* li, int stride) {
  grid_knn(g, cell_end, rec, x, k, ld, li, stride);
}
BSG_GRID_FN bool gicp_nearest(const PointGrid& g, const int* cell_end, const double* rec, const double* x, double mc2, double* d2_out, double* q_out,
                              double* idx_out) {
  GridBest m;
  const bool kept = grid_shell_nearest(g, cell_end, rec, x, mc2, &m);
  *d2_out = m.d2; *idx_out = m.idx;
  q_out[0] = m.x; q_out[1] = m.y; q_out[2] = m.z;
  return kept;
}

// ---- covariances ----------------------------------------------------------------------------------------------------------------------------
// C' of one point from its k neighbours (indices into pts, 3 doubles each, in list order): mean, centred covariance (1/k), its
// eigenvectors by Jacobi rotations (icp.h's rotation on the symmetric matrix: the columns of C V become orthogonal, their norms are
// the eigenvalues, V's columns the eigenvectors), eigenvalues in falling order, C' = u1 u1^T + u2 u2^T + epsilon u3 u3^T.
// c6: xx, xy, xz, yy, yz, zz.  A covariance without a direction (all neighbours equal) leaves V = I: C' = diag(1, 1, epsilon).
BSG_GRID_FN void gicp_covariance(const double* pts, const double* li, int stride, int k, double epsilon, double* c6) {
  BSG_GRID_EXACT
  double mx = 0.0, my = 0.0, mz = 0.0;
  for (int j = 0; j < k; ++j) {
    const double* p = pts + 3 * (size_t)li[j * stride];
    mx = mx + p[0]; my = my + p[1]; mz = mz + p[2];
  }
  const double kd = (double)k;
  mx = mx / kd; my = my / kd; mz = mz / kd;
  double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  for (int j = 0; j < k; ++j) {
    const double* p = pts + 3 * (size_t)li[j * stride];
    const double dx = p[0] - mx, dy = p[1] - my, dz = p[2] - mz;
    xx = xx + dx * dx; xy = xy + dx * dy; xz = xz + dx * dz; yy = yy + dy * dy; yz = yz + dy * dz; zz = zz + dz * dz;
  }
  double a[3][3] = {{xx / kd, xy / kd, xz / kd}, {xy / kd, yy / kd, yz / kd}, {xz / kd, yz / kd, zz / kd}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < 30; ++sweep) {
    const bool r01 = icp_jacobi<0, 1>(a, v), r02 = icp_jacobi<0, 2>(a, v), r12 = icp_jacobi<1, 2>(a, v);
    if (!(r01 || r02 || r12)) break;
  }
  double sig[3];
  for (int j = 0; j < 3; ++j) sig[j] = sqrt(a[0][j] * a[0][j] + a[1][j] * a[1][j] + a[2][j] * a[2][j]);
  icp_order<0, 1>(sig, a, v); icp_order<1, 2>(sig, a, v); icp_order<0, 1>(sig, a, v);
  c6[0] = (v[0][0] * v[0][0] + v[0][1] * v[0][1]) + epsilon * (v[0][2] * v[0][2]);
  c6[1] = (v[0][0] * v[1][0] + v[0][1] * v[1][1]) + epsilon * (v[0][2] * v[1][2]);
  c6[2] = (v[0][0] * v[2][0] + v[0][1] * v[2][1]) + epsilon * (v[0][2] * v[2][2]);
  c6[3] = (v[1][0] * v[1][0] + v[1][1] * v[1][1]) + epsilon * (v[1][2] * v[1][2]);
  c6[4] = (v[1][0] * v[2][0] + v[1][1] * v[2][1]) + epsilon * (v[1][2] * v[2][2]);
  c6[5] = (v[2][0] * v[2][0] + v[2][1] * v[2][1]) + epsilon * (v[2][2] * v[2][2]);
}

// M = (C'^Q + R C'^S R^T)^-1, R the rotation block of T (row-major 3 x 4); the inverse of the symmetric positive definite sum by
// its cofactors.  All three as xx, xy, xz, yy, yz, zz.
BSG_GRID_FN void gicp_mahalanobis(const double* T, const double* cs, const double* cq, double* m6) {
  BSG_GRID_EXACT
  const double C[3][3] = {{cs[0], cs[1], cs[2]}, {cs[1], cs[3], cs[4]}, {cs[2], cs[4], cs[5]}};
  double P[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) P[i][j] = T[4 * i] * C[0][j] + T[4 * i + 1] * C[1][j] + T[4 * i + 2] * C[2][j];
  const double a00 = cq[0] + (P[0][0] * T[0] + P[0][1] * T[1] + P[0][2] * T[2]);
  const double a01 = cq[1] + (P[0][0] * T[4] + P[0][1] * T[5] + P[0][2] * T[6]);
  const double a02 = cq[2] + (P[0][0] * T[8] + P[0][1] * T[9] + P[0][2] * T[10]);
  const double a11 = cq[3] + (P[1][0] * T[4] + P[1][1] * T[5] + P[1][2] * T[6]);
  const double a12 = cq[4] + (P[1][0] * T[8] + P[1][1] * T[9] + P[1][2] * T[10]);
  const double a22 = cq[5] + (P[2][0] * T[8] + P[2][1] * T[9] + P[2][2] * T[10]);
  const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  m6[0] = c00 / det; m6[1] = c01 / det; m6[2] = c02 / det; m6[3] = c11 / det; m6[4] = c12 / det; m6[5] = c22 / det;
}

// ---- the sums' terms ------------------------------------------------------------------------------------------------------------------------
// One correspondence under T: s = T S_i, r = s - q, J = [-[s]x | I] (column k of -[s]x is e_k x s).  H = J^T M J (upper triangle,
// row-major), g = J^T M r, F = r^T M r; zeros when the point has no correspondence.
BSG_GRID_FN void gicp_terms(bool kept, const double* s, const double* q, const double* m6, double* t) {
  BSG_GRID_EXACT
  const double M[3][3] = {{m6[0], m6[1], m6[2]}, {m6[1], m6[3], m6[4]}, {m6[2], m6[4], m6[5]}};
  const double A[3][3] = {{0.0, -s[2], s[1]}, {s[2], 0.0, -s[0]}, {-s[1], s[0], 0.0}};      // A[k]: e_k x s
  const double r[3] = {s[0] - q[0], s[1] - q[1], s[2] - q[2]};
  double MA[3][3], Mr[3];                                                                   // MA[k] = M (e_k x s)
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i) MA[k][i] = M[i][0] * A[k][0] + M[i][1] * A[k][1] + M[i][2] * A[k][2];
  for (int i = 0; i < 3; ++i) Mr[i] = M[i][0] * r[0] + M[i][1] * r[1] + M[i][2] * r[2];
  double H[6][6];
  for (int k = 0; k < 3; ++k) {
    for (int l = k; l < 3; ++l) H[k][l] = A[k][0] * MA[l][0] + A[k][1] * MA[l][1] + A[k][2] * MA[l][2];
    for (int l = 0; l < 3; ++l) H[k][3 + l] = MA[k][l];
    for (int l = k; l < 3; ++l) H[3 + k][3 + l] = M[k][l];
  }
  int at = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) t[at++] = kept ? H[i][j] : 0.0;
  for (int k = 0; k < 3; ++k) t[21 + k] = kept ? A[k][0] * Mr[0] + A[k][1] * Mr[1] + A[k][2] * Mr[2] : 0.0;
  for (int k = 0; k < 3; ++k) t[24 + k] = kept ? Mr[k] : 0.0;
  t[27] = kept ? r[0] * Mr[0] + r[1] * Mr[1] + r[2] * Mr[2] : 0.0;
}

// ---- the step -------------------------------------------------------------------------------------------------------------------------------
// xi = -H^-1 g by a Cholesky factorisation of the summed H.  false: a pivot <= kGicpPivot x its diagonal entry of H (or not a number).
BSG_GRID_FN bool gicp_solve(const double* sum, double* xi) {
  BSG_GRID_EXACT
  double H[6][6], L[6][6], y[6];
  int at = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { H[i][j] = sum[at]; H[j][i] = sum[at]; ++at; }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) L[i][j] = 0.0;
  bool ok = true;
  for (int j = 0; j < 6; ++j) {
    double d = H[j][j];
    for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
    ok = ok && d > kGicpPivot * H[j][j];
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double v = H[i][j];
      for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  for (int i = 0; i < 6; ++i) {
    double v = -sum[21 + i];
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * xi[k];
    xi[i] = v / L[i][i];
  }
  return ok;
}
// R = exp([w]x) by Rodrigues' formula, R = I + A [w]x + B [w]x^2 with A = sin(th) / th and B = (1 - cos th) / th^2 from their series
// in th^2 (ten terms: below 2^-60 of the sum at th <= 1/2); a longer w is halved until th <= 1/2 and the rotation squared as often.
BSG_GRID_FN void gicp_exp(const double* w_in, double* R) {
  BSG_GRID_EXACT
  double w[3] = {w_in[0], w_in[1], w_in[2]};
  double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  int halvings = 0;
  while (th2 > 0.25 && halvings < 64) {
    w[0] = 0.5 * w[0]; w[1] = 0.5 * w[1]; w[2] = 0.5 * w[2];
    th2 = 0.25 * th2;
    ++halvings;
  }
  double A = 1.0, B = 1.0;
  for (int n = 10; n >= 1; --n) {
    A = 1.0 - th2 / (double)((2 * n) * (2 * n + 1)) * A;
    B = 1.0 - th2 / (double)((2 * n + 1) * (2 * n + 2)) * B;
  }
  B = 0.5 * B;
  R[0] = 1.0 + B * (w[0] * w[0] - th2); R[1] = B * (w[0] * w[1]) - A * w[2]; R[2] = B * (w[0] * w[2]) + A * w[1];
  R[3] = B * (w[0] * w[1]) + A * w[2]; R[4] = 1.0 + B * (w[1] * w[1] - th2); R[5] = B * (w[1] * w[2]) - A * w[0];
  R[6] = B * (w[0] * w[2]) - A * w[1]; R[7] = B * (w[1] * w[2]) + A * w[0]; R[8] = 1.0 + B * (w[2] * w[2] - th2);
  for (int h = 0; h < halvings; ++h) {
    double Q[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Q[3 * i + j] = R[3 * i] * R[j] + R[3 * i + 1] * R[3 + j] + R[3 * i + 2] * R[6 + j];
    for (int i = 0; i < 9; ++i) R[i] = Q[i];
  }
}
// T <- [exp(w) | v] T, xi = (w, v)
BSG_GRID_FN void gicp_update(const double* xi, double* T) {
  BSG_GRID_EXACT
  double R[9], Tn[12];
  gicp_exp(xi, R);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) Tn[4 * i + j] = R[3 * i] * T[j] + R[3 * i + 1] * T[4 + j] + R[3 * i + 2] * T[8 + j];
    Tn[4 * i + 3] = Tn[4 * i + 3] + xi[3 + i];
  }
  for (int i = 0; i < 12; ++i) T[i] = Tn[i];
}
// PCL's outer rule (recalled): delta = max(max |R - R0| / r_eps, max |t - t0| / t_eps); k >= max_iter first, then delta < 1
BSG_GRID_FN int gicp_outer_status(const double* T0, const double* T, int k, const GicpParams& P) {
  BSG_GRID_EXACT
  double delta = 0.0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      const double v = fabs(T[4 * i + j] - T0[4 * i + j]) / P.r_eps;
      delta = v > delta ? v : delta;
    }
    const double v = fabs(T[4 * i + 3] - T0[4 * i + 3]) / P.t_eps;
    delta = v > delta ? v : delta;
  }
  if (k >= P.max_iter) return GICP_MAX_ITERATIONS;
  return delta < 1.0 ? GICP_TRANSFORM : GICP_NOT_CONVERGED;
}

BSG_GRID_FN void gicp_state_init(bool enough_points, GicpState* st) {
  for (int i = 0; i < 12; ++i) { st->T[i] = i % 5 == 0 ? 1.0 : 0.0; st->T0[i] = st->T[i]; }
  st->cost = 0.0;
  st->n_corr = 0; st->n_iters = 0; st->n_inner = 0; st->stopped_at = 0;
  st->status = enough_points ? GICP_NOT_CONVERGED : GICP_TOO_FEW_CORRESPONDENCES;
}
// Gauss-Newton step `it` (1-based) of outer iteration k from the 28 sums and the number of kept correspondences.  Fewer than 4 kept:
// TOO_FEW_CORRESPONDENCES, T stays.  A refused pivot: DEGENERATE, T as before this outer iteration.  Otherwise the step is applied;
// the inner loop ends after the step whose max |xi| < inner_eps, or after max_inner steps, and the outer criterion is then taken.
BSG_GRID_FN void gicp_advance(const double* sum, int n_kept, int k, int it, const GicpParams& P, GicpState* st) {
  BSG_GRID_EXACT
  if (it == 1) {
    for (int i = 0; i < 12; ++i) st->T0[i] = st->T[i];
    st->n_corr = n_kept;
  }
  if (n_kept < kGicpMinCorr) { st->status = GICP_TOO_FEW_CORRESPONDENCES; st->n_iters = k - 1; st->stopped_at = k; return; }
  st->cost = sum[27] / (double)n_kept;
  double xi[6];
  if (!gicp_solve(sum, xi)) {
    for (int i = 0; i < 12; ++i) st->T[i] = st->T0[i];
    st->status = GICP_DEGENERATE; st->n_iters = k - 1; st->stopped_at = k;
    return;
  }
  gicp_update(xi, st->T);
  st->n_inner = st->n_inner + 1;
  bool small = true;
  for (int i = 0; i < 6; ++i) small = small && fabs(xi[i]) < P.inner_eps;
  if (small || it >= P.max_inner) {
    st->stopped_at = k;
    st->n_iters = k;
    st->status = gicp_outer_status(st->T0, st->T, k, P);
  }
}

// ---- one pair on one core (host) ------------------------------------------------------------------------------------------------------------
// The covariances of one cloud (already in the frame it is searched in) through its grid; cov: 6 per point.
inline void gicp_cloud_covariances(int n, const double* pts, const SerialGrid& G, int k, double epsilon, double* cov) {
  std::vector<double> ld((size_t)k), li((size_t)k);
  for (int i = 0; i < n; ++i) {
    gicp_knn(G.g, G.cell_end.data(), G.rec.data(), pts + 3 * (size_t)i, k, ld.data(), li.data(), 1);
    gicp_covariance(pts, li.data(), 1, k, epsilon, cov + 6 * (size_t)i);
  }
}

// bsgpu_register_scans_gicp for one pair.  false: a grid would exceed max_cells (the entry point's BSGPU_ERR_UNSUPPORTED).
// ref_cov (6 n_src) and tgt_cov (6 n_tgt) may be null; they are zero for a pair with a cloud of fewer than k points.
inline bool gicp_register_serial(int n_src, const double* S, int n_tgt, const double* Q, const double* T_init, const GicpParams& P,
                                 double grid_cell, double max_cells, double* T, double* T_ref_tgt, double* cost, int* n_corr, int* n_iters,
                                 int* n_inner, int* status, double* ref_cov, double* tgt_cov) {
  BSG_GRID_EXACT
  static const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const double* Ti = T_init ? T_init : eye;
  std::vector<double> tq(3 * (size_t)n_tgt);
  for (int i = 0; i < n_tgt; ++i) grid_apply(Ti, Q + 3 * i, &tq[3 * (size_t)i]);
  SerialGrid GS, GQ;
  if (!grid_build_serial(n_src, S, grid_cell, max_cells, &GS) || !grid_build_serial(n_tgt, tq.data(), grid_cell, max_cells, &GQ)) return false;
  std::vector<double> cs(6 * (size_t)n_src, 0.0), cq(6 * (size_t)n_tgt, 0.0);
  if (n_src >= P.k) gicp_cloud_covariances(n_src, S, GS, P.k, P.epsilon, cs.data());
  if (n_tgt >= P.k) gicp_cloud_covariances(n_tgt, tq.data(), GQ, P.k, P.epsilon, cq.data());
  if (ref_cov) for (size_t i = 0; i < cs.size(); ++i) ref_cov[i] = cs[i];
  if (tgt_cov) for (size_t i = 0; i < cq.size(); ++i) tgt_cov[i] = cq[i];
  GicpState st;
  gicp_state_init(n_src >= P.k && n_tgt >= P.k, &st);
  const double mc2 = P.max_corr * P.max_corr;
  std::vector<double> M(6 * (size_t)n_src);
  std::vector<int> corr((size_t)n_src);
  for (int k = 1; st.status == GICP_NOT_CONVERGED; ++k) {
    int kept = 0;
    for (int i = 0; i < n_src; ++i) {
      double s[3], q[3], d2, idx;
      grid_apply(st.T, S + 3 * (size_t)i, s);
      const bool keep = gicp_nearest(GQ.g, GQ.cell_end.data(), GQ.rec.data(), s, mc2, &d2, q, &idx);
      corr[i] = keep ? (int)idx : -1;
      kept += keep ? 1 : 0;
      if (keep) gicp_mahalanobis(st.T, &cs[6 * (size_t)i], &cq[6 * (size_t)corr[i]], &M[6 * (size_t)i]);
      else for (int t = 0; t < 6; ++t) M[6 * (size_t)i + t] = 0.0;
    }
    for (int it = 1; st.status == GICP_NOT_CONVERGED && st.stopped_at != k; ++it) {
      double sum[kGicpRec];
      grid_chunked_sums<kGicpRec>(n_src, [&](int i, double* r) {
        if (corr[i] < 0) { for (int t = 0; t < kGicpRec; ++t) r[t] = 0.0; return; }
        double s[3];
        grid_apply(st.T, S + 3 * (size_t)i, s);
        gicp_terms(true, s, &tq[3 * (size_t)corr[i]], &M[6 * (size_t)i], r);
      }, sum);
      gicp_advance(sum, kept, k, it, P, &st);
    }
  }
  for (int i = 0; i < 12; ++i) T[i] = st.T[i];
  if (T_ref_tgt) icp_inverse_times(st.T, Ti, T_ref_tgt);
  *cost = st.cost; *n_corr = st.n_corr; *n_iters = st.n_iters; *n_inner = st.n_inner; *status = st.status;
  return true;
}

}  // namespace bsg
