// LOAM feature registration of one scan pair (bsgpu_register_scans_loam, k_loam.hip): the reference's LoamMatcher from feature clouds,
// as include/bsgpu.h pins it.  libbeam's LoamMatcher, LoamScanRegistration and its two Ceres cost functions are not in the reference
// checkout: the correspondence rules, the residuals and the outer criterion are RECALLED, not verified.  Host- and device-compilable in
// the manner of gicp.h: the grids, the k-nearest search and the chunked sums are point_grid.h's, the trust-region loop, the loss and
// the 6 x 6 Cholesky are frame_lm.h's (Ceres' Levenberg-Marquardt as lm_state.h restates it).
//
//   loam_quat_plus             frame_lm.h's Plus without library sines: the series of cos and sin(x) / x, halving and squaring
//   loam_edge_residual         r = |(x - a) x (x - b)| / |a - b| and its gradient in x
//   loam_surface_residual      r = n . (x - a) / |n|, n = (b - a) x (c - a), and its gradient in x
//   loam_keep_edge / _surface  the correspondence rules on a neighbour list of grid_knn
//   loam_term                  one measurement's term of the 28-sum record (kFlmSums layout)
//   loam_criterion             the outer criterion
//   loam_run                   the outer loop of one pair over a back-end: loam_register_serial's on the host, the workgroup's in k_loam.hip
//   loam_register_serial       (host only) one pair on one core, in the kernel's order of addition
//
// Roles: the reference clouds are searched, the target features are the queries and it is the target that moves: the estimate is
// T = T_REF_TGT as a pose (q wxyz, p), x = R(q) e + p for a target feature e, tangent [p, theta] with q <- q (x) exp(theta) (frame_lm.h).
//
// Bits.  As in point_grid.h: contraction is off in every body here, and the translation unit of the kernel is compiled with contraction
// off as a whole (csrc/Makefile), because frame_lm.h's helpers carry no pragma of their own; a GCC build passes -ffp-contract=off.  An
// fma appears only where it is written (grid_apply).  Nothing here, and nothing that loam_run reaches in frame_lm.h, calls sin, cos, acos,
// atan or log: the angle test compares a cosine with a bound that the host derives once (loam_cos_bound, host only).
#pragma once
#include "frame_lm.h"
#include "point_grid.h"

namespace bsg {

enum { LOAM_NOT_CONVERGED = 0, LOAM_MAX_ITERATIONS = 1, LOAM_TRANSFORM = 2, LOAM_TOO_FEW_MEASUREMENTS = 5, LOAM_SOLVER_FAILED = 6 };

constexpr int kLoamMaxOuter = 100;
constexpr int kLoamMaxInner = 1000;
constexpr int kLoamMaxFeatures = 65536;
constexpr int kLoamEdgeK = 2, kLoamSurfaceK = 3;

struct LoamParams {
  double mc2;                 // max_corr^2
  int min_measurements, max_outer;
  double conv_translation;    // metres
  double cos_rotation;        // the cosine of conv_rotation_deg, +infinity for 0 (host: loam_cos_bound)
  int loss_kind;
  double loss_a;
  bsgpu_options inner;
};

struct LoamResult {
  double q[4], p[3], cost, cov[36];
  int n_edge, n_surf, n_iters, n_inner, status;
};

// ---- the orientation's Plus ---------------------------------------------------------------------------------------------------------------
// x (x) [cos |w|, sin |w| / |w| w], w = d / 2: flm_quat_plus with the two functions from their series in |w|^2 (ten terms: below 2^-60
// of the sum at |w| <= 1/2); a longer w is halved until |w| <= 1/2 and the quaternion squared as often (gicp_exp's scheme).
BSG_FLM_FN void loam_quat_plus(const double x[4], const double d[3], double out[4]) {
  BSG_GRID_EXACT
  double w[3] = {0.5 * d[0], 0.5 * d[1], 0.5 * d[2]};
  double h2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  int halvings = 0;
  while (h2 > 0.25 && halvings < 64) {
    w[0] = 0.5 * w[0]; w[1] = 0.5 * w[1]; w[2] = 0.5 * w[2];
    h2 = 0.25 * h2;
    ++halvings;
  }
  double C = 1.0, S = 1.0;
  for (int n = 10; n >= 1; --n) {
    C = 1.0 - h2 / (double)((2 * n - 1) * (2 * n)) * C;
    S = 1.0 - h2 / (double)((2 * n) * (2 * n + 1)) * S;
  }
  double b[4] = {C, S * w[0], S * w[1], S * w[2]};
  for (int h = 0; h < halvings; ++h) {
    const double b0 = b[0] * b[0] - (b[1] * b[1] + b[2] * b[2] + b[3] * b[3]), k = 2.0 * b[0];
    b[1] = k * b[1]; b[2] = k * b[2]; b[3] = k * b[3]; b[0] = b0;
  }
  out[0] = x[0] * b[0] - x[1] * b[1] - x[2] * b[2] - x[3] * b[3];
  out[1] = x[0] * b[1] + x[1] * b[0] + x[2] * b[3] - x[3] * b[2];
  out[2] = x[0] * b[2] - x[1] * b[3] + x[2] * b[0] + x[3] * b[1];
  out[3] = x[0] * b[3] + x[1] * b[2] - x[2] * b[1] + x[3] * b[0];
}
struct LoamQuatPlus {
  BSG_FLM_FN void operator()(const double x[4], const double d[3], double out[4]) const { loam_quat_plus(x, d, out); }
};

// (q, p) -> row-major 3 x 4
BSG_FLM_FN void loam_pose_matrix(const double q[4], const double p[3], double T[12]) {
  double R[9];
  flm_quat_to_rot(q, R);
  for (int i = 0; i < 3; ++i) { T[4 * i] = R[3 * i]; T[4 * i + 1] = R[3 * i + 1]; T[4 * i + 2] = R[3 * i + 2]; T[4 * i + 3] = p[i]; }
}

// ---- the two residuals --------------------------------------------------------------------------------------------------------------------
// Point to line through a and b: r = |(x - a) x (x - b)| / |a - b|, g = dr/dx = ((a - b) x v^) / |a - b| with v^ the unit vector of the
// cross product.  r == 0 exactly: g = 0, the library's choice (automatic differentiation of the square root at 0 has no value).
BSG_FLM_FN double loam_edge_residual(const double* x, const double* a, const double* b, double g[3]) {
  BSG_GRID_EXACT
  const double xa[3] = {x[0] - a[0], x[1] - a[1], x[2] - a[2]}, xb[3] = {x[0] - b[0], x[1] - b[1], x[2] - b[2]};
  const double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
  const double v[3] = {xa[1] * xb[2] - xa[2] * xb[1], xa[2] * xb[0] - xa[0] * xb[2], xa[0] * xb[1] - xa[1] * xb[0]};
  const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (nv > 0.0) {
    const double u[3] = {v[0] / nv, v[1] / nv, v[2] / nv};
    g[0] = (d[1] * u[2] - d[2] * u[1]) / len; g[1] = (d[2] * u[0] - d[0] * u[2]) / len; g[2] = (d[0] * u[1] - d[1] * u[0]) / len;
  } else {
    g[0] = 0.0; g[1] = 0.0; g[2] = 0.0;
  }
  return nv / len;
}
// n = (b - a) x (c - a)
BSG_FLM_FN void loam_normal(const double* a, const double* b, const double* c, double n[3]) {
  BSG_GRID_EXACT
  const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  n[0] = u[1] * w[2] - u[2] * w[1]; n[1] = u[2] * w[0] - u[0] * w[2]; n[2] = u[0] * w[1] - u[1] * w[0];
}
// Point to plane through a, b and c: r = n . (x - a) / |n|, g = n / |n|
BSG_FLM_FN double loam_surface_residual(const double* x, const double* a, const double* b, const double* c, double g[3]) {
  BSG_GRID_EXACT
  double n[3];
  loam_normal(a, b, c, n);
  const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  g[0] = n[0] / nn; g[1] = n[1] / nn; g[2] = n[2] / nn;
  return (n[0] * (x[0] - a[0]) + n[1] * (x[1] - a[1]) + n[2] * (x[2] - a[2])) / nn;
}

// ---- the correspondence rules ---------------------------------------------------------------------------------------------------------------
// On the neighbour list of grid_knn (k = 2 / 3, ascending (d^2, index); +infinity where the cloud has no such point); pts: the searched
// cloud.  Kept iff the farthest of the k has d^2 < max_corr^2 (strict: the library's choice) and the neighbours span a line / a plane:
// a != b as points, n not the zero vector as computed (exact degeneracy only: the library's choice).  corr: the k indices.
BSG_FLM_FN bool loam_keep_edge(const double* pts, const double* ld, const double* li, int stride, double mc2, int* corr) {
  if (!(ld[stride] < mc2)) return false;
  corr[0] = (int)li[0]; corr[1] = (int)li[stride];
  const double *a = pts + 3 * (size_t)corr[0], *b = pts + 3 * (size_t)corr[1];
  return a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
}
BSG_FLM_FN bool loam_keep_surface(const double* pts, const double* ld, const double* li, int stride, double mc2, int* corr) {
  if (!(ld[2 * stride] < mc2)) return false;
  corr[0] = (int)li[0]; corr[1] = (int)li[stride]; corr[2] = (int)li[2 * stride];
  double n[3];
  loam_normal(pts + 3 * (size_t)corr[0], pts + 3 * (size_t)corr[1], pts + 3 * (size_t)corr[2], n);
  return n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0;
}

// ---- one measurement's term -----------------------------------------------------------------------------------------------------------------
// e: the target feature before T (what a measurement stores); T = [R | p]; r and g from the residual at x = T e.  With the loss'
// rho(r^2): cost 1/2 rho; the loss-corrected row J = sqrt(rho') [g^T | (e x R^T g)^T] over [p, theta] (dx/dtheta = -R [e]x) and
// residual sqrt(rho') r; t[1 .. 21] J^T J's upper triangle, t[22 .. 27] J^T r.  with_J false: t[0] only.
BSG_FLM_FN void loam_term(const double* T, const double* e, double r, const double g[3], int loss_kind, double loss_a, bool with_J, double* t) {
  BSG_GRID_EXACT
  double rho1;
  const double rho = flm_loss(loss_kind, loss_a, r * r, &rho1);
  t[0] = 0.5 * rho;
  if (!with_J) return;
  const double sc = sqrt(rho1), rc = sc * r;
  const double a[3] = {T[0] * g[0] + T[4] * g[1] + T[8] * g[2], T[1] * g[0] + T[5] * g[1] + T[9] * g[2], T[2] * g[0] + T[6] * g[1] + T[10] * g[2]};
  const double J[6] = {sc * g[0], sc * g[1], sc * g[2], sc * (e[1] * a[2] - e[2] * a[1]), sc * (e[2] * a[0] - e[0] * a[2]), sc * (e[0] * a[1] - e[1] * a[0])};
  int k = 1;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) t[k++] = J[i] * J[j];
  for (int i = 0; i < 6; ++i) t[22 + i] = J[i] * rc;
}
// The term of target feature e with its stored neighbours (corr[0] < 0: not kept, zeros); pts: the searched cloud.
BSG_FLM_FN void loam_feature_term(bool edge, const double* T, const double* e, const int* corr, const double* pts, int loss_kind, double loss_a,
                                  bool with_J, double* t) {
  const int n = with_J ? kFlmSums : 1;
  if (corr[0] < 0) { for (int k = 0; k < n; ++k) t[k] = 0.0; return; }
  double x[3], g[3];
  grid_apply(T, e, x);
  const double* a = pts + 3 * (size_t)corr[0];
  const double* b = pts + 3 * (size_t)corr[1];
  const double r = edge ? loam_edge_residual(x, a, b, g) : loam_surface_residual(x, a, b, pts + 3 * (size_t)corr[2], g);
  loam_term(T, e, r, g, loss_kind, loss_a, with_J, t);
}

// ---- the outer criterion --------------------------------------------------------------------------------------------------------------------
// After outer iteration k moved the pose (q0, p0) to (q, p): k >= max_outer first (MAX_ITERATIONS, a success as in the reference); else
// with D = inv(T0) T: |D.t| < conv_translation and (tr D.R - 1) / 2 > cos_rotation, i.e. the angle below its threshold: TRANSFORM.
BSG_FLM_FN int loam_criterion(const double q0[4], const double p0[3], const double q[4], const double p[3], int k, const LoamParams& P) {
  BSG_GRID_EXACT
  if (k >= P.max_outer) return LOAM_MAX_ITERATIONS;
  double R0[9], R[9];
  flm_quat_to_rot(q0, R0);
  flm_quat_to_rot(q, R);
  const double d[3] = {p[0] - p0[0], p[1] - p0[1], p[2] - p0[2]};
  double t2 = 0.0, tr = 0.0;
  for (int j = 0; j < 3; ++j) {
    const double c = R0[j] * d[0] + R0[3 + j] * d[1] + R0[6 + j] * d[2];      // (R0^T d)_j
    t2 = t2 + c * c;
    tr = tr + (R0[j] * R[j] + R0[3 + j] * R[3 + j] + R0[6 + j] * R[6 + j]);   // (R0^T R)_jj
  }
  return sqrt(t2) < P.conv_translation && (tr - 1.0) / 2.0 > P.cos_rotation ? LOAM_TRANSFORM : LOAM_NOT_CONVERGED;
}

// ---- the outer loop of one pair ---------------------------------------------------------------------------------------------------------------
// B: b.correspond(q, p, &n_edge, &n_surf) finds and stores every target feature's neighbours under the pose and counts the kept;
// b(q, p, with_J, sums) is flm_solve's evaluator over the stored measurements.  Every caller (every lane of a workgroup) gets the same
// counts and sums, so all take the same decisions.
template <class B>
BSG_FLM_FN void loam_run(const LoamParams& P, B& b, LoamResult& out) {
  BSG_GRID_EXACT
  double q[4] = {1.0, 0.0, 0.0, 0.0}, p[3] = {0.0, 0.0, 0.0};
  out.cost = 0.0;
  out.n_edge = 0; out.n_surf = 0; out.n_iters = 0; out.n_inner = 0;
  int status = LOAM_NOT_CONVERGED;
  for (int i = 0; i < 36; ++i) out.cov[i] = NAN;
  for (int k = 1; status == LOAM_NOT_CONVERGED; ++k) {
    b.correspond(q, p, &out.n_edge, &out.n_surf);
    if (out.n_edge + out.n_surf < P.min_measurements) { status = LOAM_TOO_FEW_MEASUREMENTS; break; }
    FlmResult res;
    flm_solve(P.inner, q, p, b, res, nullptr, LoamQuatPlus());
    out.n_inner = out.n_inner + res.iterations;
    out.cost = res.cost;
    if (res.status == FLM_UNUSABLE) { status = LOAM_SOLVER_FAILED; break; }
    status = loam_criterion(q, p, res.q, res.p, k, P);
    for (int i = 0; i < 4; ++i) q[i] = res.q[i];
    for (int i = 0; i < 3; ++i) p[i] = res.p[i];
    for (int i = 0; i < 36; ++i) out.cov[i] = res.cov[i];
    out.n_iters = k;
  }
  if (status != LOAM_MAX_ITERATIONS && status != LOAM_TRANSFORM)
    for (int i = 0; i < 36; ++i) out.cov[i] = NAN;
  for (int i = 0; i < 4; ++i) out.q[i] = q[i];
  for (int i = 0; i < 3; ++i) out.p[i] = p[i];
  out.status = status;
}

// The entry point's transforms from the pose: T_refest_ref = inv(T); T_ref_tgt = T T_init
BSG_FLM_FN void loam_outputs(const double q[4], const double p[3], const double* Ti, double* T_refest_ref, double* T_ref_tgt) {
  BSG_GRID_EXACT
  double T[12];
  loam_pose_matrix(q, p, T);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T_refest_ref[4 * i + j] = T[4 * j + i];
    T_refest_ref[4 * i + 3] = -(T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11]);
    for (int j = 0; j < 4; ++j) T_ref_tgt[4 * i + j] = T[4 * i] * Ti[j] + T[4 * i + 1] * Ti[4 + j] + T[4 * i + 2] * Ti[8 + j];
    T_ref_tgt[4 * i + 3] = T_ref_tgt[4 * i + 3] + T[4 * i + 3];
  }
}

// ---- host only --------------------------------------------------------------------------------------------------------------------------------
// The bound of the angle test, derived once per call: the one library function of the contract, and never the device's.
inline double loam_cos_bound(double conv_rotation_deg) {
  return conv_rotation_deg > 0.0 ? std::cos(conv_rotation_deg * (3.14159265358979323846 / 180.0)) : std::numeric_limits<double>::infinity();
}

// One pair on one core: the back-end of loam_run whose sums are grid_chunked_sums over the target features, edges then surfaces.
struct LoamSerial {
  const LoamParams* P;
  int n_edge, n_surf;                      // target features
  const double *edges, *surfs;             // the reference clouds
  const SerialGrid *GE, *GS;
  std::vector<double> te, ts;              // the target features under T_init
  std::vector<int> corr;                   // 3 per target feature

  void correspond(const double q[4], const double p[3], int* kept_edges, int* kept_surfs) {
    double T[12], x[3], ld[3], li[3];
    loam_pose_matrix(q, p, T);
    *kept_edges = 0; *kept_surfs = 0;
    for (int i = 0; i < n_edge + n_surf; ++i) {
      const bool edge = i < n_edge;
      int* c = &corr[3 * (size_t)i];
      grid_apply(T, edge ? &te[3 * (size_t)i] : &ts[3 * (size_t)(i - n_edge)], x);
      const SerialGrid& G = edge ? *GE : *GS;
      grid_knn(G.g, G.cell_end.data(), G.rec.data(), x, edge ? kLoamEdgeK : kLoamSurfaceK, ld, li, 1);
      const bool kept = edge ? loam_keep_edge(edges, ld, li, 1, P->mc2, c) : loam_keep_surface(surfs, ld, li, 1, P->mc2, c);
      if (!kept) c[0] = -1;
      *(edge ? kept_edges : kept_surfs) += kept ? 1 : 0;
    }
  }
  void operator()(const double q[4], const double p[3], bool with_J, FlmSums& s) {
    double T[12];
    loam_pose_matrix(q, p, T);
    const auto term = [&](int i, double* t) {
      const bool edge = i < n_edge;
      loam_feature_term(edge, T, edge ? &te[3 * (size_t)i] : &ts[3 * (size_t)(i - n_edge)], &corr[3 * (size_t)i], edge ? edges : surfs, P->loss_kind,
                        P->loss_a, with_J, t);
    };
    for (int k = 0; k < kFlmSums; ++k) s.v[k] = 0.0;
    if (with_J) grid_chunked_sums<kFlmSums>(n_edge + n_surf, term, s.v);
    else grid_chunked_sums<1>(n_edge + n_surf, term, s.v);
  }
};

// bsgpu_register_scans_loam for one pair.  false: a grid would exceed max_cells (the entry point's BSGPU_ERR_UNSUPPORTED).
inline bool loam_register_serial(int n_ref_edge, const double* ref_edges, int n_ref_surf, const double* ref_surfs, int n_tgt_edge,
                                 const double* tgt_edges, int n_tgt_surf, const double* tgt_surfs, const double* T_init, const LoamParams& P,
                                 double grid_cell, double max_cells, double* T_refest_ref, double* T_ref_tgt, LoamResult* res) {
  static const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const double* Ti = T_init ? T_init : eye;
  SerialGrid GE, GS;
  if (!grid_build_serial(n_ref_edge, ref_edges, grid_cell, max_cells, &GE) || !grid_build_serial(n_ref_surf, ref_surfs, grid_cell, max_cells, &GS))
    return false;
  LoamSerial b{&P, n_tgt_edge, n_tgt_surf, ref_edges, ref_surfs, &GE, &GS, {}, {}, {}};
  b.te.resize(3 * (size_t)n_tgt_edge); b.ts.resize(3 * (size_t)n_tgt_surf);
  b.corr.assign(3 * (size_t)(n_tgt_edge + n_tgt_surf), -1);
  for (int i = 0; i < n_tgt_edge; ++i) grid_apply(Ti, tgt_edges + 3 * (size_t)i, &b.te[3 * (size_t)i]);
  for (int i = 0; i < n_tgt_surf; ++i) grid_apply(Ti, tgt_surfs + 3 * (size_t)i, &b.ts[3 * (size_t)i]);
  loam_run(P, b, *res);
  loam_outputs(res->q, res->p, Ti, T_refest_ref, T_ref_tgt);
  return true;
}

}  // namespace bsg
