// Point-to-point ICP of one scan pair (bsgpu_register_scans, k_icp.hip): the reference's generic matcher in its shipped ICP
// configuration (config/matchers/icp.json), as include/bsgpu.h pins it.  libbeam's IcpMatcher and PCL's IterativeClosestPoint are not in
// the reference checkout: the correspondence rule, the Kabsch step and the order of the convergence criteria are RECALLED, not verified.
// Host- and device-compilable in the style of p3p.h and inertial_align.h: plain C++, nothing from HIP but the qualifiers.
//
// Shared by the kernels, the CPU test program (tests/plan/test_icp.cpp) and the one-core timing (scripts/time_icp_cpu.cpp):
//   icp_apply, icp_cell_of     a point through a 3 x 4 transform; its cell of the target grid
//   icp_nearest[_part]         the thresholded nearest neighbour of one point through the grid (exact: see there)
//   icp_point_record           the 17 sums' terms of one source point
//   icp_step                   the 17 sums of an iteration -> the Kabsch step, T <- dT T, the convergence criteria
//   icp_register_serial        (host only) grid build, iterations and outputs of one pair on one core, in the kernels' order of addition
//
// Bits.  Device and host must produce the same doubles (tests/test_gpu_register_scans.py compares them bit for bit), so every function
// body switches floating-point contraction off (clang's pragma; a GCC build of this header passes -ffp-contract=off, which matters
// where the target has a fused multiply-add): a * b + c is two roundings on both sides, and fma() appears only where it is written.
// Division and square root are correctly rounded on both.  The sums over the correspondences are taken in a fixed order: source points
// in chunks of kIcpChunk; inside a chunk the tree of a 64-lane shuffle-down reduction per wave, the waves then in order; the chunks in
// order.  icp_register_serial walks the same tree, so a pair's result depends neither on its neighbours in the batch nor on the launch.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define BSG_ICP_FN __host__ __device__ inline
#else
#define BSG_ICP_FN inline
#endif
#if defined(__clang__)
#define BSG_ICP_EXACT _Pragma("clang fp contract(off)")
#else
#define BSG_ICP_EXACT
#endif

namespace bsg {

// status of a pair: the first criterion that fired (the values of PCL's DefaultConvergenceCriteria::ConvergenceState, recalled)
enum { ICP_NOT_CONVERGED = 0, ICP_MAX_ITERATIONS = 1, ICP_TRANSFORM = 2, ICP_ABS_MSE = 3, ICP_REL_MSE = 4, ICP_TOO_FEW_CORRESPONDENCES = 5 };

constexpr int kIcpChunk = 128;        // source points per partial record (one workgroup); their sums: two waves' trees
constexpr int kIcpWave = 64;
constexpr int kIcpSub = 8;            // lanes that share one source point's candidates in the kernel
constexpr int kIcpRec = 17;           // [count | sum s (3) | sum q (3) | sum s_a q_b (9, a-major) | sum d^2]
constexpr int kIcpMinCorr = 3;
constexpr double kIcpEps = 2.220446049250313e-16;   // 2^-52

// The target's dense grid: cell edge h = max_corr, origin at the bounding box's lower corner, n cells per axis, x fastest.  The cells
// of all pairs of a call lie in one array, this pair's from cell0; cell_end[c] is where cell c's records end in the sorted records
// of the whole call, and they begin where cell c - 1's end (at 0 for c == 0).
struct IcpGrid {
  double o[3];
  double h;
  int n[3];
  int cell0;
};

struct IcpParams {
  int max_iter;
  double t_eps, fit_eps, rotation_threshold, rel_mse_eps;
};

// out = T p, T row-major 3 x 4.  (The only fused multiply-adds of this file: written, so the same on both sides.)
BSG_ICP_FN void icp_apply(const double* T, const double* p, double* out) {
  out[0] = fma(T[0], p[0], fma(T[1], p[1], fma(T[2], p[2], T[3])));
  out[1] = fma(T[4], p[0], fma(T[5], p[1], fma(T[6], p[2], T[7])));
  out[2] = fma(T[8], p[0], fma(T[9], p[1], fma(T[10], p[2], T[11])));
}

// floor((x - o) / h) as a double: non-decreasing in x, which is all the search below relies on
BSG_ICP_FN double icp_cell_f(double x, double o, double h) {
  BSG_ICP_EXACT
  return floor((x - o) / h);
}
BSG_ICP_FN int icp_clampi(double f, int n) { return f < 0.0 ? 0 : (f > (double)(n - 1) ? n - 1 : (int)f); }
// the cell (index into the call's cell array) of a target point; a point of the bounding box is never clamped
BSG_ICP_FN int icp_cell_of(const IcpGrid& g, const double* q) {
  const int cx = icp_clampi(icp_cell_f(q[0], g.o[0], g.h), g.n[0]);
  const int cy = icp_clampi(icp_cell_f(q[1], g.o[1], g.h), g.n[1]);
  const int cz = icp_clampi(icp_cell_f(q[2], g.o[2], g.h), g.n[2]);
  return g.cell0 + (cz * g.n[1] + cy) * g.n[0] + cx;
}
// cells per axis of a bounding box [lo, hi]; as doubles, so that the product can be compared with the cap before it is an int
BSG_ICP_FN double icp_axis_cells(double lo, double hi, double h) { return icp_cell_f(hi, lo, h) + 1.0; }

// The cells [lo, hi] of one axis that can hold a target within h of s; false: none.  A kept target has a COMPUTED d^2 <= h^2, hence
// |q - s| <= h up to rounding; the interval is widened by 4 ulp of (|s| + h) on each side, which covers that rounding and the one of
// s -+ h itself, and icp_cell_f is monotone.  So every target that can be kept lies in the cells searched: the search is exact, not
// approximate.  (In all but such rounding cases the interval is the three cells of the usual 3 x 3 x 3 neighbourhood.)
BSG_ICP_FN bool icp_axis_range(double s, double o, double h, int n, int* lo, int* hi) {
  BSG_ICP_EXACT
  const double pad = 4.0 * kIcpEps * (fabs(s) + h);
  const double fl = icp_cell_f(s - h - pad, o, h), fh = icp_cell_f(s + h + pad, o, h);
  if (!(fh >= 0.0) || !(fl <= (double)(n - 1))) return false;
  *lo = icp_clampi(fl, n);
  *hi = icp_clampi(fh, n);
  return true;
}

// The nearest target of s among those with d^2 <= h2, squared distance in FP64, ties to the lowest target index: (d^2, index) is
// compared lexicographically, so neither the order in which a cell was filled nor the order in which candidates are visited can
// change the answer.  rec: 4 doubles per sorted target (x, y, z, index within its cloud).  A row of cells is contiguous in the sorted
// records: 9 ranges, not 27 cells.  icp_nearest_part visits every nsub-th candidate of each range from the sub-th on (the kernel
// gives a point to nsub neighbouring lanes and merges their bests with icp_better) and applies no threshold; *best stays +infinity
// when it saw nothing.
BSG_ICP_FN bool icp_better(double d2, double idx, double best, double bidx) { return d2 < best || (d2 == best && idx < bidx); }
BSG_ICP_FN void icp_nearest_part(const IcpGrid& g, const int* cell_end, const double* rec, const double* s, int sub, int nsub, double* best_out,
                                 double* bidx_out, double* q_out) {
  BSG_ICP_EXACT
  double best = std::numeric_limits<double>::infinity(), bidx = std::numeric_limits<double>::infinity(), bx = 0.0, by = 0.0, bz = 0.0;
  int x0 = 0, x1 = -1, y0 = 0, y1 = -1, z0 = 0, z1 = -1;
  const bool any = g.n[0] > 0 && g.n[1] > 0 && g.n[2] > 0 && icp_axis_range(s[0], g.o[0], g.h, g.n[0], &x0, &x1) &&
                   icp_axis_range(s[1], g.o[1], g.h, g.n[1], &y0, &y1) && icp_axis_range(s[2], g.o[2], g.h, g.n[2], &z0, &z1);
  if (any) {
    for (int z = z0; z <= z1; ++z) {
      for (int y = y0; y <= y1; ++y) {
        const int row = g.cell0 + (z * g.n[1] + y) * g.n[0];
        const int c0 = row + x0, c1 = row + x1;
        const int b = c0 > 0 ? cell_end[c0 - 1] : 0, e = cell_end[c1];
        for (int p = b + sub; p < e; p += nsub) {
          const double* r = rec + 4 * (size_t)p;
          const double dx = r[0] - s[0], dy = r[1] - s[1], dz = r[2] - s[2];
          const double d2 = dx * dx + dy * dy + dz * dz;
          const bool better = icp_better(d2, r[3], best, bidx);
          best = better ? d2 : best; bidx = better ? r[3] : bidx;
          bx = better ? r[0] : bx; by = better ? r[1] : by; bz = better ? r[2] : bz;
        }
      }
    }
  }
  *best_out = best; *bidx_out = bidx;
  q_out[0] = bx; q_out[1] = by; q_out[2] = bz;
}
BSG_ICP_FN bool icp_nearest(const IcpGrid& g, const int* cell_end, const double* rec, const double* s, double h2, double* d2_out,
                            double* q_out, double* idx_out) {
  icp_nearest_part(g, cell_end, rec, s, 0, 1, d2_out, idx_out, q_out);
  return *d2_out <= h2;
}

// The terms of one source point under T from s = T S_i and its correspondence q at squared distance d2 — zeros when it has none
BSG_ICP_FN void icp_record(bool kept, const double* s, const double* q, double d2, double* r) {
  BSG_ICP_EXACT
  r[0] = kept ? 1.0 : 0.0;
  r[1] = kept ? s[0] : 0.0; r[2] = kept ? s[1] : 0.0; r[3] = kept ? s[2] : 0.0;
  r[4] = kept ? q[0] : 0.0; r[5] = kept ? q[1] : 0.0; r[6] = kept ? q[2] : 0.0;
  r[7] = kept ? s[0] * q[0] : 0.0; r[8] = kept ? s[0] * q[1] : 0.0; r[9] = kept ? s[0] * q[2] : 0.0;
  r[10] = kept ? s[1] * q[0] : 0.0; r[11] = kept ? s[1] * q[1] : 0.0; r[12] = kept ? s[1] * q[2] : 0.0;
  r[13] = kept ? s[2] * q[0] : 0.0; r[14] = kept ? s[2] * q[1] : 0.0; r[15] = kept ? s[2] * q[2] : 0.0;
  r[16] = kept ? d2 : 0.0;
}
BSG_ICP_FN void icp_point_record(const double* T, const double* S, const IcpGrid& g, const int* cell_end, const double* rec, double h2,
                                 double* r) {
  double s[3], q[3], d2, idx;
  icp_apply(T, S, s);
  const bool kept = icp_nearest(g, cell_end, rec, s, h2, &d2, q, &idx);
  icp_record(kept, s, q, d2, r);
}

// ---- the 3 x 3 singular value decomposition: one-sided Jacobi (Hestenes), in registers ---------------------------------------------------
// One rotation of the columns P, Q of a (and of v) that makes them orthogonal; false: they already are, to rounding.
template <int P, int Q>
BSG_ICP_FN bool icp_jacobi(double a[3][3], double v[3][3]) {
  BSG_ICP_EXACT
  const double alpha = a[0][P] * a[0][P] + a[1][P] * a[1][P] + a[2][P] * a[2][P];
  const double beta = a[0][Q] * a[0][Q] + a[1][Q] * a[1][Q] + a[2][Q] * a[2][Q];
  const double gamma = a[0][P] * a[0][Q] + a[1][P] * a[1][Q] + a[2][P] * a[2][Q];
  if (!(fabs(gamma) > kIcpEps * sqrt(alpha * beta))) return false;
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
BSG_ICP_FN void icp_order(double* sig, double a[3][3], double v[3][3]) {
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
BSG_ICP_FN void icp_kabsch_rotation(const double* H, double* R) {
  BSG_ICP_EXACT
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
BSG_ICP_FN int icp_step(const double* sum, int k, const IcpParams& P, double* T, double* mse_prev, double* mse_out, int* n_corr) {
  BSG_ICP_EXACT
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
BSG_ICP_FN int icp_iterations(int status, int k) { return status == ICP_TOO_FEW_CORRESPONDENCES ? k - 1 : k; }

// out = inv(T) Tinit (MatchScans' T_LIDARREF_LIDARTGT = InvertTransform(T_RefEst_Ref) * T_LidarRefEst_LidarTgt), all row-major 3 x 4
BSG_ICP_FN void icp_inverse_times(const double* T, const double* Ti, double* out) {
  BSG_ICP_EXACT
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) out[4 * i + j] = T[i] * Ti[j] + T[4 + i] * Ti[4 + j] + T[8 + i] * Ti[8 + j];
    out[4 * i + 3] = out[4 * i + 3] - (T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11]);
  }
}

// ---- one pair on one core (host) ---------------------------------------------------------------------------------------------------------
// lane 0's value of a shuffle-down reduction over the 64 values v[0], v[stride], ...: offsets 32, 16, .., 1
inline double icp_wave_tree(double* v, int stride) {
  BSG_ICP_EXACT
  for (int off = kIcpWave / 2; off >= 1; off /= 2)
    for (int i = 0; i < off; ++i) v[i * stride] = v[i * stride] + v[(i + off) * stride];
  return v[0];
}

struct IcpSerialGrid {
  IcpGrid g;
  std::vector<int> cell_end;
  std::vector<double> rec;
};
// The grid of one cloud (already in the frame it is searched in) by a counting sort; false: more than max_cells cells.
inline bool icp_grid_build_serial(int n, const double* q, double h, double max_cells, IcpSerialGrid* G) {
  IcpGrid& g = G->g;
  g.h = h; g.cell0 = 0;
  for (int a = 0; a < 3; ++a) { g.o[a] = 0.0; g.n[a] = 0; }
  G->cell_end.clear(); G->rec.assign(4 * (size_t)n, 0.0);
  if (n == 0) return true;
  double hi[3];
  for (int a = 0; a < 3; ++a) g.o[a] = hi[a] = q[a];
  for (int i = 1; i < n; ++i)
    for (int a = 0; a < 3; ++a) { g.o[a] = q[3 * i + a] < g.o[a] ? q[3 * i + a] : g.o[a]; hi[a] = q[3 * i + a] > hi[a] ? q[3 * i + a] : hi[a]; }
  const double nx = icp_axis_cells(g.o[0], hi[0], h), ny = icp_axis_cells(g.o[1], hi[1], h), nz = icp_axis_cells(g.o[2], hi[2], h);
  if (!(nx * ny * nz <= max_cells)) return false;
  g.n[0] = (int)nx; g.n[1] = (int)ny; g.n[2] = (int)nz;
  std::vector<int>& ce = G->cell_end;
  ce.assign((size_t)(g.n[0] * g.n[1] * g.n[2]), 0);
  for (int i = 0; i < n; ++i) ++ce[icp_cell_of(g, q + 3 * i)];
  int run = 0;
  for (int& c : ce) { const int k = c; c = run; run += k; }      // starts; the scatter below turns them into ends
  for (int i = 0; i < n; ++i) {
    double* r = &G->rec[4 * (size_t)ce[icp_cell_of(g, q + 3 * i)]++];
    r[0] = q[3 * i]; r[1] = q[3 * i + 1]; r[2] = q[3 * i + 2]; r[3] = (double)i;
  }
  return true;
}

// bsgpu_register_scans for one pair.  false: the grid would exceed max_cells (the entry point's BSGPU_ERR_UNSUPPORTED).
inline bool icp_register_serial(int n_src, const double* S, int n_tgt, const double* Q, const double* T_init, double max_corr,
                                const IcpParams& P, double max_cells, double* T, double* T_ref_tgt, double* mse, int* n_corr,
                                int* n_iters, int* status) {
  BSG_ICP_EXACT
  static const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const double* Ti = T_init ? T_init : eye;
  std::vector<double> tq(3 * (size_t)n_tgt);
  for (int i = 0; i < n_tgt; ++i) icp_apply(Ti, Q + 3 * i, &tq[3 * (size_t)i]);
  IcpSerialGrid G;
  if (!icp_grid_build_serial(n_tgt, tq.data(), max_corr, max_cells, &G)) return false;
  const double h2 = max_corr * max_corr;
  for (int i = 0; i < 12; ++i) T[i] = eye[i];
  double mse_prev = std::numeric_limits<double>::infinity();
  const int n_chunks = (n_src + kIcpChunk - 1) / kIcpChunk;
  std::vector<double> lanes((size_t)kIcpChunk * kIcpRec);
  *status = ICP_NOT_CONVERGED; *n_iters = 0; *n_corr = 0; *mse = 0.0;
  for (int k = 1; *status == ICP_NOT_CONVERGED; ++k) {
    double sum[kIcpRec];
    for (int t = 0; t < kIcpRec; ++t) sum[t] = 0.0;
    for (int c = 0; c < n_chunks; ++c) {
      for (int l = 0; l < kIcpChunk; ++l) {
        double* r = &lanes[(size_t)l * kIcpRec];
        const int i = c * kIcpChunk + l;
        if (i < n_src) icp_point_record(T, S + 3 * (size_t)i, G.g, G.cell_end.data(), G.rec.data(), h2, r);
        else for (int t = 0; t < kIcpRec; ++t) r[t] = 0.0;
      }
      for (int t = 0; t < kIcpRec; ++t) {
        double part = 0.0;
        for (int w = 0; w < kIcpChunk / kIcpWave; ++w) part = part + icp_wave_tree(&lanes[(size_t)w * kIcpWave * kIcpRec + t], kIcpRec);
        sum[t] = sum[t] + part;
      }
    }
    *status = icp_step(sum, k, P, T, &mse_prev, mse, n_corr);
    *n_iters = icp_iterations(*status, k);
  }
  if (T_ref_tgt) icp_inverse_times(T, Ti, T_ref_tgt);
  return true;
}

}  // namespace bsg
