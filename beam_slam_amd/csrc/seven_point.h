// Seven-point RANSAC two-view bootstrap (bsgpu_relative_pose_ransac): steps 1 and 2 of bs_models::vision::ComputePathWithVision
// (bs_models/src/lib/vision/utils.cpp:44-94) — [EXT] beam_cv::RelativePoseEstimator::RANSACEstimator(cam, cam, first, last,
// SEVENPOINT, 100), [EXT] beam_cv::Triangulation::TriangulatePoints and the 10 px / 80 % gate.  libbeam is not part of the reference
// checkout: the semantics restated here are RECALLED, not verified (DESIGN.md "Relative-pose RANSAC").
//
// Host- and device-compilable, in the style of p3p.h: plain C++, nothing from HIP but the qualifiers; every loop over a small array
// has compile-time bounds and every index is a loop counter, so that the device copy lives in registers.  The solver is split so that
// relpose_kernel (k_relpose.hip) can give a sample to a group of lanes: sp7_models is the part all of them repeat, sp7_decompose is
// one hypothesis'.  sp7_solve and sp7_ransac_serial compose the same blocks serially: the contract's loop for one set, used by the
// CPU tests and the host stand-in and by nothing in the product at run time.
//
// The minimal solver:
//   1. the 7 epipolar rows x_last^T E x_first = 0 orthonormalised (Gram-Schmidt, twice), then two more orthonormal vectors from the
//      unit vectors with the largest residual: N1, N2 span the null space;
//   2. the pencil D + x V with (V, D) the one of (N1, N2), (N2, N1), ((N1 + N2) / sqrt 2, (N2 - N1) / sqrt 2) and its swap whose
//      det V is largest in magnitude: det(D + x V) = det D + x tr(adj D V) + x^2 tr(adj V D) + x^3 det V has a leading coefficient
//      that cannot vanish (a cubic form that is not zero has at most three zeros on the projective line, and four directions are
//      tried), so a root "at infinity" of one parametrisation is an ordinary root of the one chosen;
//   3. ALL real roots: an outer root by Newton from the far side of the outer stationary point, where the iteration is monotone,
//      the other two from the deflated quadratic, each polished on the cubic itself;
//   4. E = D + x V scaled to |E|_F = 1, largest-magnitude entry positive; ascending E[0].
// Every E gives four poses T_last_first = [R|t] from E = U diag(s) V^T (sp7_decompose), in the canonical order of the contract.
// A match is scored by triangulating it (sp7_triangulate: bsgpu_triangulate's DLT for the views [I|0] and [R|t], the 4 x 4 Gram
// matrix diagonalised by cyclic Jacobi with compile-time indices) and reprojecting the point into both images (sp7_inlier).
// (bsgpu_triangulate's definition, not its method: in the first camera's frame with a unit baseline A is well conditioned and the
// Gram matrix loses nothing that matters; bsgpu_triangulate works in world coordinates and takes the singular vector from A.)
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BSG_SP7_FN __host__ __device__ inline
#define BSG_SP7_UNROLL _Pragma("unroll")
#else
#define BSG_SP7_FN inline
#define BSG_SP7_UNROLL
#endif

namespace bsg {

constexpr int kSp7MaxSol = 3;    // essential matrices of one sample
constexpr int kSp7MaxHyp = 12;   // poses of one sample: 4 per matrix
enum { SP7_OK = 0, SP7_TOO_FEW = 1, SP7_NO_MODEL = 2 };   // BSGPU_RANSAC_* of include/bsgpu.h

// ---- sampler: the contract's counter-based splitmix64 stream and redraw rule, seven indices -------------------------------------------
BSG_SP7_FN int sp7_draw(uint64_t& state, int n) {
  state += 0x9E3779B97F4A7C15ull;
  uint64_t z = state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (int)(z % (uint64_t)n);
}
// n >= 7
BSG_SP7_FN void sp7_sample(uint64_t seed, uint64_t set_index, uint64_t sample_index, int n, int* idx /* 7 */) {
  uint64_t state = seed ^ (set_index * 0x9E3779B97F4A7C15ull) ^ (sample_index * 0xBF58476D1CE4E5B9ull);
  BSG_SP7_UNROLL
  for (int k = 0; k < 7; ++k) idx[k] = -1;
  BSG_SP7_UNROLL
  for (int k = 0; k < 7; ++k) {
    int i;
    bool dup;
    do {
      i = sp7_draw(state, n);
      dup = false;
      BSG_SP7_UNROLL
      for (int j = 0; j < 7; ++j) dup = dup || (j < k && idx[j] == i);
    } while (dup);
    idx[k] = i;
  }
}

BSG_SP7_FN double sp7_pixel(double v, int truncate) { return truncate ? trunc(v) : v; }
// p3p_update_niters' rule with exponent 7; prob outside (0, 1) (the contract's prob == 0): no early termination
BSG_SP7_FN int sp7_update_niters(double p, double ep, int niters) {
  if (!(p > 0.0 && p < 1.0)) return niters;
  const double num = log(1.0 - p), q = 1.0 - ep;
  const double q2 = q * q, q4 = q2 * q2;
  const double t = 1.0 - q4 * q2 * q;
  const double den = t > 0.0 ? log(t) : -INFINITY;
  if (den >= 0.0 || -num >= (double)niters * (-den)) return niters;
  return (int)round(num / den);
}

// ---- 3 x 3 helpers ------------------------------------------------------------------------------------------------------------------------
BSG_SP7_FN void sp7_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
BSG_SP7_FN double sp7_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
BSG_SP7_FN double sp7_det(const double* A) {
  return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}
// tr(adj(A) B): the derivative of det at A in the direction B
BSG_SP7_FN double sp7_tr_adj(const double* A, const double* B) {
  return (A[4] * A[8] - A[5] * A[7]) * B[0] + (A[5] * A[6] - A[3] * A[8]) * B[1] + (A[3] * A[7] - A[4] * A[6]) * B[2] +
         (A[2] * A[7] - A[1] * A[8]) * B[3] + (A[0] * A[8] - A[2] * A[6]) * B[4] + (A[1] * A[6] - A[0] * A[7]) * B[5] +
         (A[1] * A[5] - A[2] * A[4]) * B[6] + (A[2] * A[3] - A[0] * A[5]) * B[7] + (A[0] * A[4] - A[1] * A[3]) * B[8];
}
BSG_SP7_FN double sp7_dot9(const double* a, const double* b) {
  double s = 0.0;
  BSG_SP7_UNROLL
  for (int j = 0; j < 9; ++j) s += a[j] * b[j];
  return s;
}

// ---- the cubic: all real roots of x^3 + b x^2 + c x + d; returns 1 or 3 --------------------------------------------------------------------
BSG_SP7_FN double sp7_newton(double x, double b, double c, double d, int steps) {
  for (int it = 0; it < steps; ++it) {
    const double f = ((x + b) * x + c) * x + d, df = (3.0 * x + 2.0 * b) * x + c;
    if (f == 0.0 || !(fabs(df) > 0.0)) break;
    const double xn = x - f / df;
    if (xn == x || !std::isfinite(xn)) break;
    const bool done = fabs(xn - x) <= 4e-16 * fabs(xn);
    x = xn;
    if (done) break;
  }
  return x;
}
BSG_SP7_FN int sp7_cubic_roots(double b, double c, double d, double* r /* 3 */) {
  // an outer root.  With two stationary points t1 < t2 (local maximum, local minimum): a root lies left of t1 iff f(t1) > 0, and the
  // zero of the parabola osculating there is left of it, where f is concave and rising; otherwise one lies right of t2, mirrored.
  double x;
  const double disc = b * b - 3.0 * c;
  if (disc > 0.0) {
    const double sq = sqrt(disc), t1 = (-b - sq) / 3.0, t2 = (-b + sq) / 3.0;
    const double h1 = ((t1 + b) * t1 + c) * t1 + d;
    if (h1 > 0.0) {
      x = t1 - sqrt(h1 / sq);
    } else {
      const double h2 = ((t2 + b) * t2 + c) * t2 + d;
      x = t2 + sqrt(fmax(-h2, 0.0) / sq);
    }
  } else {
    x = -b / 3.0;   // monotone cubic: from the inflection point the first step lands on the root's convex side
  }
  const double r0 = sp7_newton(x, b, c, d, 60);
  r[0] = r0; r[1] = r[2] = NAN;
  // x^3 + b x^2 + c x + d = (x - r0) (x^2 + p x + q)
  const double p = b + r0, q = c + p * r0;
  const double dq = p * p - 4.0 * q;
  if (!(dq >= 0.0) || !std::isfinite(r0)) return 1;
  const double sq = sqrt(dq), qq = -0.5 * (p + (p < 0.0 ? -sq : sq));
  const double ra = qq, rb = qq != 0.0 ? q / qq : 0.0;
  r[1] = sp7_newton(ra, b, c, d, 8);
  r[2] = sp7_newton(rb, b, c, d, 8);
  return 3;
}

// ---- the essential matrices of a sample --------------------------------------------------------------------------------------------------
// |E|_F = 1, largest-magnitude entry positive
BSG_SP7_FN void sp7_normalize_E(double* E) {
  double big = E[0];
  BSG_SP7_UNROLL
  for (int j = 1; j < 9; ++j) big = fabs(E[j]) > fabs(big) ? E[j] : big;
  const double s = (big < 0.0 ? -1.0 : 1.0) / sqrt(sp7_dot9(E, E));
  BSG_SP7_UNROLL
  for (int j = 0; j < 9; ++j) E[j] *= s;
}

// m: 7 x (x_first, y_first, x_last, y_last), normalised coordinates.  E: up to 3 x 9, row-major, ascending E[0].  Returns 0, 1 or 3.
BSG_SP7_FN int sp7_models(const double* m, double* E) {
  double Q[9][9];
  bool ok = true;
  BSG_SP7_UNROLL
  for (int i = 0; i < 9; ++i) {
    double n0 = 1.0;
    if (i < 7) {
      const double x1 = m[4 * i], y1 = m[4 * i + 1], x2 = m[4 * i + 2], y2 = m[4 * i + 3];
      Q[i][0] = x2 * x1; Q[i][1] = x2 * y1; Q[i][2] = x2;
      Q[i][3] = y2 * x1; Q[i][4] = y2 * y1; Q[i][5] = y2;
      Q[i][6] = x1;      Q[i][7] = y1;      Q[i][8] = 1.0;
      n0 = sqrt(sp7_dot9(Q[i], Q[i]));
    } else {
      // the unit vector that the rows so far span least
      int bj = 0;
      double best = -1.0;
      BSG_SP7_UNROLL
      for (int j = 0; j < 9; ++j) {
        double res = 1.0;
        BSG_SP7_UNROLL
        for (int q = 0; q < 9; ++q) res -= q < i ? Q[q][j] * Q[q][j] : 0.0;
        if (res > best) { best = res; bj = j; }
      }
      BSG_SP7_UNROLL
      for (int j = 0; j < 9; ++j) Q[i][j] = j == bj ? 1.0 : 0.0;
    }
    BSG_SP7_UNROLL
    for (int pass = 0; pass < 2; ++pass) {
      BSG_SP7_UNROLL
      for (int q = 0; q < 9; ++q) {
        if (q < i) {
          const double dd = sp7_dot9(Q[q], Q[i]);
          BSG_SP7_UNROLL
          for (int j = 0; j < 9; ++j) Q[i][j] -= dd * Q[q][j];
        }
      }
    }
    const double nn = sqrt(sp7_dot9(Q[i], Q[i]));
    ok = ok && nn > 1e-10 * n0;
    const double inv = 1.0 / nn;
    BSG_SP7_UNROLL
    for (int j = 0; j < 9; ++j) Q[i][j] *= inv;
  }
  // the pencil's direction V: the largest |det| of four
  const double h = 0.70710678118654752440;
  double S[9], Dm[9];
  BSG_SP7_UNROLL
  for (int j = 0; j < 9; ++j) { S[j] = h * (Q[7][j] + Q[8][j]); Dm[j] = h * (Q[8][j] - Q[7][j]); }
  const double d0 = fabs(sp7_det(Q[7])), d1 = fabs(sp7_det(Q[8])), d2 = fabs(sp7_det(S)), d3 = fabs(sp7_det(Dm));
  const int pick = (d0 >= d1 && d0 >= d2 && d0 >= d3) ? 0 : (d1 >= d2 && d1 >= d3) ? 1 : d2 >= d3 ? 2 : 3;
  double V[9], D[9];
  BSG_SP7_UNROLL
  for (int j = 0; j < 9; ++j) {
    V[j] = pick == 0 ? Q[7][j] : pick == 1 ? Q[8][j] : pick == 2 ? S[j] : Dm[j];
    D[j] = pick == 0 ? Q[8][j] : pick == 1 ? Q[7][j] : pick == 2 ? Dm[j] : S[j];
  }
  const double k0 = sp7_det(D), k1 = sp7_tr_adj(D, V), k2 = sp7_tr_adj(V, D), k3 = sp7_det(V);
  if (!ok || !(fabs(k3) > 0.0) || !std::isfinite(k3)) return 0;
  double r[3];
  const int nr = sp7_cubic_roots(k2 / k3, k1 / k3, k0 / k3, r);
  if (!std::isfinite(r[0])) return 0;
  BSG_SP7_UNROLL
  for (int k = 0; k < 3; ++k) {
    BSG_SP7_UNROLL
    for (int j = 0; j < 9; ++j) E[9 * k + j] = D[j] + (k < nr ? r[k] : r[0]) * V[j];
    sp7_normalize_E(E + 9 * k);
  }
  if (nr == 3) {   // ascending first entry: three compare-exchanges
    BSG_SP7_UNROLL
    for (int step = 0; step < 3; ++step) {
      const int a = step == 1 ? 1 : 0, bb = step == 1 ? 2 : 1;
      if (E[9 * bb] < E[9 * a]) {
        BSG_SP7_UNROLL
        for (int j = 0; j < 9; ++j) { const double t = E[9 * a + j]; E[9 * a + j] = E[9 * bb + j]; E[9 * bb + j] = t; }
      }
    }
  }
  return nr;
}

// ---- the four poses of an essential matrix -------------------------------------------------------------------------------------------------
// E = U diag(s) V^T with U, V proper rotations; R in {U W V^T, U W^T V^T}, t = +-u3.  dec 0..3: (R_a, +t), (R_a, -t), (R_b, +t),
// (R_b, -t); R_a has the larger trace, +t its largest-magnitude component positive.  T: 12, row-major [R|t], |t| = 1.
// Written without an SVD routine: v3 is the largest cross product of two rows of E, (v1, v2) diagonalise E^T E inside the plane
// orthogonal to it (one Jacobi rotation), u_i = E v_i / |E v_i|, u3 = u1 x u2.  Then U W V^T = u3 v3^T + (u2 v1^T - u1 v2^T) and
// U W^T V^T = u3 v3^T - (u2 v1^T - u1 v2^T): the pair does not depend on the signs or the order the SVD leaves open.
BSG_SP7_FN void sp7_decompose(const double* E, int dec, double* T) {
  double c01[3], c02[3], c12[3];
  sp7_cross(E, E + 3, c01); sp7_cross(E, E + 6, c02); sp7_cross(E + 3, E + 6, c12);
  const double m0 = sp7_dot(c01, c01), m1 = sp7_dot(c02, c02), m2 = sp7_dot(c12, c12);
  const bool u0 = m0 >= m1 && m0 >= m2, u1s = !u0 && m1 >= m2;
  const double vn = 1.0 / sqrt(u0 ? m0 : u1s ? m1 : m2);
  double v3[3], a[3], b[3];
  BSG_SP7_UNROLL
  for (int i = 0; i < 3; ++i) v3[i] = (u0 ? c01[i] : u1s ? c02[i] : c12[i]) * vn;
  const double n0 = sp7_dot(E, E), n1 = sp7_dot(E + 3, E + 3), n2 = sp7_dot(E + 6, E + 6);
  const bool w0 = n0 >= n1 && n0 >= n2, w1 = !w0 && n1 >= n2;
  BSG_SP7_UNROLL
  for (int i = 0; i < 3; ++i) a[i] = w0 ? E[i] : w1 ? E[3 + i] : E[6 + i];
  const double av = sp7_dot(a, v3);
  BSG_SP7_UNROLL
  for (int i = 0; i < 3; ++i) a[i] -= av * v3[i];
  const double an = 1.0 / sqrt(sp7_dot(a, a));
  BSG_SP7_UNROLL
  for (int i = 0; i < 3; ++i) a[i] *= an;
  sp7_cross(v3, a, b);
  double Ea[3], Eb[3];
  BSG_SP7_UNROLL
  for (int i = 0; i < 3; ++i) { Ea[i] = sp7_dot(E + 3 * i, a); Eb[i] = sp7_dot(E + 3 * i, b); }
  const double gp = sp7_dot(Ea, Ea), gq = sp7_dot(Ea, Eb), gr = sp7_dot(Eb, Eb);
  double cs = 1.0, sn = 0.0;
  if (gq != 0.0) {
    const double theta = (gr - gp) / (2.0 * gq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    cs = 1.0 / sqrt(t * t + 1.0); sn = t * cs;
  }
  double v1[3], v2[3], u1[3], u2[3], u3[3];
  BSG_SP7_UNROLL
  for (int i = 0; i < 3; ++i) {
    v1[i] = cs * a[i] - sn * b[i]; v2[i] = sn * a[i] + cs * b[i];
    u1[i] = cs * Ea[i] - sn * Eb[i]; u2[i] = sn * Ea[i] + cs * Eb[i];
  }
  const double s1 = 1.0 / sqrt(sp7_dot(u1, u1)), s2 = 1.0 / sqrt(sp7_dot(u2, u2));
  BSG_SP7_UNROLL
  for (int i = 0; i < 3; ++i) { u1[i] *= s1; u2[i] *= s2; }
  sp7_cross(u1, u2, u3);
  const double s3 = 1.0 / sqrt(sp7_dot(u3, u3));
  BSG_SP7_UNROLL
  for (int i = 0; i < 3; ++i) u3[i] *= s3;
  const double trM = (u2[0] * v1[0] - u1[0] * v2[0]) + (u2[1] * v1[1] - u1[1] * v2[1]) + (u2[2] * v1[2] - u1[2] * v2[2]);
  const double sg = ((trM >= 0.0) != ((dec & 2) != 0)) ? 1.0 : -1.0;
  double big = u3[0];
  big = fabs(u3[1]) > fabs(big) ? u3[1] : big;
  big = fabs(u3[2]) > fabs(big) ? u3[2] : big;
  const double st = ((big >= 0.0) != ((dec & 1) != 0)) ? 1.0 : -1.0;
  BSG_SP7_UNROLL
  for (int i = 0; i < 3; ++i) {
    BSG_SP7_UNROLL
    for (int j = 0; j < 3; ++j) T[4 * i + j] = u3[i] * v3[j] + sg * (u2[i] * v1[j] - u1[i] * v2[j]);
    T[4 * i + 3] = st * u3[i];
  }
}

// ---- two-view triangulation and the inlier test ----------------------------------------------------------------------------------------------
template <int P, int Q>
BSG_SP7_FN void sp7_jacobi(double a[4][4], double v[4][4]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  BSG_SP7_UNROLL
  for (int k = 0; k < 4; ++k) {
    const double akp = a[k][P], akq = a[k][Q];
    a[k][P] = c * akp - s * akq; a[k][Q] = s * akp + c * akq;
  }
  BSG_SP7_UNROLL
  for (int k = 0; k < 4; ++k) {
    const double apk = a[P][k], aqk = a[Q][k];
    a[P][k] = c * apk - s * aqk; a[Q][k] = s * apk + c * aqk;
  }
  a[P][Q] = a[Q][P] = 0.0;
  BSG_SP7_UNROLL
  for (int k = 0; k < 4; ++k) {
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq; v[k][Q] = s * vkp + c * vkq;
  }
}

// bsgpu_triangulate's definition (what is computed; triangulate_core.h computes it without the Gram matrix, which far from the
// world origin squares a large condition number — here the frame is the first camera's and the baseline 1) for the views [I|0] and
// T = [R|t]: unit bearings of the normalised coordinates (x1, y1), (x2, y2),
// four DLT rows, the right singular vector of the smallest singular value (the eigenvector of the smallest eigenvalue of the Gram
// matrix), de-homogenised.  false: the point at infinity (homogeneous w == 0, bsgpu_triangulate's status 5); P is then NaN.
// The sweeps stop once the off-diagonal mass is below 1e-20 of the trace: Jacobi converges quadratically, so the eigenvectors are
// then exact to the last bit that the gap between the eigenvalues allows.
BSG_SP7_FN bool sp7_triangulate(const double* T, double x1, double y1, double x2, double y2, double* P) {
  const double i1 = 1.0 / sqrt(x1 * x1 + y1 * y1 + 1.0), i2 = 1.0 / sqrt(x2 * x2 + y2 * y2 + 1.0);
  const double mx = x1 * i1, my = y1 * i1, mz = i1, nx = x2 * i2, ny = y2 * i2, nz = i2;
  double r[4][4];
  r[0][0] = -mz; r[0][1] = 0.0; r[0][2] = mx; r[0][3] = 0.0;
  r[1][0] = 0.0; r[1][1] = -mz; r[1][2] = my; r[1][3] = 0.0;
  BSG_SP7_UNROLL
  for (int k = 0; k < 4; ++k) {
    r[2][k] = nx * T[8 + k] - nz * T[k];
    r[3][k] = ny * T[8 + k] - nz * T[4 + k];
  }
  double a[4][4], v[4][4];
  BSG_SP7_UNROLL
  for (int i = 0; i < 4; ++i) {
    BSG_SP7_UNROLL
    for (int j = 0; j < 4; ++j) {
      a[i][j] = r[0][i] * r[0][j] + r[1][i] * r[1][j] + r[2][i] * r[2][j] + r[3][i] * r[3][j];
      v[i][j] = i == j ? 1.0 : 0.0;
    }
  }
  const double tiny = 1e-20 * (a[0][0] + a[1][1] + a[2][2] + a[3][3]);
  for (int sweep = 0; sweep < 10; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
    if (!(off > tiny)) break;
    sp7_jacobi<0, 1>(a, v); sp7_jacobi<0, 2>(a, v); sp7_jacobi<0, 3>(a, v);
    sp7_jacobi<1, 2>(a, v); sp7_jacobi<1, 3>(a, v); sp7_jacobi<2, 3>(a, v);
  }
  double best = a[0][0];
  double h[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
  BSG_SP7_UNROLL
  for (int j = 1; j < 4; ++j) {
    const bool lt = a[j][j] < best;
    best = lt ? a[j][j] : best;
    BSG_SP7_UNROLL
    for (int k = 0; k < 4; ++k) h[k] = lt ? v[k][j] : h[k];
  }
  if (h[3] == 0.0 || !(h[3] == h[3])) { P[0] = P[1] = P[2] = NAN; return false; }
  P[0] = h[0] / h[3]; P[1] = h[1] / h[3]; P[2] = h[2] / h[3];
  return true;
}

// K = (fx, fy, cx, cy); (u1, v1) / (u2, v2): the pixels of the first / last image; P in the first camera's frame.  Inlier iff P is
// finite, its depth is positive in both cameras and the squared reprojection distance is below thr2 in BOTH images.  Every
// multiply-add is an explicit fma so that all inlined copies round alike.
BSG_SP7_FN bool sp7_inlier(const double* T, const double* K, double u1, double v1, double u2, double v2, const double* P, double thr2) {
  const double X = P[0], Y = P[1], Z = P[2];
  const double x = fma(T[0], X, fma(T[1], Y, fma(T[2], Z, T[3])));
  const double y = fma(T[4], X, fma(T[5], Y, fma(T[6], Z, T[7])));
  const double z = fma(T[8], X, fma(T[9], Y, fma(T[10], Z, T[11])));
  const double ax = fma(K[0], X / Z, K[2]) - u1, ay = fma(K[1], Y / Z, K[3]) - v1;
  const double bx = fma(K[0], x / z, K[2]) - u2, by = fma(K[1], y / z, K[3]) - v2;
  const bool fin = std::isfinite(X) && std::isfinite(Y) && std::isfinite(Z);
  return fin && Z > 0.0 && z > 0.0 && fma(ax, ax, ay * ay) < thr2 && fma(bx, bx, by * by) < thr2;
}

// one match under one pose: the point (NaN at infinity) and whether it is an inlier at thr2
BSG_SP7_FN bool sp7_score(const double* T, const double* K, double u1, double v1, double u2, double v2, double thr2, double* P) {
  sp7_triangulate(T, (u1 - K[2]) / K[0], (v1 - K[3]) / K[1], (u2 - K[2]) / K[0], (v2 - K[3]) / K[1], P);
  return sp7_inlier(T, K, u1, v1, u2, v2, P, thr2);
}

// ---- T_WORLD_BASELINK of the two images, world = first camera (AddCameraPose, utils.cpp:108-109) --------------------------------------------
// the rotation R (row-major) as a unit quaternion wxyz with w >= 0
BSG_SP7_FN void sp7_quat(const double* R, double* q) {
  const double tr = R[0] + R[4] + R[8];
  double w, x, y, z;
  if (tr > 0.0) {
    const double s = 2.0 * sqrt(1.0 + tr);
    w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
    w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
    w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s;
  } else {
    const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
    w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s;
  }
  const double nn = (w < 0.0 ? -1.0 : 1.0) / sqrt(w * w + x * x + y * y + z * z);
  q[0] = w * nn; q[1] = x * nn; q[2] = y * nn; q[3] = z * nn;
}
// q: 2 x 4, p: 2 x 3: the first image's pose is T_cam_baselink, the last image's T_last_first^-1 T_cam_baselink
BSG_SP7_FN void sp7_baselink_poses(const double* T, const double* R_cb, const double* t_cb, double* q, double* p) {
  double R[9];
  sp7_quat(R_cb, q);
  BSG_SP7_UNROLL
  for (int i = 0; i < 3; ++i) {
    p[i] = t_cb[i];
    BSG_SP7_UNROLL
    for (int j = 0; j < 3; ++j) R[3 * i + j] = T[i] * R_cb[j] + T[4 + i] * R_cb[3 + j] + T[8 + i] * R_cb[6 + j];
    p[3 + i] = T[i] * (t_cb[0] - T[3]) + T[4 + i] * (t_cb[1] - T[7]) + T[8 + i] * (t_cb[2] - T[11]);
  }
  sp7_quat(R, q + 4);
}

// ---- the serial compositions -------------------------------------------------------------------------------------------------------------------
// m: 7 x (x_first, y_first, x_last, y_last) normalised; E: up to 3 x 9; T: 4 poses per E, 12 each; returns the number of E
inline int sp7_solve(const double* m, double* E, double* T) {
  const int ns = sp7_models(m, E);
  for (int k = 0; k < ns; ++k)
    for (int dec = 0; dec < 4; ++dec) sp7_decompose(E + 9 * k, dec, T + 12 * (4 * k + dec));
  return ns;
}

// The contract's loop for one set.  Outputs as bsgpu_relative_pose_ransac's for that set (T_out 12; points 3 per match).
inline void sp7_ransac_serial(int n, const double* px_first, const double* px_last, const double* K, double prob, double threshold_px,
                              int max_iters, uint64_t seed, uint64_t set_index, int truncate, double validate_px, double min_inlier_ratio,
                              uint8_t* mask, double* T_out, double* points, uint8_t* valid_mask, double* inlier_ratio, int* pair_valid,
                              int* n_inliers, int* n_iters, int* best_sample, int* status) {
  for (int i = 0; i < n; ++i) { mask[i] = 0; valid_mask[i] = 0; points[3 * i] = points[3 * i + 1] = points[3 * i + 2] = NAN; }
  for (int e = 0; e < 12; ++e) T_out[e] = NAN;
  for (int k = 0; k < 7; ++k) best_sample[k] = -1;
  *n_inliers = 0; *n_iters = 0; *inlier_ratio = NAN; *pair_valid = 0;
  if (n < 8) { *status = SP7_TOO_FEW; return; }
  *status = SP7_NO_MODEL;
  const double thr2 = threshold_px * threshold_px, val2 = validate_px * validate_px;
  auto pix = [&](const double* p, int i, int j) { return sp7_pixel(p[2 * i + j], truncate); };
  int niters = max_iters, best = 0, s = 0;
  for (; s < niters; ++s) {
    int idx[7];
    double m[28], E[9 * kSp7MaxSol], T[12 * kSp7MaxHyp];
    sp7_sample(seed, set_index, (uint64_t)s, n, idx);
    for (int k = 0; k < 7; ++k) {
      m[4 * k] = (pix(px_first, idx[k], 0) - K[2]) / K[0]; m[4 * k + 1] = (pix(px_first, idx[k], 1) - K[3]) / K[1];
      m[4 * k + 2] = (pix(px_last, idx[k], 0) - K[2]) / K[0]; m[4 * k + 3] = (pix(px_last, idx[k], 1) - K[3]) / K[1];
    }
    const int ns = sp7_solve(m, E, T);
    for (int h = 0; h < 4 * ns; ++h) {
      int good = 0;
      for (int i = 0; i < n; ++i) {
        double P[3];
        good += sp7_score(T + 12 * h, K, pix(px_first, i, 0), pix(px_first, i, 1), pix(px_last, i, 0), pix(px_last, i, 1), thr2, P) ? 1 : 0;
      }
      if (good > (best > 7 ? best : 7)) {
        best = good;
        for (int e = 0; e < 12; ++e) T_out[e] = T[12 * h + e];
        for (int k = 0; k < 7; ++k) best_sample[k] = idx[k];
        niters = sp7_update_niters(prob, (double)(n - good) / (double)n, niters);
      }
    }
  }
  *n_iters = s;
  if (best == 0) return;
  *status = SP7_OK;
  *n_inliers = best;
  int n_valid = 0;
  for (int i = 0; i < n; ++i) {
    const double u1 = pix(px_first, i, 0), v1 = pix(px_first, i, 1), u2 = pix(px_last, i, 0), v2 = pix(px_last, i, 1);
    mask[i] = sp7_score(T_out, K, u1, v1, u2, v2, thr2, points + 3 * i) ? 1 : 0;
    valid_mask[i] = sp7_inlier(T_out, K, u1, v1, u2, v2, points + 3 * i, val2) ? 1 : 0;
    n_valid += valid_mask[i];
  }
  *inlier_ratio = (double)n_valid / (double)n;
  *pair_valid = *inlier_ratio < min_inlier_ratio ? 0 : 1;
}

}  // namespace bsg
