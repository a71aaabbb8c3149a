// Five-point RANSAC track screening (bsgpu_essential_ransac): what VisualOdometry::AddMeasurementsToContainer
// (bs_models/src/visual_odometry.cpp:481-527) and SLAMInitialization (bs_models/src/slam_initialization.cpp:882-910) get from [EXT]
// cv::findEssentialMat(fp1, fp2, K, cv::RANSAC, prob, threshold, mask).  The semantics restated here are RECALLED from OpenCV 4
// (findEssentialMat / RANSACPointSetRegistrator); OpenCV is not part of the reference checkout and they could not be verified
// (DESIGN.md "Essential-matrix RANSAC").
//
// Host- and device-compilable, in the style of frame_lm.h: plain C++, nothing from HIP but the qualifiers.  Every building block
// works on caller-provided memory (LDS in ransac_kernel, k_ransac.hip; the stack in fpr_five_point), so the kernel can spread one
// sample's solve over a group of lanes — a constraint row, an interval of the root search, a root's back-substitution per lane —
// without a per-lane matrix in private memory.  fpr_five_point and fpr_ransac_serial compose the same blocks serially: the contract's
// loop for one set, used by the CPU tests and by nothing in the product at run time.
//
// The minimal solver (Nister 2004, in the elimination order of his section 3.2):
//   1. the 4-dimensional null space of the 5 x 9 epipolar matrix, as an orthonormal basis: E = x E1 + y E2 + z E3 + E4;
//   2. the ten cubic constraints det E = 0, 2 E E^T E - tr(E E^T) E = 0 in the 20 monomials of degree <= 3, columns ordered
//      x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1;
//   3. Gauss-Jordan with partial pivoting on the first ten columns, for each of the three choices of which free coordinate is z,
//      keeping the choice whose reduced rows have the smallest largest entry: the rows led by x^2z, x^2, y^2z, y^2, xyz, xy give
//      <x^2z> - z <x^2>, <y^2z> - z <y^2>, <xyz> - z <xy>: B(z) (x, y, 1)^T = 0 with B 3 x 3 of degrees (3, 3, 4) in z;
//   4. det B(z), degree 10: its real roots by derivative bracketing — the roots of p^(k+1) split the line into intervals each
//      holding at most one root of p^(k), found by a bracketed Newton iteration (bounded, deterministic work, no complex arithmetic);
//   5. per root (x, y) from the null vector of B(z), a few Gauss-Newton steps on the ten constraints themselves, E normalised to |E|_F = 1 with its largest-magnitude entry positive.
// Solutions of one sample are ordered by ascending E[0] so that the loop's "first strictly better" rule does not depend on how an
// implementation enumerates them.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BSG_FPR_FN __host__ __device__ inline
#else
#define BSG_FPR_FN inline
#endif

namespace bsg {

constexpr int kFprMaxSol = 10;
enum { FPR_OK = 0, FPR_TOO_FEW = 1, FPR_NO_MODEL = 2 };   // BSGPU_RANSAC_* of include/bsgpu.h
// workspace of one sample, in doubles: [Q 81 | R 60 | B 45 | D 66 | roots 2 x 12]
constexpr int kFprQ = 0, kFprR = 81, kFprB = 141, kFprD = 186, kFprRoots = 252, kFprWork = 276;
constexpr double kFprRootBound = 1e15;   // roots of det B(z) beyond it (solutions at infinity of the parametrisation) are dropped

// ---- sampler: counter-based splitmix64, addressable by (seed, set, sample) -----------------------------------------------------------
BSG_FPR_FN void fpr_sample(uint64_t seed, uint64_t set_index, uint64_t sample_index, int n, int* idx /* 5 */) {
  uint64_t state = seed ^ (set_index * 0x9E3779B97F4A7C15ull) ^ (sample_index * 0xBF58476D1CE4E5B9ull);
  for (int k = 0; k < 5; ++k) {
    for (;;) {
      state += 0x9E3779B97F4A7C15ull;
      uint64_t z = state;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      const int i = (int)(z % (uint64_t)n);
      bool dup = false;
      for (int j = 0; j < k; ++j) dup = dup || idx[j] == i;
      if (!dup) { idx[k] = i; break; }
    }
  }
}

// ---- normalisation, error, iteration update ---------------------------------------------------------------------------------------
// K = (fx, fy, cx, cy); m = (x1, y1, x2, y2): previous, current
BSG_FPR_FN void fpr_normalize(const double* K, const double* prev, const double* cur, double* m) {
  m[0] = (prev[0] - K[2]) / K[0]; m[1] = (prev[1] - K[3]) / K[1];
  m[2] = (cur[0] - K[2]) / K[0];  m[3] = (cur[1] - K[3]) / K[1];
}
BSG_FPR_FN double fpr_threshold_sq(const double* K, double threshold_px) {
  const double t = threshold_px / (0.5 * (K[0] + K[1]));
  return t * t;
}
// squared Sampson distance; every multiply-add is an explicit fma so that all inlined copies round alike
BSG_FPR_FN double fpr_sampson_sq(const double* E, double x1, double y1, double x2, double y2) {
  const double a0 = fma(E[0], x1, fma(E[1], y1, E[2])), a1 = fma(E[3], x1, fma(E[4], y1, E[5])), a2 = fma(E[6], x1, fma(E[7], y1, E[8]));
  const double b0 = fma(E[0], x2, fma(E[3], y2, E[6])), b1 = fma(E[1], x2, fma(E[4], y2, E[7]));
  const double r = fma(x2, a0, fma(y2, a1, a2));
  const double den = fma(a0, a0, fma(a1, a1, fma(b0, b0, b1 * b1)));
  return r * r / den;
}
BSG_FPR_FN int fpr_update_niters(double p, double ep, int niters) {
  const double num = log(1.0 - p), q = 1.0 - ep;
  const double t = 1.0 - q * q * q * q * q;
  const double den = t > 0.0 ? log(t) : -INFINITY;
  if (den >= 0.0 || -num >= (double)niters * (-den)) return niters;
  return (int)round(num / den);
}

// ---- 1. null space -------------------------------------------------------------------------------------------------------------------
// Q: 9 x 9.  In: rows 0..4 the epipolar rows.  Out: rows 0..4 an orthonormal basis of their span, rows 5..8 one of its complement
// (the next unit vector with the largest residual, orthogonalised twice).  false: the five rows are dependent.
BSG_FPR_FN void fpr_epipolar_row(const double* m /* x1 y1 x2 y2 */, double* row /* 9 */) {
  row[0] = m[2] * m[0]; row[1] = m[2] * m[1]; row[2] = m[2];
  row[3] = m[3] * m[0]; row[4] = m[3] * m[1]; row[5] = m[3];
  row[6] = m[0];        row[7] = m[1];        row[8] = 1.0;
}
BSG_FPR_FN double fpr_dot9(const double* a, const double* b) {
  double s = 0.0;
  for (int j = 0; j < 9; ++j) s = fma(a[j], b[j], s);
  return s;
}
BSG_FPR_FN bool fpr_nullspace(double* Q) {
  for (int i = 0; i < 9; ++i) {
    double* qi = Q + 9 * i;
    double n0 = 1.0;
    if (i < 5) {
      n0 = sqrt(fpr_dot9(qi, qi));
    } else {
      int bj = 0;
      double best = -1.0;
      for (int j = 0; j < 9; ++j) {
        double r = 1.0;
        for (int q = 0; q < i; ++q) r -= Q[9 * q + j] * Q[9 * q + j];
        if (r > best) { best = r; bj = j; }
      }
      for (int j = 0; j < 9; ++j) qi[j] = j == bj ? 1.0 : 0.0;
    }
    for (int pass = 0; pass < 2; ++pass)
      for (int q = 0; q < i; ++q) {
        const double d = fpr_dot9(Q + 9 * q, qi);
        for (int j = 0; j < 9; ++j) qi[j] = fma(-d, Q[9 * q + j], qi[j]);
      }
    const double nn = sqrt(fpr_dot9(qi, qi));
    if (!(nn > 1e-10 * n0)) return false;
    const double inv = 1.0 / nn;
    for (int j = 0; j < 9; ++j) qi[j] *= inv;
  }
  return true;
}

// ---- 2. the cubic constraints -------------------------------------------------------------------------------------------------------
// linear (x y z 1), quadratic (x^2 y^2 z^2 xy xz yz x y z 1) and cubic (the column order above) coefficient vectors
// entry e of E = x Eb[cyc] + y Eb[cyc + 1] + z Eb[cyc + 2] + Eb[3] (first-three indices mod 3): cyc picks which of the three free
// coordinates plays z, the variable the univariate polynomial is in
BSG_FPR_FN void fpr_lin(const double* Eb /* 4 x 9 */, int cyc, int e, double l[4]) {
  l[0] = Eb[9 * (cyc % 3) + e]; l[1] = Eb[9 * ((cyc + 1) % 3) + e]; l[2] = Eb[9 * ((cyc + 2) % 3) + e]; l[3] = Eb[27 + e];
}
BSG_FPR_FN void fpr_mac11(const double a[4], const double b[4], double s, double q[10]) {   // q += s a b
  q[0] += s * (a[0] * b[0]); q[1] += s * (a[1] * b[1]); q[2] += s * (a[2] * b[2]);
  q[3] += s * (a[0] * b[1] + a[1] * b[0]); q[4] += s * (a[0] * b[2] + a[2] * b[0]); q[5] += s * (a[1] * b[2] + a[2] * b[1]);
  q[6] += s * (a[0] * b[3] + a[3] * b[0]); q[7] += s * (a[1] * b[3] + a[3] * b[1]); q[8] += s * (a[2] * b[3] + a[3] * b[2]);
  q[9] += s * (a[3] * b[3]);
}
BSG_FPR_FN void fpr_mac21(const double q[10], const double l[4], double s, double c[20]) {   // c += s q l
  c[0] += s * (q[0] * l[0]);
  c[1] += s * (q[1] * l[1]);
  c[2] += s * (q[0] * l[1] + q[3] * l[0]);
  c[3] += s * (q[1] * l[0] + q[3] * l[1]);
  c[4] += s * (q[0] * l[2] + q[4] * l[0]);
  c[5] += s * (q[0] * l[3] + q[6] * l[0]);
  c[6] += s * (q[1] * l[2] + q[5] * l[1]);
  c[7] += s * (q[1] * l[3] + q[7] * l[1]);
  c[8] += s * (q[3] * l[2] + q[4] * l[1] + q[5] * l[0]);
  c[9] += s * (q[3] * l[3] + q[6] * l[1] + q[7] * l[0]);
  c[10] += s * (q[2] * l[0] + q[4] * l[2]);
  c[11] += s * (q[4] * l[3] + q[6] * l[2] + q[8] * l[0]);
  c[12] += s * (q[6] * l[3] + q[9] * l[0]);
  c[13] += s * (q[2] * l[1] + q[5] * l[2]);
  c[14] += s * (q[5] * l[3] + q[7] * l[2] + q[8] * l[1]);
  c[15] += s * (q[7] * l[3] + q[9] * l[1]);
  c[16] += s * (q[2] * l[2]);
  c[17] += s * (q[2] * l[3] + q[8] * l[2]);
  c[18] += s * (q[8] * l[3] + q[9] * l[2]);
  c[19] += s * (q[9] * l[3]);
}
// row r of the 10 x 20 system: r < 9 entry (r / 3, r % 3) of 2 E E^T E - tr(E E^T) E, r == 9 det E
BSG_FPR_FN void fpr_constraint_row(const double* Eb, int cyc, int r, double row[20]) {
  for (int j = 0; j < 20; ++j) row[j] = 0.0;
  double a[4], b[4], q[10];
  if (r < 9) {
    const int i = r / 3, jc = r % 3;
    for (int k = 0; k < 3; ++k) {
      for (int j = 0; j < 10; ++j) q[j] = 0.0;
      for (int l = 0; l < 3; ++l) { fpr_lin(Eb, cyc, 3 * i + l, a); fpr_lin(Eb, cyc, 3 * k + l, b); fpr_mac11(a, b, 1.0, q); }
      fpr_lin(Eb, cyc, 3 * k + jc, a);
      fpr_mac21(q, a, 2.0, row);
    }
    for (int j = 0; j < 10; ++j) q[j] = 0.0;
    for (int e = 0; e < 9; ++e) { fpr_lin(Eb, cyc, e, a); fpr_mac11(a, a, 1.0, q); }
    fpr_lin(Eb, cyc, 3 * i + jc, a);
    fpr_mac21(q, a, -1.0, row);
  } else {
    for (int c = 0; c < 3; ++c) {   // E[0][c] (E[1][c+1] E[2][c+2] - E[1][c+2] E[2][c+1])
      const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
      for (int j = 0; j < 10; ++j) q[j] = 0.0;
      fpr_lin(Eb, cyc, 3 + c1, a); fpr_lin(Eb, cyc, 6 + c2, b); fpr_mac11(a, b, 1.0, q);
      fpr_lin(Eb, cyc, 3 + c2, a); fpr_lin(Eb, cyc, 6 + c1, b); fpr_mac11(a, b, -1.0, q);
      fpr_lin(Eb, cyc, c, a);
      fpr_mac21(q, a, 1.0, row);
    }
  }
}

// ---- 3. elimination (the serial form; ransac_kernel keeps a row per lane and exchanges the pivot row across lanes) -------------------
// M: 10 x 20.  Out: row k led by a 1 in column k.  false: a zero or non-finite pivot.
BSG_FPR_FN bool fpr_gauss_jordan(double* M) {
  for (int k = 0; k < 10; ++k) {
    int p = k;
    for (int i = k + 1; i < 10; ++i) if (fabs(M[20 * i + k]) > fabs(M[20 * p + k])) p = i;
    const double piv = M[20 * p + k];
    if (!(fabs(piv) > 0.0) || !std::isfinite(piv)) return false;
    for (int j = 0; j < 20; ++j) { const double t = M[20 * p + j]; M[20 * p + j] = M[20 * k + j]; M[20 * k + j] = t / piv; }
    for (int i = 0; i < 10; ++i) {
      if (i == k) continue;
      const double f = M[20 * i + k];
      for (int j = 0; j < 20; ++j) M[20 * i + j] = fma(-f, M[20 * k + j], M[20 * i + j]);
    }
  }
  return true;
}

// The size of what the elimination left in the six rows used: the measure by which one of the three choices of z is kept.  The
// leading 10 x 10 block is badly conditioned for some choices (entries of 1e5..1e7 from an orthonormal basis, and a true E lost
// altogether in about 1 % of noise-free problems when z is fixed in advance); the smallest of the three keeps it below ~4e5.
BSG_FPR_FN double fpr_growth(double g, double v) { return std::isfinite(v) ? fmax(g, fabs(v)) : INFINITY; }

// ---- 4. B(z), its determinant, the derivative table -----------------------------------------------------------------------------------
// R: 6 x 10, the trailing columns of the rows led by x^2z, x^2, y^2z, y^2, xyz, xy.  B: 3 x 3 x 5 ascending coefficients.
// c: the 11 ascending coefficients of det B(z), scaled to a largest magnitude of 1.  false: not finite or identically zero.
BSG_FPR_FN bool fpr_det_poly(const double* R, double* B, double* c) {
  for (int p = 0; p < 3; ++p) {
    const double *a = R + 20 * p, *b = a + 10;
    double* Bp = B + 15 * p;
    for (int v = 0; v < 2; ++v) {
      Bp[5 * v] = a[3 * v + 2]; Bp[5 * v + 1] = a[3 * v + 1] - b[3 * v + 2]; Bp[5 * v + 2] = a[3 * v] - b[3 * v + 1];
      Bp[5 * v + 3] = -b[3 * v]; Bp[5 * v + 4] = 0.0;
    }
    Bp[10] = a[9]; Bp[11] = a[8] - b[9]; Bp[12] = a[7] - b[8]; Bp[13] = a[6] - b[7]; Bp[14] = -b[6];
  }
  for (int i = 0; i < 11; ++i) c[i] = 0.0;
  for (int p = 0; p < 3; ++p) {   // B[p][2] (B[p1][0] B[p2][1] - B[p1][1] B[p2][0])
    const int p1 = (p + 1) % 3, p2 = (p + 2) % 3;
    double t[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j)
        t[i + j] += B[15 * p1 + i] * B[15 * p2 + 5 + j] - B[15 * p1 + 5 + i] * B[15 * p2 + j];
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 7; ++j) c[i + j] = fma(B[15 * p + 10 + i], t[j], c[i + j]);
  }
  double mx = 0.0;
  bool fin = true;
  for (int i = 0; i < 11; ++i) { mx = fmax(mx, fabs(c[i])); fin = fin && std::isfinite(c[i]); }
  if (!fin || !(mx > 0.0)) return false;
  for (int i = 0; i < 11; ++i) c[i] /= mx;
  return true;
}
// the coefficients of p^(k), k = 0..9, packed: level k at D + fpr_level(k), 11 - k ascending coefficients.  Column i of the table
// (every level's share of c[i]) is independent of the others.
BSG_FPR_FN int fpr_level(int k) { return k * 11 - k * (k - 1) / 2; }
BSG_FPR_FN void fpr_deriv_column(double ci, int i, double* D) {
  double f = 1.0;
  for (int k = 0; k <= i && k < 10; ++k) { D[fpr_level(k) + i - k] = ci * f; f *= (double)(i - k); }
}
// Cauchy's bound on every root of p and, by Gauss-Lucas, of its derivatives; capped
BSG_FPR_FN double fpr_root_bound(const double* c) {
  double mx = 0.0;
  for (int i = 0; i < 10; ++i) mx = fmax(mx, fabs(c[i]));
  const double b = 1.0 + mx / fabs(c[10]);
  return b < kFprRootBound ? b : kFprRootBound;   // (NaN or inf: the cap)
}
BSG_FPR_FN void fpr_horner(const double* d, int deg, double z, double& f, double& df) {
  f = d[deg]; df = 0.0;
  for (int i = deg - 1; i >= 0; --i) { df = fma(df, z, f); f = fma(f, z, d[i]); }
}
// the root of the degree-deg polynomial d in (lo, hi) when its values there differ in sign: Newton kept inside a shrinking bracket,
// bisection whenever Newton leaves it or converges slowly; at most 200 evaluations
BSG_FPR_FN bool fpr_interval_root(const double* d, int deg, double lo, double hi, double* root) {
  double flo, fhi, f, df;
  fpr_horner(d, deg, lo, flo, df);
  fpr_horner(d, deg, hi, fhi, df);
  if (!((flo < 0.0 && fhi > 0.0) || (flo > 0.0 && fhi < 0.0))) return false;
  double xl = flo < 0.0 ? lo : hi, xh = flo < 0.0 ? hi : lo;
  double x = 0.5 * (lo + hi), dxold = fabs(hi - lo), dx = dxold;
  fpr_horner(d, deg, x, f, df);
  for (int it = 0; it < 200; ++it) {
    if (f == 0.0) break;
    if (((x - xh) * df - f) * ((x - xl) * df - f) > 0.0 || fabs(2.0 * f) > fabs(dxold * df) || !std::isfinite(df)) {
      dxold = dx; dx = 0.5 * (xh - xl);
      const double xn = xl + dx;
      if (xn == xl || xn == xh) break;
      x = xn;
    } else {
      dxold = dx; dx = f / df;
      const double xn = x - dx;
      if (xn == x) break;
      x = xn;
    }
    fpr_horner(d, deg, x, f, df);
    if (f < 0.0) xl = x; else xh = x;
    if (fabs(dx) <= 2e-16 * fabs(x)) break;
  }
  *root = x;
  return true;
}

// ---- 5. back-substitution -------------------------------------------------------------------------------------------------------------
// Gauss-Newton on the ten ORIGINAL constraints over the coefficients c of Eb[0..2] (E = c0 Eb0 + c1 Eb1 + c2 Eb2 + Eb3): what the
// elimination and the degree-10 polynomial lost is recovered from the well-conditioned system they came from.  At most three steps,
// each kept only while the residual norm falls, so a root never gets worse.
BSG_FPR_FN void fpr_mm3(const double* A, const double* B, double* C, bool ta, bool tb) {   // C = op(A) op(B)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s = fma(ta ? A[3 * k + i] : A[3 * i + k], tb ? B[3 * j + k] : B[3 * k + j], s);
      C[3 * i + j] = s;
    }
}
BSG_FPR_FN void fpr_polish(const double* Eb, double c[3]) {
  double prev[3] = {c[0], c[1], c[2]}, fprev = INFINITY;
  for (int it = 0; it < 4; ++it) {
    double E[9], EEt[9], EtE[9], cof[9], r[10];
    for (int e = 0; e < 9; ++e) E[e] = fma(c[0], Eb[e], fma(c[1], Eb[9 + e], fma(c[2], Eb[18 + e], Eb[27 + e])));
    fpr_mm3(E, E, EEt, false, true);
    fpr_mm3(E, E, EtE, true, false);
    const double tr = EEt[0] + EEt[4] + EEt[8];
    fpr_mm3(EEt, E, r, false, false);
    double f = 0.0;
    for (int e = 0; e < 9; ++e) { r[e] = 2.0 * r[e] - tr * E[e]; f = fma(r[e], r[e], f); }
    cof[0] = E[4] * E[8] - E[5] * E[7]; cof[1] = E[5] * E[6] - E[3] * E[8]; cof[2] = E[3] * E[7] - E[4] * E[6];
    cof[3] = E[2] * E[7] - E[1] * E[8]; cof[4] = E[0] * E[8] - E[2] * E[6]; cof[5] = E[1] * E[6] - E[0] * E[7];
    cof[6] = E[1] * E[5] - E[2] * E[4]; cof[7] = E[2] * E[3] - E[0] * E[5]; cof[8] = E[0] * E[4] - E[1] * E[3];
    r[9] = E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2];
    f = fma(r[9], r[9], f);
    if (!(f < fprev)) { c[0] = prev[0]; c[1] = prev[1]; c[2] = prev[2]; return; }
    if (it == 3 || f == 0.0) return;
    fprev = f; prev[0] = c[0]; prev[1] = c[1]; prev[2] = c[2];
    double J[3][10], H[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    for (int b = 0; b < 3; ++b) {
      const double* dE = Eb + 9 * b;
      double t1[9], t2[9], t3[9], t4[9], ip = 0.0;
      fpr_mm3(dE, EtE, t1, false, false);
      fpr_mm3(dE, E, t2, true, false);
      fpr_mm3(E, t2, t3, false, false);
      fpr_mm3(EEt, dE, t4, false, false);
      J[b][9] = 0.0;
      for (int e = 0; e < 9; ++e) { ip = fma(E[e], dE[e], ip); J[b][9] = fma(cof[e], dE[e], J[b][9]); }
      for (int e = 0; e < 9; ++e) J[b][e] = 2.0 * (t1[e] + t3[e] + t4[e]) - 2.0 * ip * E[e] - tr * dE[e];
    }
    for (int k = 0; k < 10; ++k) {
      H[0] = fma(J[0][k], J[0][k], H[0]); H[1] = fma(J[0][k], J[1][k], H[1]); H[2] = fma(J[0][k], J[2][k], H[2]);
      H[3] = fma(J[1][k], J[1][k], H[3]); H[4] = fma(J[1][k], J[2][k], H[4]); H[5] = fma(J[2][k], J[2][k], H[5]);
      g[0] = fma(J[0][k], r[k], g[0]); g[1] = fma(J[1][k], r[k], g[1]); g[2] = fma(J[2][k], r[k], g[2]);
    }
    // H = [0 1 2; 1 3 4; 2 4 5]: the step from its adjugate
    const double a0 = H[3] * H[5] - H[4] * H[4], a1 = H[2] * H[4] - H[1] * H[5], a2 = H[1] * H[4] - H[2] * H[3];
    const double dt = H[0] * a0 + H[1] * a1 + H[2] * a2;
    if (!(dt > 0.0) || !std::isfinite(dt)) return;
    const double a3 = H[0] * H[5] - H[2] * H[2], a4 = H[1] * H[2] - H[0] * H[4], a5 = H[0] * H[3] - H[1] * H[1];
    c[0] -= (a0 * g[0] + a1 * g[1] + a2 * g[2]) / dt;
    c[1] -= (a1 * g[0] + a3 * g[1] + a4 * g[2]) / dt;
    c[2] -= (a2 * g[0] + a4 * g[1] + a5 * g[2]) / dt;
  }
}

BSG_FPR_FN bool fpr_backsub(const double* B, const double* Eb, int cyc, double z, double* E /* 9 */) {
  double M[9];
  for (int e = 0; e < 9; ++e) {
    const double* b = B + 5 * e;
    M[e] = fma(fma(fma(fma(b[4], z, b[3]), z, b[2]), z, b[1]), z, b[0]);
  }
  double x = 0.0, y = 0.0, w = 0.0;
  for (int p = 0; p < 3; ++p) {   // the null vector from the pair of rows whose cross product has the largest third entry
    const double *r0 = M + 3 * (p == 2 ? 1 : 0), *r1 = M + 3 * (p == 0 ? 1 : 2);
    const double v2 = r0[0] * r1[1] - r0[1] * r1[0];
    if (fabs(v2) > fabs(w)) { w = v2; x = r0[1] * r1[2] - r0[2] * r1[1]; y = r0[2] * r1[0] - r0[0] * r1[2]; }
  }
  if (!(fabs(w) > 0.0)) return false;
  x /= w; y /= w;
  double c[3];   // coefficients of Eb[0..2]
  c[0] = cyc == 0 ? x : cyc == 1 ? z : y;
  c[1] = cyc == 0 ? y : cyc == 1 ? x : z;
  c[2] = cyc == 0 ? z : cyc == 1 ? y : x;
  if (std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2])) fpr_polish(Eb, c);
  double n2 = 0.0, big = 0.0;
  for (int e = 0; e < 9; ++e) {
    E[e] = fma(c[0], Eb[e], fma(c[1], Eb[9 + e], fma(c[2], Eb[18 + e], Eb[27 + e])));
    n2 = fma(E[e], E[e], n2);
    if (fabs(E[e]) > fabs(big)) big = E[e];
  }
  if (!(n2 > 0.0) || !std::isfinite(n2)) return false;
  const double s = (big < 0.0 ? -1.0 : 1.0) / sqrt(n2);
  for (int e = 0; e < 9; ++e) E[e] *= s;
  return true;
}

// ---- the serial compositions -----------------------------------------------------------------------------------------------------------
// m: 5 normalised matches (x1 y1 x2 y2 each); E: up to kFprMaxSol x 9, ascending E[0]; returns the number of solutions
inline int fpr_five_point(const double* m, double* E) {
  double ws[kFprWork], M[200];
  double *Q = ws + kFprQ, *R = ws + kFprR, *B = ws + kFprB, *D = ws + kFprD, *roots = ws + kFprRoots;
  for (int i = 0; i < 5; ++i) fpr_epipolar_row(m + 4 * i, Q + 9 * i);
  if (!fpr_nullspace(Q)) return 0;
  const double* Eb = Q + 45;
  int cyc = -1;
  double growth = INFINITY;
  for (int v = 0; v < 3; ++v) {
    for (int r = 0; r < 10; ++r) fpr_constraint_row(Eb, v, r, M + 20 * r);
    if (!fpr_gauss_jordan(M)) continue;
    double g = 0.0;
    for (int r = 0; r < 6; ++r)
      for (int j = 0; j < 10; ++j) g = fpr_growth(g, M[20 * (4 + r) + 10 + j]);
    if (!(g < growth)) continue;
    growth = g; cyc = v;
    for (int r = 0; r < 6; ++r)
      for (int j = 0; j < 10; ++j) R[10 * r + j] = M[20 * (4 + r) + 10 + j];
  }
  if (cyc < 0) return 0;
  double c[11];
  if (!fpr_det_poly(R, B, c)) return 0;
  for (int i = 0; i <= 10; ++i) fpr_deriv_column(c[i], i, D);
  const double bound = fpr_root_bound(c);
  int m_prev = 0;
  double *prev = roots, *cur = roots + 12;
  for (int k = 9; k >= 0; --k) {
    int mc = 0;
    for (int iv = 0; iv <= m_prev; ++iv) {
      const double lo = iv == 0 ? -bound : prev[iv - 1], hi = iv == m_prev ? bound : prev[iv];
      double r;
      if (fpr_interval_root(D + fpr_level(k), 10 - k, lo, hi, &r)) cur[mc++] = r;
    }
    double* t = prev; prev = cur; cur = t;
    m_prev = mc;
  }
  int ns = 0;
  for (int i = 0; i < m_prev; ++i) {
    double Ei[9];
    if (!fpr_backsub(B, Eb, cyc, prev[i], Ei)) continue;
    int pos = ns++;
    while (pos > 0 && E[9 * (pos - 1)] > Ei[0]) { for (int e = 0; e < 9; ++e) E[9 * pos + e] = E[9 * (pos - 1) + e]; --pos; }
    for (int e = 0; e < 9; ++e) E[9 * pos + e] = Ei[e];
  }
  return ns;
}

// The contract's loop for one set.  xn: 4 n doubles of workspace (the normalised matches).  Outputs as bsgpu_essential_ransac's.
inline void fpr_ransac_serial(int n, const double* px_prev, const double* px_cur, const double* K, double prob, double threshold_px,
                              int max_iters, uint64_t seed, uint64_t set_index, double* xn, uint8_t* mask, double* E_out,
                              int* n_inliers, int* n_iters, int* best_sample, int* status) {
  for (int i = 0; i < n; ++i) mask[i] = 1;
  for (int e = 0; e < 9; ++e) E_out[e] = 0.0;
  for (int k = 0; k < 5; ++k) best_sample[k] = -1;
  *n_inliers = 0; *n_iters = 0;
  if (n < 5) { *status = FPR_TOO_FEW; return; }
  *status = FPR_NO_MODEL;
  for (int i = 0; i < n; ++i) fpr_normalize(K, px_prev + 2 * i, px_cur + 2 * i, xn + 4 * i);
  const double thr2 = fpr_threshold_sq(K, threshold_px);
  int niters = max_iters, best = 0, s = 0;
  for (; s < niters; ++s) {
    int idx[5];
    double m[20], E[9 * kFprMaxSol];
    fpr_sample(seed, set_index, (uint64_t)s, n, idx);
    for (int k = 0; k < 5; ++k) for (int j = 0; j < 4; ++j) m[4 * k + j] = xn[4 * idx[k] + j];
    const int ns = fpr_five_point(m, E);
    for (int h = 0; h < ns; ++h) {
      int good = 0;
      for (int i = 0; i < n; ++i) good += fpr_sampson_sq(E + 9 * h, xn[4 * i], xn[4 * i + 1], xn[4 * i + 2], xn[4 * i + 3]) <= thr2 ? 1 : 0;
      if (good > (best > 4 ? best : 4)) {
        best = good;
        for (int e = 0; e < 9; ++e) E_out[e] = E[9 * h + e];
        for (int k = 0; k < 5; ++k) best_sample[k] = idx[k];
        niters = fpr_update_niters(prob, (double)(n - good) / (double)n, niters);
      }
    }
  }
  *n_iters = s;
  if (best == 0) return;
  *status = FPR_OK;
  *n_inliers = best;
  for (int i = 0; i < n; ++i) mask[i] = fpr_sampson_sq(E_out, xn[4 * i], xn[4 * i + 1], xn[4 * i + 2], xn[4 * i + 3]) <= thr2 ? 1 : 0;
}

}  // namespace bsg
