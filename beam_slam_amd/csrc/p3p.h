// P3P RANSAC frame poses (bsgpu_absolute_pose_ransac): what bs_models::vision::ComputePathWithVision
// (bs_models/src/lib/vision/utils.cpp:143-188) gets per keyframe from [EXT]
// beam_cv::AbsolutePoseEstimator::RANSACEstimator(camera_model, pixels, points, 100).  libbeam is not part of the reference checkout:
// the semantics restated here are RECALLED, not verified (DESIGN.md "Absolute-pose RANSAC").
//
// Host- and device-compilable, in the style of five_point.h: plain C++, nothing from HIP but the qualifiers.  The solver is split so
// that p3p_kernel (k_p3p.hip) can give a sample to four lanes: p3p_setup is the part all of them repeat, p3p_candidate /
// p3p_polish / p3p_pose are one solution's.  p3p_solve and p3p_ransac_serial compose the same blocks serially: the contract's loop
// for one frame, used by the CPU tests and the host stand-in and by nothing in the product at run time.
//
// The minimal solver is Lambda Twist (Persson & Nordberg, ECCV 2018), written from the paper's derivation:
//   1. unit bearings y_i, cosines c_ij = y_i . y_j, squared distances a_ij = |x_i - x_j|^2; the depths satisfy
//      l_i^2 + l_j^2 - 2 c_ij l_i l_j = a_ij, i.e. L^T M_ij L = a_ij;
//   2. two homogeneous combinations A = a23 M12 - a12 M23, B = a23 M13 - a13 M23 (swapped so that |det B| >= |det A|); one real root
//      g of the cubic det(A + g B) = 0 — an outer root, by Newton from the far side of the outer stationary point, where the
//      iteration is monotone; bounded work, no complex arithmetic;
//   3. D = A + g B has the eigenvalues (s1, s2, 0) with s1 s2 < 0 when a real solution exists: L^T D L = 0 factors into two planes
//      (sqrt|s1| e1 +- sqrt|s2| e2) . L = 0;
//   4. on each plane l1 = p l2 + q l3; with l3 = tau l2 the other combination (B when |g| < 1, A otherwise: the one D is not close to)
//      is a quadratic in tau: up to two roots per plane, four depth triples, l2 from the (2, 3) constraint;
//   5. per triple a few Gauss-Newton steps on the three constraints, each kept only while the residual falls, then
//      R = Y X^-1 from the two difference vectors and their cross product on either side, t = l1 y1 - R x1.
// Solutions of one sample are ordered by ascending camera-frame depth of the sample's first point so that the loop's "first strictly
// better" rule does not depend on how an implementation enumerates them.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BSG_P3P_FN __host__ __device__ inline
#else
#define BSG_P3P_FN inline
#endif

namespace bsg {

constexpr int kP3pMaxSol = 4;
enum { P3P_OK = 0, P3P_TOO_FEW = 1, P3P_NO_MODEL = 2 };   // BSGPU_RANSAC_* of include/bsgpu.h

// ---- sampler: fpr_sample's counter-based splitmix64 stream and redraw rule, three indices -----------------------------------------------
BSG_P3P_FN int p3p_draw(uint64_t& state, int n) {
  state += 0x9E3779B97F4A7C15ull;
  uint64_t z = state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (int)(z % (uint64_t)n);
}
// n >= 3.  (Written without an index array so that the kernel's copy stays in registers.)
BSG_P3P_FN void p3p_sample(uint64_t seed, uint64_t frame_index, uint64_t sample_index, int n, int& i0, int& i1, int& i2) {
  uint64_t state = seed ^ (frame_index * 0x9E3779B97F4A7C15ull) ^ (sample_index * 0xBF58476D1CE4E5B9ull);
  i0 = p3p_draw(state, n);
  do i1 = p3p_draw(state, n); while (i1 == i0);
  do i2 = p3p_draw(state, n); while (i2 == i0 || i2 == i1);
}

// ---- score, iteration update ------------------------------------------------------------------------------------------------------------
// T: T_CAMERA_WORLD, 12 row-major [R|t]; K = (fx, fy, cx, cy).  Inlier iff P_c.z > 0 and |z - pi(K, P_c)|^2 < thr2.  Every
// multiply-add is an explicit fma so that all inlined copies round alike.
BSG_P3P_FN bool p3p_inlier(const double* T, const double* K, double u, double v, double X, double Y, double Z, double thr2) {
  const double x = fma(T[0], X, fma(T[1], Y, fma(T[2], Z, T[3])));
  const double y = fma(T[4], X, fma(T[5], Y, fma(T[6], Z, T[7])));
  const double z = fma(T[8], X, fma(T[9], Y, fma(T[10], Z, T[11])));
  const double ex = fma(K[0], x / z, K[2]) - u, ey = fma(K[1], y / z, K[3]) - v;
  return z > 0.0 && fma(ex, ex, ey * ey) < thr2;
}
BSG_P3P_FN double p3p_pixel(double v, int truncate) { return truncate ? trunc(v) : v; }
// fpr_update_niters with exponent 3; prob outside (0, 1) (the contract's prob == 0): no early termination
BSG_P3P_FN int p3p_update_niters(double p, double ep, int niters) {
  if (!(p > 0.0 && p < 1.0)) return niters;
  const double num = log(1.0 - p), q = 1.0 - ep;
  const double t = 1.0 - q * q * q;
  const double den = t > 0.0 ? log(t) : -INFINITY;
  if (den >= 0.0 || -num >= (double)niters * (-den)) return niters;
  return (int)round(num / den);
}

// ---- small symmetric 3 x 3 algebra: (00 01 02 11 12 22) --------------------------------------------------------------------------------
BSG_P3P_FN void p3p_adj(const double* A, double* J) {
  J[0] = A[3] * A[5] - A[4] * A[4]; J[1] = A[2] * A[4] - A[1] * A[5]; J[2] = A[1] * A[4] - A[2] * A[3];
  J[3] = A[0] * A[5] - A[2] * A[2]; J[4] = A[1] * A[2] - A[0] * A[4]; J[5] = A[0] * A[3] - A[1] * A[1];
}
BSG_P3P_FN double p3p_tr(const double* J, const double* B) {   // trace(J B)
  return J[0] * B[0] + J[3] * B[3] + J[5] * B[5] + 2.0 * (J[1] * B[1] + J[2] * B[2] + J[4] * B[4]);
}
BSG_P3P_FN void p3p_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
BSG_P3P_FN double p3p_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// unit null vector of D - e I (D symmetric, e an eigenvalue): the largest cross product of two of its rows
BSG_P3P_FN void p3p_eigvec(const double* D, double e, double* v) {
  const double r0[3] = {D[0] - e, D[1], D[2]}, r1[3] = {D[1], D[3] - e, D[4]}, r2[3] = {D[2], D[4], D[5] - e};
  double c0[3], c1[3], c2[3];
  p3p_cross(r0, r1, c0); p3p_cross(r0, r2, c1); p3p_cross(r1, r2, c2);
  const double n0 = p3p_dot(c0, c0), n1 = p3p_dot(c1, c1), n2 = p3p_dot(c2, c2);
  const bool use0 = n0 >= n1 && n0 >= n2, use1 = !use0 && n1 >= n2;
  const double nn = 1.0 / sqrt(use0 ? n0 : use1 ? n1 : n2);
  for (int i = 0; i < 3; ++i) v[i] = (use0 ? c0[i] : use1 ? c1[i] : c2[i]) * nn;
}
// one real root of x^3 + b x^2 + c x + d: an outer one when there are three
BSG_P3P_FN double p3p_cubic_root(double b, double c, double d) {
  double x;
  const double disc = b * b - 3.0 * c;
  if (disc > 0.0) {
    const double sq = sqrt(disc), t1 = (-b - sq) / 3.0, t2 = (-b + sq) / 3.0;   // local maximum, local minimum
    const double h1 = ((t1 + b) * t1 + c) * t1 + d;
    if (h1 > 0.0) {   // a root left of the maximum: start from the parabola fitted there
      x = t1 - sqrt(h1 / sq);
    } else {
      const double h2 = ((t2 + b) * t2 + c) * t2 + d;
      x = t2 + sqrt(fmax(-h2, 0.0) / sq);
    }
  } else {
    x = -b / 3.0;   // monotone: from the inflection point the first step lands on the root's convex side
  }
  for (int it = 0; it < 60; ++it) {
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

// ---- the solver ----------------------------------------------------------------------------------------------------------------------------
// what every solution of a sample shares
struct P3pSetup {
  double y[9];            // unit bearings, one per row
  double x0[3];           // the first world point
  double Xi[9];           // rows of X^-1 |d1 x d2|^2: d2 x d3, d3 x d1, d3 (d1 = x0 - x1, d2 = x0 - x2, d3 = d1 x d2)
  double inv_det;         // 1 / |d3|^2
  double c12, c13, c23, a12, a13, a23;
  double Q[6];            // the combination the quadratic in tau comes from
  double e1[3], e2[3];    // sqrt|s1| e1, sqrt|s2| e2
  bool ok;
};

BSG_P3P_FN void p3p_setup(const double* px /* 3 x 2 */, const double* P /* 3 x 3 */, const double* K, P3pSetup& S) {
  for (int i = 0; i < 3; ++i) {
    const double bx = (px[2 * i] - K[2]) / K[0], by = (px[2 * i + 1] - K[3]) / K[1];
    const double nn = 1.0 / sqrt(bx * bx + by * by + 1.0);
    S.y[3 * i] = bx * nn; S.y[3 * i + 1] = by * nn; S.y[3 * i + 2] = nn;
  }
  double d1[3], d2[3], d3[3], d23[3];
  for (int i = 0; i < 3; ++i) { S.x0[i] = P[i]; d1[i] = P[i] - P[3 + i]; d2[i] = P[i] - P[6 + i]; d23[i] = P[3 + i] - P[6 + i]; }
  p3p_cross(d1, d2, d3);
  p3p_cross(d2, d3, S.Xi); p3p_cross(d3, d1, S.Xi + 3);
  for (int i = 0; i < 3; ++i) S.Xi[6 + i] = d3[i];
  const double det = p3p_dot(d3, d3);
  S.inv_det = 1.0 / det;
  S.c12 = p3p_dot(S.y, S.y + 3); S.c13 = p3p_dot(S.y, S.y + 6); S.c23 = p3p_dot(S.y + 3, S.y + 6);
  S.a12 = p3p_dot(d1, d1); S.a13 = p3p_dot(d2, d2); S.a23 = p3p_dot(d23, d23);
  const double a12 = S.a12, a13 = S.a13, a23 = S.a23;
  double A[6] = {a23, -a23 * S.c12, 0.0, a23 - a12, a12 * S.c23, -a12};
  double B[6] = {a23, 0.0, -a23 * S.c13, -a13, a13 * S.c23, a23 - a13};
  double JA[6], JB[6];
  p3p_adj(A, JA); p3p_adj(B, JB);
  double k0 = A[0] * JA[0] + A[1] * JA[1] + A[2] * JA[2], k3 = B[0] * JB[0] + B[1] * JB[1] + B[2] * JB[2];
  double k1 = p3p_tr(JA, B), k2 = p3p_tr(JB, A);
  const bool swap = fabs(k3) < fabs(k0);
  if (swap) {
    for (int i = 0; i < 6; ++i) { const double t = A[i]; A[i] = B[i]; B[i] = t; }
    double t = k0; k0 = k3; k3 = t;
    t = k1; k1 = k2; k2 = t;
  }
  const double g = p3p_cubic_root(k2 / k3, k1 / k3, k0 / k3);
  double D[6];
  for (int i = 0; i < 6; ++i) { D[i] = A[i] + g * B[i]; S.Q[i] = fabs(g) < 1.0 ? B[i] : A[i]; }
  // the two non-zero eigenvalues: roots of s^2 - tr s + m, m the sum of the principal 2 x 2 minors; of opposite sign iff m < 0
  const double tr = D[0] + D[3] + D[5];
  const double m = (D[0] * D[3] - D[1] * D[1]) + (D[0] * D[5] - D[2] * D[2]) + (D[3] * D[5] - D[4] * D[4]);
  const double h = 0.5 * tr, rad = sqrt(h * h - m);
  const double s1 = h + (h < 0.0 ? -rad : rad), s2 = m / s1;
  S.ok = det > 0.0 && std::isfinite(g) && m < 0.0 && std::isfinite(s1) && std::isfinite(s2);
  p3p_eigvec(D, s1, S.e1); p3p_eigvec(D, s2, S.e2);
  const double w1 = sqrt(fabs(s1)), w2 = sqrt(fabs(s2));
  for (int i = 0; i < 3; ++i) { S.e1[i] *= w1; S.e2[i] *= w2; }
}

// candidate k = 2 * plane + root: the depth triple, before its polish.  false: no such real solution with positive depths
BSG_P3P_FN bool p3p_candidate(const P3pSetup& S, int k, double* l /* 3 */) {
  const double sg = (k & 2) ? -1.0 : 1.0;
  const double v0 = S.e1[0] + sg * S.e2[0], v1 = S.e1[1] + sg * S.e2[1], v2 = S.e1[2] + sg * S.e2[2];
  const double p = -v1 / v0, q = -v2 / v0;   // l1 = p l2 + q l3
  const double* Q = S.Q;
  const double qa = Q[0] * q * q + 2.0 * Q[2] * q + Q[5];
  const double qb = 2.0 * (Q[0] * p * q + Q[1] * q + Q[2] * p + Q[4]);
  const double qc = Q[0] * p * p + 2.0 * Q[1] * p + Q[3];
  const double disc = qb * qb - 4.0 * qa * qc;
  if (!S.ok || !(disc >= 0.0)) return false;
  const double sq = sqrt(disc), qq = -0.5 * (qb + (qb < 0.0 ? -sq : sq));
  const double tau = (k & 1) ? qc / qq : qq / qa;
  if (!(tau > 0.0) || !std::isfinite(tau)) return false;
  const double den = tau * (tau - 2.0 * S.c23) + 1.0;
  l[1] = sqrt(S.a23 / den); l[2] = tau * l[1]; l[0] = (p + q * tau) * l[1];
  return l[0] > 0.0 && l[1] > 0.0 && std::isfinite(l[0]) && std::isfinite(l[2]);
}

// Gauss-Newton on the three distance constraints; at most five steps, each kept only while the residual norm falls
BSG_P3P_FN double p3p_residual(const P3pSetup& S, double l0, double l1, double l2, double* r) {
  r[0] = l0 * l0 + l1 * l1 - 2.0 * S.c12 * l0 * l1 - S.a12;
  r[1] = l0 * l0 + l2 * l2 - 2.0 * S.c13 * l0 * l2 - S.a13;
  r[2] = l1 * l1 + l2 * l2 - 2.0 * S.c23 * l1 * l2 - S.a23;
  return r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
}
BSG_P3P_FN void p3p_polish(const P3pSetup& S, double* l) {
  double l0 = l[0], l1 = l[1], l2 = l[2], r[3];
  double f = p3p_residual(S, l0, l1, l2, r);
  for (int it = 0; it < 5 && f > 0.0; ++it) {
    // J = [j00 j01 0; j10 0 j12; 0 j21 j22]
    const double j00 = 2.0 * (l0 - S.c12 * l1), j01 = 2.0 * (l1 - S.c12 * l0), j10 = 2.0 * (l0 - S.c13 * l2), j12 = 2.0 * (l2 - S.c13 * l0);
    const double j21 = 2.0 * (l1 - S.c23 * l2), j22 = 2.0 * (l2 - S.c23 * l1);
    const double dt = -j00 * j12 * j21 - j01 * j10 * j22;
    if (!(fabs(dt) > 0.0) || !std::isfinite(dt)) break;
    const double n0 = l0 - (-j12 * j21 * r[0] - j01 * j22 * r[1] + j01 * j12 * r[2]) / dt;
    const double n1 = l1 - (-j10 * j22 * r[0] + j00 * j22 * r[1] - j00 * j12 * r[2]) / dt;
    const double n2 = l2 - (j10 * j21 * r[0] - j00 * j21 * r[1] - j01 * j10 * r[2]) / dt;
    double rn[3];
    const double fn = p3p_residual(S, n0, n1, n2, rn);
    if (!(fn < f)) break;
    l0 = n0; l1 = n1; l2 = n2; f = fn;
    for (int i = 0; i < 3; ++i) r[i] = rn[i];
  }
  l[0] = l0; l[1] = l1; l[2] = l2;
}

// T_CAMERA_WORLD (12, row-major [R|t]) of a depth triple.  false: a depth not positive or a pose not finite
BSG_P3P_FN bool p3p_pose(const P3pSetup& S, const double* l, double* T) {
  double z1[3], z2[3], z3[3];
  for (int i = 0; i < 3; ++i) { z1[i] = l[0] * S.y[i] - l[1] * S.y[3 + i]; z2[i] = l[0] * S.y[i] - l[2] * S.y[6 + i]; }
  p3p_cross(z1, z2, z3);
  bool fin = l[0] > 0.0 && l[1] > 0.0 && l[2] > 0.0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = (z1[i] * S.Xi[j] + z2[i] * S.Xi[3 + j] + z3[i] * S.Xi[6 + j]) * S.inv_det;
    T[4 * i + 3] = l[0] * S.y[i] - (T[4 * i] * S.x0[0] + T[4 * i + 1] * S.x0[1] + T[4 * i + 2] * S.x0[2]);
    for (int j = 0; j < 4; ++j) fin = fin && std::isfinite(T[4 * i + j]);
  }
  return fin;
}
// the ordering key of a solution: the camera-frame depth of the sample's first point
BSG_P3P_FN double p3p_key(const P3pSetup& S, const double* l) { return l[0] * S.y[2]; }

// T_WORLD_BASELINK = T_CAMERA_WORLD^-1 T_cam_baselink (visual_odometry.cpp:252-253): quaternion wxyz, w >= 0, unit; position
BSG_P3P_FN void p3p_baselink_pose(const double* T, const double* R_cb, const double* t_cb, double* q, double* p) {
  double R[9];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[3 * i + j] = T[i] * R_cb[j] + T[4 + i] * R_cb[3 + j] + T[8 + i] * R_cb[6 + j];
    p[i] = T[i] * (t_cb[0] - T[3]) + T[4 + i] * (t_cb[1] - T[7]) + T[8 + i] * (t_cb[2] - T[11]);
  }
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

// ---- the serial compositions ---------------------------------------------------------------------------------------------------------------
// px: 3 pixels, P: 3 world points; T: up to kP3pMaxSol x 12, ascending key; returns the number of solutions
inline int p3p_solve(const double* px, const double* P, const double* K, double* T) {
  P3pSetup S;
  p3p_setup(px, P, K, S);
  double keys[kP3pMaxSol];
  int ns = 0;
  for (int k = 0; k < 4; ++k) {
    double l[3], Tk[12];
    if (!p3p_candidate(S, k, l)) continue;
    p3p_polish(S, l);
    if (!p3p_pose(S, l, Tk)) continue;
    const double key = p3p_key(S, l);
    int pos = ns++;
    while (pos > 0 && keys[pos - 1] > key) { keys[pos] = keys[pos - 1]; for (int e = 0; e < 12; ++e) T[12 * pos + e] = T[12 * (pos - 1) + e]; --pos; }
    keys[pos] = key;
    for (int e = 0; e < 12; ++e) T[12 * pos + e] = Tk[e];
  }
  return ns;
}

// The contract's loop for one frame.  Outputs as bsgpu_absolute_pose_ransac's (T_out: T_CAMERA_WORLD, NaN without a model).
inline void p3p_ransac_serial(int n, const double* pixels, const double* points, const double* K, double prob, double threshold_px,
                              int max_iters, uint64_t seed, uint64_t frame_index, int truncate, uint8_t* mask, double* T_out,
                              int* n_inliers, int* n_iters, int* best_sample, int* status) {
  for (int i = 0; i < n; ++i) mask[i] = 0;
  for (int e = 0; e < 12; ++e) T_out[e] = NAN;
  for (int k = 0; k < 3; ++k) best_sample[k] = -1;
  *n_inliers = 0; *n_iters = 0;
  if (n < 4) { *status = P3P_TOO_FEW; return; }
  *status = P3P_NO_MODEL;
  const double thr2 = threshold_px * threshold_px;
  int niters = max_iters, best = 0, s = 0;
  for (; s < niters; ++s) {
    int idx[3];
    double px[6], P[9], T[12 * kP3pMaxSol];
    p3p_sample(seed, frame_index, (uint64_t)s, n, idx[0], idx[1], idx[2]);
    for (int k = 0; k < 3; ++k) {
      for (int j = 0; j < 2; ++j) px[2 * k + j] = p3p_pixel(pixels[2 * idx[k] + j], truncate);
      for (int j = 0; j < 3; ++j) P[3 * k + j] = points[3 * idx[k] + j];
    }
    const int ns = p3p_solve(px, P, K, T);
    for (int h = 0; h < ns; ++h) {
      int good = 0;
      for (int i = 0; i < n; ++i)
        good += p3p_inlier(T + 12 * h, K, p3p_pixel(pixels[2 * i], truncate), p3p_pixel(pixels[2 * i + 1], truncate), points[3 * i],
                           points[3 * i + 1], points[3 * i + 2], thr2) ? 1 : 0;
      if (good > (best > 3 ? best : 3)) {
        best = good;
        for (int e = 0; e < 12; ++e) T_out[e] = T[12 * h + e];
        for (int k = 0; k < 3; ++k) best_sample[k] = idx[k];
        niters = p3p_update_niters(prob, (double)(n - good) / (double)n, niters);
      }
    }
  }
  *n_iters = s;
  if (best == 0) return;
  *status = P3P_OK;
  *n_inliers = best;
  for (int i = 0; i < n; ++i)
    mask[i] = p3p_inlier(T_out, K, p3p_pixel(pixels[2 * i], truncate), p3p_pixel(pixels[2 * i + 1], truncate), points[3 * i],
                         points[3 * i + 1], points[3 * i + 2], thr2) ? 1 : 0;
}

}  // namespace bsg
