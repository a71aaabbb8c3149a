// One track of bsgpu_triangulate (k_triang.hip): the DLT of [EXT] beam_cv::Triangulation::TriangulatePoint restated — the right
// singular vector of the smallest singular value of the 2V x 4 matrix A of the track, de-homogenised, then the three rejection tests.
//
// Host- and device-compilable, in the style of p3p.h: plain C++, nothing from HIP but the qualifiers.  triangulate_kernel gives a
// track to a lane; tests/plan/test_triangulate.cpp runs the same function on the CPU.
//
// The singular vector is taken from A itself, never from the Gram matrix A^T A: the fourth column of A grows with the distance of the
// scene from the world origin, cond(A) reaches 1e6 one kilometre out at a 0.05 m baseline, and the eigenvector of A^T A is then only
// good to cond(A)^2 * 1e-16 — centimetres (DESIGN.md "Triangulation: singular vector of A, not of A^T A").  Two backward-stable steps:
//   1. every row of A is rotated into a 4 x 4 upper-triangular R as it is formed (Givens; R^T R = A^T A without ever forming it), so a
//      track of any length costs the lane 10 doubles;
//   2. one-sided (Hestenes) Jacobi on R: column pairs of G = R V are rotated until they are orthogonal; the columns of V are the right
//      singular vectors, the column norms of G the singular values.
// That is backward stable, but a long track's R has been through two rotations per view, and their roundings add up to several times
// what a Householder QR of the whole of A commits (measured: up to 20 x LAPACK's error at 40 views).  So
//   3. the rows are formed once more and, expressed in the basis V, summed into the 4 x 4 matrix (A V)^T (A V).  It is nearly diagonal
//      and graded — an entry's error is an ulp of the product of ITS two singular values, not of the largest — which is where
//      Jacobi's eigenvectors are accurate to the ulp; a sweep or two of two-sided rotations finish V.  (On A itself, without step 2,
//      this would be the Gram route again: the grading only exists once V is nearly right.)
// Every index is compile-time (unrolled loops, templates): R, G, V and the refinement's matrix stay in registers.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define BSG_TRI_FN __host__ __device__ __forceinline__
#define BSG_TRI_UNROLL _Pragma("unroll")
#else
#define BSG_TRI_FN inline
#define BSG_TRI_UNROLL
#endif

namespace bsg {

// status of a track (bsgpu_triangulate, include/bsgpu.h)
enum { TRI_OK = 0, TRI_TOO_FEW_VIEWS = 1, TRI_BEHIND_CAMERA = 2, TRI_TOO_FAR = 3, TRI_REPROJECTION = 4, TRI_AT_INFINITY = 5 };

// Eigen::Quaternion::toRotationMatrix() (no normalisation), row-major: quat_to_rot of bsgpu_device.h, which the host cannot include
BSG_TRI_FN void tri_quat_to_rot(const double q[4], double R[9]) {
  const double tx = 2.0 * q[1], ty = 2.0 * q[2], tz = 2.0 * q[3];
  const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
  const double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
  const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

// rows 0..2 of T_camera_world = T_cam_baselink * T_world_baselink^-1, row-major 3x4.  Cam: fx fy cx cy R[9] t[3] (DevCamera)
template <class Cam>
BSG_TRI_FN void tri_camera_from_world(const double* __restrict__ x, int xq, int xp, const Cam& cam, double T[12]) {
  const double q[4] = {x[xq], x[xq + 1], x[xq + 2], x[xq + 3]};
  const double t[3] = {x[xp], x[xp + 1], x[xp + 2]};
  double Rwb[9];
  tri_quat_to_rot(q, Rwb);
  // R = Rcb * Rwb^T ;  tt = tcb - R t
  BSG_TRI_UNROLL
  for (int i = 0; i < 3; ++i) {
    BSG_TRI_UNROLL
    for (int j = 0; j < 3; ++j)
      T[4 * i + j] = cam.R[3 * i] * Rwb[3 * j] + cam.R[3 * i + 1] * Rwb[3 * j + 1] + cam.R[3 * i + 2] * Rwb[3 * j + 2];
    T[4 * i + 3] = cam.t[i] - (T[4 * i] * t[0] + T[4 * i + 1] * t[1] + T[4 * i + 2] * t[2]);
  }
}

// R <- the triangular factor of [R; r^T]: four Givens rotations, each zeroing one entry of the new row against the diagonal
BSG_TRI_FN void tri_givens_row(double R[4][4], double r[4]) {
  BSG_TRI_UNROLL
  for (int k = 0; k < 4; ++k) {
    const double a = R[k][k], b = r[k];
    if (b != 0.0) {
      const double rho = sqrt(a * a + b * b), c = a / rho, s = b / rho;
      R[k][k] = rho;
      BSG_TRI_UNROLL
      for (int j = k + 1; j < 4; ++j) {
        const double rk = R[k][j], rj = r[j];
        R[k][j] = c * rk + s * rj;
        r[j] = c * rj - s * rk;
      }
    }
  }
}

// One Hestenes step on the columns P < Q of G (and of V): true if they were rotated.  The pair counts as orthogonal when its cosine is
// below one ulp; a rotation by less than an ulp of angle (a column that is rounding noise against a far larger one) changes nothing.
template <int P, int Q>
BSG_TRI_FN bool tri_hestenes(double g[4][4], double v[4][4]) {
  double alpha = 0.0, beta = 0.0, gamma = 0.0;
  BSG_TRI_UNROLL
  for (int k = 0; k < 4; ++k) { alpha += g[k][P] * g[k][P]; beta += g[k][Q] * g[k][Q]; gamma += g[k][P] * g[k][Q]; }
  if (gamma == 0.0 || gamma * gamma <= (2.3e-16 * 2.3e-16) * alpha * beta) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
  if (fabs(t) < 1.2e-16) return false;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  BSG_TRI_UNROLL
  for (int k = 0; k < 4; ++k) {
    const double gp = g[k][P], gq = g[k][Q];
    g[k][P] = c * gp - s * gq;
    g[k][Q] = s * gp + c * gq;
    const double vp = v[k][P], vq = v[k][Q];
    v[k][P] = c * vp - s * vq;
    v[k][Q] = s * vp + c * vq;
  }
  return true;
}

// v: the right singular vectors of the upper-triangular R (which is overwritten), in no particular order
BSG_TRI_FN void tri_right_singular_vectors(double g[4][4], double v[4][4]) {
  BSG_TRI_UNROLL
  for (int i = 0; i < 4; ++i)
    BSG_TRI_UNROLL
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  // cyclic sweeps converge quadratically; a 4 x 4 takes 3 to 6 of them, the limit only bounds the work on pathological input
  for (int sweep = 0; sweep < 16; ++sweep) {
    bool any = tri_hestenes<0, 1>(g, v);
    any |= tri_hestenes<0, 2>(g, v); any |= tri_hestenes<0, 3>(g, v);
    any |= tri_hestenes<1, 2>(g, v); any |= tri_hestenes<1, 3>(g, v); any |= tri_hestenes<2, 3>(g, v);
    if (!any) break;
  }
}

// One two-sided Jacobi step on the symmetric a, the rotation accumulated into v: true if (P, Q) was rotated
template <int P, int Q>
BSG_TRI_FN bool tri_jacobi(double a[4][4], double v[4][4]) {
  const double apq = a[P][Q];
  if (apq == 0.0 || apq * apq <= (1.2e-16 * 1.2e-16) * a[P][P] * a[Q][Q]) return false;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  BSG_TRI_UNROLL
  for (int k = 0; k < 4; ++k) {   // A <- A G
    const double akp = a[k][P], akq = a[k][Q];
    a[k][P] = c * akp - s * akq;
    a[k][Q] = s * akp + c * akq;
  }
  BSG_TRI_UNROLL
  for (int k = 0; k < 4; ++k) {   // A <- G^T A
    const double apk = a[P][k], aqk = a[Q][k];
    a[P][k] = c * apk - s * aqk;
    a[Q][k] = s * apk + c * aqk;
  }
  a[P][Q] = a[Q][P] = 0.0;
  BSG_TRI_UNROLL
  for (int k = 0; k < 4; ++k) {
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq;
    v[k][Q] = s * vkp + c * vkq;
  }
  return true;
}

// the two DLT rows of one view: m.x * T.row(2) - m.z * T.row(0), m.y * T.row(2) - m.z * T.row(1), m the pixel's unit bearing
template <class Cam>
BSG_TRI_FN void tri_view_rows(const double* __restrict__ x, int xq, int xp, const Cam& cam, double zx, double zy, double r0[4],
                              double r1[4]) {
  double T[12];
  tri_camera_from_world(x, xq, xp, cam, T);
  double m[3] = {(zx - cam.cx) / cam.fx, (zy - cam.cy) / cam.fy, 1.0};
  const double inv = 1.0 / sqrt(m[0] * m[0] + m[1] * m[1] + 1.0);
  m[0] *= inv; m[1] *= inv; m[2] *= inv;
  BSG_TRI_UNROLL
  for (int k = 0; k < 4; ++k) {
    r0[k] = m[0] * T[8 + k] - m[2] * T[k];
    r1[k] = m[1] * T[8 + k] - m[2] * T[4 + k];
  }
}

// Track of the observations [beg, end): pose_off[o] = (.x, .y) value offsets of the keyframe's orientation and position in x,
// pix[o] = (.x, .y) the measured pixel.  Writes the point (zero when there are fewer than two views) and returns the status.
template <class Off, class Pix, class Cam>
BSG_TRI_FN int triangulate_track(int beg, int end, const Off* __restrict__ pose_off, const Pix* __restrict__ pix,
                                 const double* __restrict__ x, const Cam& cam, int truncate, double max_dist, double max_reproj,
                                 double P[3]) {
  P[0] = P[1] = P[2] = 0.0;
  if (end - beg < 2) return TRI_TOO_FEW_VIEWS;
  double R[4][4];
  BSG_TRI_UNROLL
  for (int i = 0; i < 4; ++i)
    BSG_TRI_UNROLL
    for (int j = 0; j < 4; ++j) R[i][j] = 0.0;
  for (int o = beg; o < end; ++o) {
    const Off po = pose_off[o];
    const Pix z = pix[o];
    double zx = z.x, zy = z.y;
    if (truncate) { zx = trunc(zx); zy = trunc(zy); }
    double r0[4], r1[4];
    tri_view_rows(x, po.x, po.y, cam, zx, zy, r0, r1);
    tri_givens_row(R, r0);
    tri_givens_row(R, r1);
  }
  double v[4][4];
  tri_right_singular_vectors(R, v);
  // refinement: a = (A V)^T (A V) from the rows themselves, then Jacobi on it
  double a[4][4];
  BSG_TRI_UNROLL
  for (int i = 0; i < 4; ++i)
    BSG_TRI_UNROLL
    for (int j = 0; j < 4; ++j) a[i][j] = 0.0;
  for (int o = beg; o < end; ++o) {
    const Off po = pose_off[o];
    const Pix z = pix[o];
    double zx = z.x, zy = z.y;
    if (truncate) { zx = trunc(zx); zy = trunc(zy); }
    double r0[4], r1[4], y0[4], y1[4];
    tri_view_rows(x, po.x, po.y, cam, zx, zy, r0, r1);
    BSG_TRI_UNROLL
    for (int j = 0; j < 4; ++j) {
      y0[j] = r0[0] * v[0][j] + r0[1] * v[1][j] + r0[2] * v[2][j] + r0[3] * v[3][j];
      y1[j] = r1[0] * v[0][j] + r1[1] * v[1][j] + r1[2] * v[2][j] + r1[3] * v[3][j];
    }
    BSG_TRI_UNROLL
    for (int i = 0; i < 4; ++i)
      BSG_TRI_UNROLL
      for (int j = 0; j < 4; ++j) a[i][j] += y0[i] * y0[j] + y1[i] * y1[j];
  }
  for (int sweep = 0; sweep < 8; ++sweep) {
    bool any = tri_jacobi<0, 1>(a, v);
    any |= tri_jacobi<0, 2>(a, v); any |= tri_jacobi<0, 3>(a, v);
    any |= tri_jacobi<1, 2>(a, v); any |= tri_jacobi<1, 3>(a, v); any |= tri_jacobi<2, 3>(a, v);
    if (!any) break;
  }
  // singular vector of the smallest singular value (selects instead of dynamic indexing keep v in registers)
  double best = a[0][0];
  double h[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
  BSG_TRI_UNROLL
  for (int j = 1; j < 4; ++j) {
    const bool lt = a[j][j] < best;
    best = lt ? a[j][j] : best;
    BSG_TRI_UNROLL
    for (int k = 0; k < 4; ++k) h[k] = lt ? v[k][j] : h[k];
  }
  if (h[3] == 0.0) return TRI_AT_INFINITY;
  P[0] = h[0] / h[3]; P[1] = h[1] / h[3]; P[2] = h[2] / h[3];
  for (int o = beg; o < end; ++o) {
    const Off po = pose_off[o];
    const Pix z = pix[o];
    double zx = z.x, zy = z.y;
    if (truncate) { zx = trunc(zx); zy = trunc(zy); }
    double T[12];
    tri_camera_from_world(x, po.x, po.y, cam, T);
    double pc[3];
    BSG_TRI_UNROLL
    for (int i = 0; i < 3; ++i) pc[i] = T[4 * i] * P[0] + T[4 * i + 1] * P[1] + T[4 * i + 2] * P[2] + T[4 * i + 3];
    if (pc[2] < 0.0) return TRI_BEHIND_CAMERA;
    if (max_dist > 0.0 && sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]) > max_dist) return TRI_TOO_FAR;
    if (max_reproj > 0.0) {
      const double du = zx - (cam.fx * pc[0] / pc[2] + cam.cx), dv = zy - (cam.fy * pc[1] / pc[2] + cam.cy);
      if (!(sqrt(du * du + dv * dv) <= max_reproj)) return TRI_REPROJECTION;
    }
  }
  return TRI_OK;
}

}  // namespace bsg
