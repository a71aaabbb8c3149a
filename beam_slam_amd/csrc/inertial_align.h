// Visual-inertial alignment of one candidate path (bsgpu_inertial_alignment, k_align.hip): what SLAMInitialization does between the
// up-to-scale camera path and the first large solve —
//   imu::EstimateParameters            bs_models/src/lib/imu/inertial_alignment.cpp:4-112    frames, the three Integrate passes
//   imu::ImuObservability              :114-136   excitation
//   imu::EstimateGyroBias              :138-161   3 x 3 least squares on the rotation residuals
//   imu::EstimateGravityScaleVelocities :163-202  linear least squares in gravity, scale and a velocity per frame
//   the scale gate and AlignPathAndVelocities      bs_models/src/slam_initialization.cpp:312-316, :400-431
// restated as include/bsgpu.h states the contract (steps (a)-(f) there).  Host- and device-compilable in the style of p3p.h and
// preint_core.h: plain C++, nothing from HIP but the qualifiers.  align_path is written for `nlanes` cooperating lanes that share the
// scratch arrays and meet at sy.barrier() / sy.any(): the kernel passes a workgroup, tests/plan/test_align.cpp and the timing script
// one lane with an empty barrier.  Work that is per frame (ownership, the deltas, the rotation residual, the right-hand sides, the
// final alignment) is striped over the lanes; every sum over frames and the least-squares sweep run on lane 0 in frame order, so the
// result does not depend on the number of lanes.
//
// The least squares (e) is solved by Householder reflections, never through the normal equations.  With the unknowns ordered
// v_0 .. v_{N-1}, g, s the matrix is block-bidiagonal in the velocities with a four-column border: pair i = (frame i, frame i + 1)
// contributes six rows over v_i, v_{i+1} and the border.  Step i stacks these six rows under the rows carried from step i - 1 (at
// most seven, over v_i and the border), triangularises the at most 13 x 10 block, files its first three rows (3 x 10 and the
// right-hand side: v_i is finished) and carries the next seven (over v_{i+1} and the border); what lies below is residual.  The last
// step's carried rows are the 7 x 7 triangle of v_{N-1}, g, s; back-substitution walks the filed rows backwards.
#pragma once
#include <cmath>

#include "preint_core.h"

namespace bsg {

enum { ALIGN_OK = 0, ALIGN_TOO_FEW_FRAMES = 1, ALIGN_BAD_IMU = 2, ALIGN_NOT_EXCITED = 3, ALIGN_RANK_DEFICIENT = 4, ALIGN_SCALE_REJECTED = 5 };

constexpr double kGravityNominal = 9.80665;                 // GRAVITY_NOMINAL; GRAVITY_WORLD = (0, 0, -9.80665)
constexpr double kAlignEps = 2.220446049250313e-16;         // 2^-52
constexpr int kAlignRhs = kPreintDelta;                     // per-frame scratch: the delta, then 12 doubles (J^T J, J^T r; later R dp, R dv),
constexpr int kAlignRows = kPreintDelta + 12;               // then the frame's three filed rows of the triangular factor (3 x 11)
constexpr int kAlignFrameScratch = kPreintDelta + 12 + 33;
constexpr int kAlignPathScratch = 4;                        // per-path scratch: the alignment quaternion
constexpr int kAlignWork = 13 * 11;                         // lane 0's block of the least-squares sweep: LDS in the kernel

struct AlignSerial {                                        // one lane: nothing to wait for
  BSG_PRE_FN int any(int x) const { return x; }
  BSG_PRE_FN void barrier() const {}
};

struct AlignPath {
  int n;                                   // frames
  const double *tf, *qf, *pf;              // the path's frames: stamp, T_WORLD_BASELINK (wxyz, xyz)
  int i0, i1;                              // the path's IMU samples [i0, i1) of t / w / a
  const double *t, *w, *a;
  int bridge_gap;
  double min_excitation;
  int apply_scale;
  double scale_min, scale_max, rank_tol;
  double *gravity, *bg, *scale, *excitation;
  int* gyro_rank;
  double *velocity, *q_out, *p_out, *v_out;
  int* status;
  int* own;                                // scratch, n + 1: frame f owns the samples [own[f], own[f + 1])
  double* fs;                              // scratch, n x kAlignFrameScratch
  double* ps;                              // scratch, kAlignPathScratch
  double* ws;                              // lane 0's workspace, kAlignWork
};

BSG_PRE_FN void align_rotate(const double q[4], const double v[3], double o[3]) {
  const M3 R = pre_quat_to_rot(q);
  for (int i = 0; i < 3; ++i) o[i] = R.m[3 * i] * v[0] + R.m[3 * i + 1] * v[1] + R.m[3 * i + 2] * v[2];
}

// Log of the rotation of a unit quaternion: the rotation vector with its angle in [0, pi].  [EXT] beam::RToLieAlgebra goes through
// the rotation matrix; the vector is taken from the quaternion here, which is the same map without the matrix's cancellation.
BSG_PRE_FN void align_quat_log(const double q_in[4], double r[3]) {
  double q[4] = {q_in[0], q_in[1], q_in[2], q_in[3]};
  if (q[0] < 0.0) for (int i = 0; i < 4; ++i) q[i] = -q[i];
  const double n = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double k = n > 0.0 ? 2.0 * atan2(n, q[0]) / n : 2.0;
  for (int i = 0; i < 3; ++i) r[i] = k * q[1 + i];
}

// Eigen::Quaterniond::FromTwoVectors(a, b) for 1 + cos > 2^-52; for antiparallel vectors the half turn about normalize(a x e_k),
// e_k the coordinate axis of a's smallest |component| (Eigen takes the axis from an SVD there).
BSG_PRE_FN void align_from_two_vectors(const double a[3], const double b[3], double q[4]) {
  const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  const double u[3] = {a[0] / na, a[1] / na, a[2] / na}, v[3] = {b[0] / nb, b[1] / nb, b[2] / nb};
  const double c = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
  if (1.0 + c > kAlignEps) {
    const double s = sqrt(2.0 * (1.0 + c));
    q[0] = 0.5 * s;
    q[1] = (u[1] * v[2] - u[2] * v[1]) / s; q[2] = (u[2] * v[0] - u[0] * v[2]) / s; q[3] = (u[0] * v[1] - u[1] * v[0]) / s;
  } else {
    int k = 0;
    if (fabs(u[1]) < fabs(u[k])) k = 1;
    if (fabs(u[2]) < fabs(u[k])) k = 2;
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    const double x[3] = {u[1] * e[2] - u[2] * e[1], u[2] * e[0] - u[0] * e[2], u[0] * e[1] - u[1] * e[0]};
    const double nx = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    q[0] = 0.0; q[1] = x[0] / nx; q[2] = x[1] / nx; q[3] = x[2] / nx;
  }
}

// x = A^+ b for a symmetric 3 x 3 A (row-major) by a cyclic Jacobi eigen-decomposition; an eigenvalue <= 3 * 2^-52 * lambda_max
// counts as zero ([EXT] Eigen::JacobiSVD's default threshold, recalled).  Returns the number of eigenvalues kept.
BSG_PRE_FN int align_pinv_solve3(const double A_in[9], const double b[3], double x[3]) {
  double A[3][3], V[3][3];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { A[i][j] = 0.5 * (A_in[3 * i + j] + A_in[3 * j + i]); V[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p) for (int q = p + 1; q < 3; ++q) {
      const double apq = A[p][q];
      if (apq == 0.0) continue;
      if (fabs(A[p][p]) + fabs(apq) == fabs(A[p][p]) && fabs(A[q][q]) + fabs(apq) == fabs(A[q][q])) { A[p][q] = A[q][p] = 0.0; continue; }
      rotated = true;
      const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
      const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
      const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
      const int r = 3 - p - q;
      const double arp = A[r][p], arq = A[r][q];
      A[p][p] -= tt * apq; A[q][q] += tt * apq;
      A[p][q] = A[q][p] = 0.0;
      A[r][p] = A[p][r] = c * arp - s * arq;
      A[r][q] = A[q][r] = s * arp + c * arq;
      for (int i = 0; i < 3; ++i) { const double vp = V[i][p], vq = V[i][q]; V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq; }
    }
    if (!rotated) break;
  }
  const double lmax = fmax(A[0][0], fmax(A[1][1], A[2][2]));
  int rank = 0;
  x[0] = x[1] = x[2] = 0.0;
  for (int k = 0; k < 3; ++k) {
    if (!(A[k][k] > 3.0 * kAlignEps * lmax)) continue;
    ++rank;
    const double f = (V[0][k] * b[0] + V[1][k] * b[1] + V[2][k] * b[2]) / A[k][k];
    for (int i = 0; i < 3; ++i) x[i] += f * V[i][k];
  }
  return rank;
}

// Householder triangularisation of the leading min(m, 10) columns of W (m x 11, the last column the right-hand side), in place.
// A column that is already zero below and on the diagonal keeps its zero pivot.
BSG_PRE_FN void align_householder(double (*W)[11], int m) {
  for (int c = 0; c < 10 && c < m; ++c) {
    double nn = 0.0;
    for (int r = c + 1; r < m; ++r) nn += W[r][c] * W[r][c];
    if (nn == 0.0) continue;                                  // nothing below the diagonal
    const double x0 = W[c][c], nrm = sqrt(x0 * x0 + nn), alpha = x0 > 0.0 ? -nrm : nrm;
    const double v0 = x0 - alpha, beta = 1.0 / (nn + v0 * v0);  // H = I - 2 beta v v^T,  v = (v0, W[c+1..][c])
    for (int j = c + 1; j < 11; ++j) {
      double s = v0 * W[c][j];
      for (int r = c + 1; r < m; ++r) s += W[r][c] * W[r][j];
      s *= 2.0 * beta;
      if (s == 0.0) continue;
      W[c][j] -= s * v0;
      for (int r = c + 1; r < m; ++r) W[r][j] -= s * W[r][c];
    }
    W[c][c] = alpha;
    for (int r = c + 1; r < m; ++r) W[r][c] = 0.0;
  }
}

// (e) on lane 0: the sweep over the pairs and the back-substitution.  fs holds per frame f >= 1 dt at [0] and R(q_{f-1}) dp_f,
// R(q_{f-1}) dv_f at [kAlignRhs ..]; the filed rows of frame i go to fs[i][kAlignRows ..].  x: g (3), s; vel: n x 3.  false: the
// triangular factor's smallest |diagonal| is not above rank_tol x its largest.  W: the 13 x 11 working block.
BSG_PRE_FN bool align_least_squares(int n, const double* pf, double* fs, double rank_tol, double x[4], double* vel, double (*W)[11]) {
  int c = 0;
  double dmin = INFINITY, dmax = 0.0;
  auto diag = [&](double d) { d = fabs(d); if (!(d >= dmin)) dmin = d; if (!(d <= dmax)) dmax = d; };
  for (int i = 0; i + 1 < n; ++i) {
    const double* fj = fs + (size_t)(i + 1) * kAlignFrameScratch;
    const double dt = fj[0];
    for (int r = c; r < c + 6; ++r) for (int j = 0; j < 11; ++j) W[r][j] = 0.0;
    for (int k = 0; k < 3; ++k) {
      W[c + k][k] = -dt; W[c + k][6 + k] = -0.5 * dt * dt; W[c + k][9] = pf[3 * (i + 1) + k] - pf[3 * i + k]; W[c + k][10] = fj[kAlignRhs + k];
      W[c + 3 + k][k] = -1.0; W[c + 3 + k][3 + k] = 1.0; W[c + 3 + k][6 + k] = -dt; W[c + 3 + k][10] = fj[kAlignRhs + 3 + k];
    }
    const int m = c + 6;
    align_householder(W, m);
    double* rows = fs + (size_t)i * kAlignFrameScratch + kAlignRows;
    for (int r = 0; r < 3; ++r) { diag(W[r][r]); for (int j = 0; j < 11; ++j) rows[11 * r + j] = W[r][j]; }
    c = (m < 10 ? m : 10) - 3;
    if (i + 2 < n)
      for (int r = 0; r < c; ++r) {
        for (int j = 0; j < 3; ++j) { W[r][j] = W[r + 3][3 + j]; W[r][3 + j] = 0.0; }
        for (int j = 6; j < 11; ++j) W[r][j] = W[r + 3][j];
      }
  }
  if (c != 7) return false;                                  // (n >= 4 always gets here with the full triangle)
  for (int r = 3; r < 10; ++r) diag(W[r][r]);
  if (!(dmin > rank_tol * dmax)) return false;
  double y[10];
  for (int r = 9; r >= 3; --r) {
    double s = W[r][10];
    for (int j = r + 1; j < 10; ++j) s -= W[r][j] * y[j];
    y[r] = s / W[r][r];
  }
  for (int k = 0; k < 4; ++k) x[k] = y[6 + k];
  for (int k = 0; k < 3; ++k) vel[3 * (n - 1) + k] = y[3 + k];
  for (int i = n - 2; i >= 0; --i) {
    const double* rows = fs + (size_t)i * kAlignFrameScratch + kAlignRows;
    for (int r = 2; r >= 0; --r) {
      double s = rows[11 * r + 10];
      for (int j = r + 1; j < 3; ++j) s -= rows[11 * r + j] * vel[3 * i + j];
      for (int j = 0; j < 3; ++j) s -= rows[11 * r + 3 + j] * vel[3 * (i + 1) + j];
      for (int j = 0; j < 4; ++j) s -= rows[11 * r + 6 + j] * x[j];
      vel[3 * i + r] = s / rows[11 * r + r];
    }
  }
  return true;
}

template <class Sync>
BSG_PRE_FN void align_path(const AlignPath& P, int lane, int nlanes, const Sync& sy) {
  const int N = P.n;
  const double zero3[3] = {0.0, 0.0, 0.0};
  // every output has a value whatever the status: no estimate, the aligned path is the input
  for (int f = lane; f < N; f += nlanes) {
    for (int i = 0; i < 4; ++i) P.q_out[4 * f + i] = P.qf[4 * f + i];
    for (int i = 0; i < 3; ++i) { P.p_out[3 * f + i] = P.pf[3 * f + i]; P.velocity[3 * f + i] = 0.0; P.v_out[3 * f + i] = 0.0; }
  }
  if (lane == 0) {
    for (int i = 0; i < 3; ++i) { P.gravity[i] = 0.0; P.bg[i] = 0.0; }
    *P.scale = 1.0; *P.excitation = 0.0; *P.gyro_rank = 0;
    *P.status = ALIGN_OK;
  }
  if (N < 4) { if (lane == 0) *P.status = ALIGN_TOO_FEW_FRAMES; return; }

  // (a) the inputs, then who owns which samples
  int bad = 0;
  for (int f = lane; f < N; f += nlanes) {
    bool ok = std::isfinite(P.tf[f]);
    for (int i = 0; i < 4; ++i) ok = ok && std::isfinite(P.qf[4 * f + i]);
    for (int i = 0; i < 3; ++i) ok = ok && std::isfinite(P.pf[3 * f + i]);
    if (!ok) bad = 1;
  }
  for (int s = P.i0 + lane; s < P.i1; s += nlanes) {
    bool ok = std::isfinite(P.t[s]);
    for (int i = 0; i < 3; ++i) ok = ok && std::isfinite(P.w[3 * s + i]) && std::isfinite(P.a[3 * s + i]);
    if (s + 1 < P.i1) ok = ok && P.t[s + 1] > P.t[s];
    if (!ok) bad = 1;
  }
  if (P.i1 - P.i0 < 2 || !(P.t[P.i0 + 1] <= P.tf[0])) bad = 1;        // :23-30: two samples before the first pose
  bad = sy.any(bad);
  if (bad) { if (lane == 0) *P.status = ALIGN_BAD_IMU; return; }
  if (lane == 0) P.own[0] = P.i0;
  for (int f = lane; f < N; f += nlanes) {                             // first sample not before the frame's stamp
    int lo = P.i0, hi = P.i1;
    while (lo < hi) { const int mid = lo + (hi - lo) / 2; if (P.t[mid] < P.tf[f]) lo = mid + 1; else hi = mid; }
    P.own[f + 1] = lo;
  }
  sy.barrier();
  for (int f = lane; f < N; f += nlanes) if (P.own[f + 1] <= P.own[f]) bad = 1;   // :50-55
  bad = sy.any(bad);
  if (bad) { if (lane == 0) *P.status = ALIGN_BAD_IMU; return; }

  // (b) the deltas at zero bias, (d)'s terms per frame
  auto integrate = [&](int f, const double* bg) {
    preintegrate_delta(P.own[f], P.own[f + 1], P.t, P.w, P.a, P.tf[f], bg, zero3, (P.bridge_gap && f >= 1) ? P.own[f] - 1 : -1,
                       f >= 1 ? P.tf[f - 1] : 0.0, P.fs + (size_t)f * kAlignFrameScratch);
  };
  for (int f = lane; f < N; f += nlanes) {
    integrate(f, zero3);
    double* d = P.fs + (size_t)f * kAlignFrameScratch;
    if (!(d[0] > 0.0)) bad = 1;                                        // Increment asserts dt > 0 (preintegrator.cpp:30)
    if (f == 0) continue;
    const double* J = d + 11;
    double qi[4], qc[4], e[4], r[3];
    pre_quat_mul(P.qf + 4 * (f - 1), d + 1, qi);
    qc[0] = qi[0]; qc[1] = -qi[1]; qc[2] = -qi[2]; qc[3] = -qi[3];
    pre_quat_mul(qc, P.qf + 4 * f, e);
    const double ne = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);
    for (int i = 0; i < 4; ++i) e[i] /= ne;
    align_quat_log(e, r);
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) d[kAlignRhs + 3 * i + j] = J[i] * J[j] + J[3 + i] * J[3 + j] + J[6 + i] * J[6 + j];
      d[kAlignRhs + 9 + i] = J[i] * r[0] + J[3 + i] * r[1] + J[6 + i] * r[2];
    }
  }
  bad = sy.any(bad);                                                    // (a barrier as well)
  if (bad) { if (lane == 0) *P.status = ALIGN_BAD_IMU; return; }

  // (c), (d) on lane 0, in frame order
  if (lane == 0) {
    double sum[3] = {0.0, 0.0, 0.0}, var = 0.0;                         // (the reference's sum starts from uninitialised memory)
    for (int f = 0; f < N; ++f) { const double* d = P.fs + (size_t)f * kAlignFrameScratch; for (int i = 0; i < 3; ++i) sum[i] += d[8 + i] / d[0]; }
    for (int i = 0; i < 3; ++i) sum[i] = sum[i] * 1.0 / (N - 1);
    for (int f = 0; f < N; ++f) {
      const double* d = P.fs + (size_t)f * kAlignFrameScratch;
      double s = 0.0;
      for (int i = 0; i < 3; ++i) { const double e = d[8 + i] / d[0] - sum[i]; s += e * e; }
      var += s;
    }
    const double exc = sqrt(var / (N - 1));
    *P.excitation = exc;
    if (exc < P.min_excitation) {
      *P.status = ALIGN_NOT_EXCITED;
    } else if (!std::isfinite(exc)) {
      *P.status = ALIGN_BAD_IMU;
    } else {
      double A[9], b[3] = {0.0, 0.0, 0.0}, bg[3];
      for (int i = 0; i < 9; ++i) A[i] = 0.0;
      for (int f = 1; f < N; ++f) {
        const double* d = P.fs + (size_t)f * kAlignFrameScratch + kAlignRhs;
        for (int i = 0; i < 9; ++i) A[i] += d[i];
        for (int i = 0; i < 3; ++i) b[i] += d[9 + i];
      }
      *P.gyro_rank = align_pinv_solve3(A, b, bg);
      for (int i = 0; i < 3; ++i) P.bg[i] = bg[i];
    }
  }
  sy.barrier();
  if (*P.status != ALIGN_OK) return;

  // (e) the deltas at (bg, 0); frame 0's is in no equation
  const double bg[3] = {P.bg[0], P.bg[1], P.bg[2]};
  for (int f = 1 + lane; f < N; f += nlanes) {
    integrate(f, bg);
    double* d = P.fs + (size_t)f * kAlignFrameScratch;
    align_rotate(P.qf + 4 * (f - 1), d + 5, d + kAlignRhs);
    align_rotate(P.qf + 4 * (f - 1), d + 8, d + kAlignRhs + 3);
  }
  sy.barrier();
  if (lane == 0) {
    double x[4];
    if (!align_least_squares(N, P.pf, P.fs, P.rank_tol, x, P.velocity, reinterpret_cast<double (*)[11]>(P.ws))) {
      for (int i = 0; i < 3 * N; ++i) P.velocity[i] = 0.0;
      *P.status = ALIGN_RANK_DEFICIENT;
    } else {
      const double ng = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
      for (int i = 0; i < 3; ++i) P.gravity[i] = x[i] / ng * kGravityNominal;
      *P.scale = x[3];
      // (f) the gate, then the rotation that takes the estimated gravity onto the world's
      if (!(ng > 0.0) || !std::isfinite(ng)) {
        for (int i = 0; i < 3; ++i) P.gravity[i] = 0.0;
        *P.status = ALIGN_RANK_DEFICIENT;
      } else if (P.apply_scale && !(x[3] >= P.scale_min && x[3] <= P.scale_max)) {
        *P.status = ALIGN_SCALE_REJECTED;
      } else {
        const double gw[3] = {0.0, 0.0, -kGravityNominal};
        align_from_two_vectors(P.gravity, gw, P.ps);
      }
    }
  }
  sy.barrier();
  const int st = *P.status;
  if (st == ALIGN_SCALE_REJECTED)
    for (int f = lane; f < N; f += nlanes) for (int i = 0; i < 3; ++i) P.v_out[3 * f + i] = P.velocity[3 * f + i];
  if (st != ALIGN_OK) return;
  const double qa[4] = {P.ps[0], P.ps[1], P.ps[2], P.ps[3]};
  const double sc = P.apply_scale ? *P.scale : 1.0;
  for (int f = lane; f < N; f += nlanes) {
    double po[3];
    pre_quat_mul(qa, P.qf + 4 * f, P.q_out + 4 * f);
    align_rotate(qa, P.pf + 3 * f, po);
    for (int i = 0; i < 3; ++i) P.p_out[3 * f + i] = P.apply_scale ? sc * po[i] : po[i];
    align_rotate(qa, P.velocity + 3 * f, P.v_out + 3 * f);
  }
}

// Path k of a bsgpu_inertial_alignment call.  own: total frames + n_paths ints; fs: total frames x kAlignFrameScratch; ps: n_paths x
// kAlignPathScratch; ws: kAlignWork doubles of the caller's (shared by the lanes of the path, not by paths that run at once).
template <class Sync>
BSG_PRE_FN void align_path_of_call(int k, const int* frame_start, const double* t_frame, const double* q_frame, const double* p_frame,
                                   const int* imu_range, const double* t, const double* w, const double* a, int bridge_gap,
                                   double min_excitation, int apply_scale, double scale_min, double scale_max, double rank_tol,
                                   double* gravity, double* bg, double* scale, double* excitation, int* gyro_rank, double* velocity,
                                   double* q_out, double* p_out, double* v_out, int* status, int* own, double* fs, double* ps, double* ws,
                                   int lane, int nlanes, const Sync& sy) {
  const int f0 = frame_start[k];
  AlignPath P;
  P.n = frame_start[k + 1] - f0;
  P.tf = t_frame + f0; P.qf = q_frame + 4 * (size_t)f0; P.pf = p_frame + 3 * (size_t)f0;
  P.i0 = imu_range[2 * k]; P.i1 = imu_range[2 * k + 1];
  P.t = t; P.w = w; P.a = a;
  P.bridge_gap = bridge_gap; P.min_excitation = min_excitation; P.apply_scale = apply_scale;
  P.scale_min = scale_min; P.scale_max = scale_max; P.rank_tol = rank_tol;
  P.gravity = gravity + 3 * (size_t)k; P.bg = bg + 3 * (size_t)k; P.scale = scale + k; P.excitation = excitation + k; P.gyro_rank = gyro_rank + k;
  P.velocity = velocity + 3 * (size_t)f0; P.q_out = q_out + 4 * (size_t)f0; P.p_out = p_out + 3 * (size_t)f0; P.v_out = v_out + 3 * (size_t)f0;
  P.status = status + k;
  P.own = own + f0 + k; P.fs = fs + (size_t)f0 * kAlignFrameScratch; P.ps = ps + (size_t)k * kAlignPathScratch;
  P.ws = ws;
  align_path(P, lane, nlanes, sy);
}

}  // namespace bsg
