// DOGLEG (dogleg.h; [EXT] ceres DoglegStrategy with TRADITIONAL_DOGLEG): the vector work of one step on the unscaled system.
//   dl_vec_kernel    v = g / c, the Gauss-Newton step kept aside, and the partials of |g'|^2, |gn'|^2, g'.gn'
//   dl_step_kernel   delta = a v + b delta_gn and the partials of |step'|^2 = sum c delta^2
//   dl_jv_*_kernel   J u for a full tangent vector u over every factor class of the exact paths (Euclidean-landmark reprojection factors,
//                    pose-only groups, dense priors): per-workgroup partials of |J u|^2 and (J u).r, with the Jacobians and residuals as the
//                    evaluation stored them (robustified: the loss corrector is applied).  |J u|^2 is summed directly, not as -2 (mcc + u.g),
//                    which cancels.
//   dl_sum_kernel    the partials of a launch added up by one workgroup in a fixed order: a step gives the same bits run to run.
// None of the LM path's kernels is touched: these are launches of their own (bsgpu_solve.cpp solve_dogleg).
#include "bsgpu_device.h"

namespace bsg {

constexpr int kDlThreads = 256;

__global__ __launch_bounds__(kDlThreads) void dl_vec_kernel(int n_tan, const double* __restrict__ g, const double* __restrict__ dcl,
                                                            const double* __restrict__ delta_gn, double* __restrict__ v, double* __restrict__ gn_keep,
                                                            double* __restrict__ part) {
  __shared__ double sred[4];
  const int j = blockIdx.x * kDlThreads + threadIdx.x;
  double g2 = 0.0, gn2 = 0.0, ggn = 0.0;
  if (j < n_tan) {
    const double c = dcl[j], gj = g[j], dj = delta_gn[j];
    gn_keep[j] = dj;
    double vj = 0.0;
    if (c > 0.0) {   // (a column without a clamped diagonal — no factor touches it — takes no part)
      vj = gj / c;
      g2 = gj * gj / c;
      gn2 = c * dj * dj;
      ggn = gj * dj;
    }
    v[j] = vj;
  }
  const double a = block_sum_256(g2, sred);
  const double b = block_sum_256(gn2, sred);
  const double d = block_sum_256(ggn, sred);
  if (threadIdx.x == 0) { part[3 * blockIdx.x] = a; part[3 * blockIdx.x + 1] = b; part[3 * blockIdx.x + 2] = d; }
}

__global__ __launch_bounds__(kDlThreads) void dl_step_kernel(int n_tan, const double* __restrict__ v, const double* __restrict__ gn, double a, double b,
                                                             const double* __restrict__ dcl, double* __restrict__ delta, double* __restrict__ part) {
  __shared__ double sred[4];
  const int j = blockIdx.x * kDlThreads + threadIdx.x;
  double s2 = 0.0;
  if (j < n_tan) {
    const double dj = a * v[j] + b * gn[j];
    delta[j] = dj;
    const double c = dcl[j];
    if (c > 0.0) s2 = c * dj * dj;
  }
  const double t = block_sum_256(s2, sred);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// reprojection factors: 8 lanes per eliminated landmark (its factors are contiguous, lm_start), then one lane per factor of a constant landmark
__global__ __launch_bounds__(kDlThreads) void dl_jv_vis_kernel(int n_lm, int n_lm_groups, int n_elim, int n, int n_pose, const int* __restrict__ lm_start,
                                                               const double* __restrict__ J, int ja, const double* __restrict__ JB, const double2* __restrict__ r,
                                                               const int* __restrict__ cam_pose, const int* __restrict__ cp_tq, const int* __restrict__ cp_tp,
                                                               const double* __restrict__ u, double* __restrict__ part) {
  __shared__ double sred[4];
  double jj = 0.0, jr = 0.0;
  auto factor = [&](int f, const double* ul) {
    const int cp = cam_pose[f], tq = cp_tq[cp], tp = cp_tp[cp];
    double j0 = 0.0, j1 = 0.0;
    if (tq >= 0)
      for (int k = 0; k < 3; ++k) { const double uv = u[tq + k]; j0 += pose_part_entry(J, JB, ja, f, 0, k) * uv; j1 += pose_part_entry(J, JB, ja, f, 1, k) * uv; }
    if (tp >= 0)
      for (int k = 0; k < 3; ++k) { const double uv = u[tp + k]; j0 += pose_part_entry(J, JB, ja, f, 0, 3 + k) * uv; j1 += pose_part_entry(J, JB, ja, f, 1, 3 + k) * uv; }
    if (ul) {
      const double* B = JB + (size_t)f * 6;
      j0 += B[0] * ul[0] + B[1] * ul[1] + B[2] * ul[2];
      j1 += B[3] * ul[0] + B[4] * ul[1] + B[5] * ul[2];
    }
    const double2 rf = r[f];
    jj += j0 * j0 + j1 * j1;
    jr += j0 * rf.x + j1 * rf.y;
  };
  if ((int)blockIdx.x < n_lm_groups) {
    const int gid = blockIdx.x * kDlThreads + threadIdx.x;
    const int l = gid >> 3, sub = gid & 7;
    if (l < n_lm) {
      const double* ul = u + n_pose + 3 * l;
      for (int f = lm_start[l] + sub; f < lm_start[l + 1]; f += 8) factor(f, ul);
    }
  } else {
    const int f = n_elim + ((int)blockIdx.x - n_lm_groups) * kDlThreads + (int)threadIdx.x;
    if (f < n) factor(f, nullptr);
  }
  const double a = block_sum_256(jj, sred);
  const double b = block_sum_256(jr, sred);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = a; part[2 * blockIdx.x + 1] = b; }
}

// a pose-only group: one lane per residual row (small_mcc_unit's layout: J is n x m x 3 nv, slot sl's tangent offset toff[f nv + sl])
__global__ __launch_bounds__(kDlThreads) void dl_jv_small_kernel(SmallGroup g, const double* __restrict__ u, double* __restrict__ part) {
  __shared__ double sred[4];
  const int id = blockIdx.x * kDlThreads + threadIdx.x;
  double jj = 0.0, jr = 0.0;
  if (id < g.n * g.m) {
    const int f = id / g.m, k = id - f * g.m, nv = g.nv, tw = 3 * nv;
    if (g.active[f]) {
      const double* Jr = g.J + ((size_t)f * g.m + k) * tw;
      double jv = 0.0;
      for (int sl = 0; sl < nv; ++sl) {
        const int t = g.toff[(size_t)f * nv + sl];
        if (t < 0) continue;
        const int w = sl == nv - 1 ? g.w_last : 3;
        for (int i = 0; i < w; ++i) jv += Jr[3 * sl + i] * u[t + i];
      }
      jj = jv * jv;
      jr = jv * g.r[(size_t)f * g.m + k];
    }
  }
  const double a = block_sum_256(jj, sred);
  const double b = block_sum_256(jr, sred);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = a; part[2 * blockIdx.x + 1] = b; }
}

// a dense prior: one wave per row
__global__ __launch_bounds__(64) void dl_jv_marg_kernel(MargDev m, const double* __restrict__ u, double* __restrict__ part) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const double* Jr = m.J + (size_t)row * m.cols;
  double jv = 0.0;
  for (int k = lane; k < m.cols; k += 64) { const int t = m.col_t[k]; if (t >= 0) jv = fma(Jr[k], u[t], jv); }
  jv = wave_sum(jv);
  if (lane == 0) { part[2 * row] = jv * jv; part[2 * row + 1] = jv * m.r[row]; }
}

// out[c] = sum over the n records of component c (records of k doubles), one workgroup, a fixed order
__global__ __launch_bounds__(kDlThreads) void dl_sum_kernel(const double* __restrict__ part, int n, int k, double* __restrict__ out) {
  __shared__ double sred[4];
  for (int c = 0; c < k; ++c) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kDlThreads) acc += part[(size_t)i * k + c];
    const double t = block_sum_256(acc, sred);
    if (threadIdx.x == 0) out[c] = t;
  }
}

void launch_dl_sum(hipStream_t s, const double* part, int n, int k, double* out) {
  hipLaunchKernelGGL(dl_sum_kernel, dim3(1), dim3(kDlThreads), 0, s, part, n, k, out);
}

void launch_dl_vec(hipStream_t s, int n_tan, const double* g, const double* dcl, const double* delta_gn, double* v, double* gn_keep, double* part,
                   double* out3) {
  const int grid = (n_tan + kDlThreads - 1) / kDlThreads;
  if (grid == 0) return;
  hipLaunchKernelGGL(dl_vec_kernel, dim3(grid), dim3(kDlThreads), 0, s, n_tan, g, dcl, delta_gn, v, gn_keep, part);
  launch_dl_sum(s, part, grid, 3, out3);
}

void launch_dl_step(hipStream_t s, int n_tan, const double* v, const double* gn, double a, double b, const double* dcl, double* delta, double* part,
                    double* out1) {
  const int grid = (n_tan + kDlThreads - 1) / kDlThreads;
  if (grid == 0) return;
  hipLaunchKernelGGL(dl_step_kernel, dim3(grid), dim3(kDlThreads), 0, s, n_tan, v, gn, a, b, dcl, delta, part);
  launch_dl_sum(s, part, grid, 1, out1);
}

int dl_jv_records(const Visual& vis, const SmallGroup* small, int n_small, const MargDev* marg, int n_marg) {
  int n = 0;
  if (vis.n > 0) n += (vis.n_lm * 8 + kDlThreads - 1) / kDlThreads + (vis.n - vis.n_elim + kDlThreads - 1) / kDlThreads;
  for (int i = 0; i < n_small; ++i) n += (small[i].n * small[i].m + kDlThreads - 1) / kDlThreads;
  for (int i = 0; i < n_marg; ++i) n += marg[i].rows;
  return n;
}

void launch_dl_jv(hipStream_t s, const Visual& vis, int n_pose, const SmallGroup* small, int n_small, const MargDev* marg, int n_marg, const double* u,
                  double* part, double* out2) {
  int off = 0;   // records written so far (2 doubles each), in a fixed order: visual, the groups in the caller's order, the priors
  if (vis.n > 0) {
    const int g_lm = (vis.n_lm * 8 + kDlThreads - 1) / kDlThreads, g_const = (vis.n - vis.n_elim + kDlThreads - 1) / kDlThreads;
    if (g_lm + g_const > 0)
      hipLaunchKernelGGL(dl_jv_vis_kernel, dim3(g_lm + g_const), dim3(kDlThreads), 0, s, vis.n_lm, g_lm, vis.n_elim, vis.n, n_pose, vis.lm_start, vis.J,
                         vis.ja, vis.JB, vis.r, vis.cam_pose, vis.cp_tq, vis.cp_tp, u, part + 2 * (size_t)off);
    off += g_lm + g_const;
  }
  for (int i = 0; i < n_small; ++i) {
    const int grid = (small[i].n * small[i].m + kDlThreads - 1) / kDlThreads;
    if (grid > 0) hipLaunchKernelGGL(dl_jv_small_kernel, dim3(grid), dim3(kDlThreads), 0, s, small[i], u, part + 2 * (size_t)off);
    off += grid;
  }
  for (int i = 0; i < n_marg; ++i) {
    if (marg[i].rows > 0) hipLaunchKernelGGL(dl_jv_marg_kernel, dim3(marg[i].rows), dim3(64), 0, s, marg[i], u, part + 2 * (size_t)off);
    off += marg[i].rows;
  }
  if (off == 0) { launch_zero(s, out2, 2); return; }
  launch_dl_sum(s, part, off, 2, out2);
}

}  // namespace bsg
