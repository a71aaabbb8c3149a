// Point-to-point ICP scan registration for a batch of scan pairs (bsgpu_register_scans) — the reference's matcher_->Match() of
// MultiScanRegistration::MatchScans (bs_models/src/lib/scan_registration/multi_scan_registration.cpp:451-487) in its shipped ICP
// configuration.  The arithmetic of one pair is icp.h, shared with the CPU tests.
// A call has few pairs (1-10) of large clouds (a VLP-16 revolution: 29 000 points), so a pair is spread over many workgroups:
//   once per call    launch_point_grid_build  (k_point_grid.hip) the counting-sort grid of every pair's target under its T_init
//                    icp_init_kernel          a pair's state: T = I, no previous mse, not done
//   per iteration    icp_correspond_kernel    grid (chunk, pair): kGridChunk source points, kGridSub lanes each -> one partial record of 17 doubles
//                    icp_update_kernel        one workgroup per pair: the partials in chunk order, the step, the criteria, the done word
// All max_iter iterations are enqueued back to back; the workgroups of a pair that is done return at once.  No workgroup waits for
// another inside a launch: no fences, no spinning.  No floating-point atomics: the sums have a fixed order (point_grid.h), so a pair's
// bits depend neither on the other pairs of the call nor on the launch geometry.
#include "icp.h"
#include "k_point_grid.h"

namespace bsg {

__global__ __launch_bounds__(64) void icp_init_kernel(int n_pairs, double* T, double* mse_prev, int* done) {
  const int p = (int)(blockIdx.x * 64 + threadIdx.x);
  if (p >= n_pairs) return;
#pragma unroll
  for (int t = 0; t < 12; ++t) T[12 * p + t] = t % 5 == 0 ? 1.0 : 0.0;
  mse_prev[p] = std::numeric_limits<double>::infinity();
  done[p] = 0;
}

// kGridSub neighbouring lanes share a source point: each visits every kGridSub-th candidate of the point's 9 ranges (neighbouring
// lanes read neighbouring 32-byte records), their bests are merged, and the point's terms go to LDS, from where the first kGridChunk
// threads add them.  (With one lane per point the launch had less than one wave per SIMD and nothing to hide its loads behind.)
__global__ __launch_bounds__(kGridChunk * kGridSub) void icp_correspond_kernel(const int* ref_start, const double* ref, const int* chunk_start,
                                                                               const PointGrid* grids, const int* cells, const double* rec,
                                                                               const double* T, const int* done, double h2, double* part) {
  __shared__ double terms[kGridChunk][kIcpRec];
  const int p = (int)blockIdx.y;
  const int c0 = chunk_start[p];
  if (done[p] != 0 || (int)blockIdx.x >= chunk_start[p + 1] - c0) return;
  const int first = ref_start[p], n = ref_start[p + 1] - first;
  const int point = (int)threadIdx.x / kGridSub, sub = (int)threadIdx.x % kGridSub, i = (int)blockIdx.x * kGridChunk + point;
  double s[3] = {0.0, 0.0, 0.0};
  GridBest m = grid_no_best();
  if (i < n) {
    grid_apply(T + 12 * p, ref + 3 * (size_t)(first + i), s);
    m = grid_near_part(grids[p], cells, rec, s, sub, kGridSub);
  }
  GridSubMerge()(&m);
  if (sub == 0) {
    const double q[3] = {m.x, m.y, m.z};
    double r[kIcpRec];
    icp_record(m.d2 <= h2, s, q, m.d2, r);
#pragma unroll
    for (int t = 0; t < kIcpRec; ++t) terms[point][t] = r[t];
  }
  __syncthreads();
  grid_chunk_reduce<kIcpRec>(terms[threadIdx.x % kGridChunk], part + (size_t)(c0 + (int)blockIdx.x) * kIcpRec);
}

__global__ __launch_bounds__(64) void icp_update_kernel(int k, const int* chunk_start, const double* part, IcpParams P, const double* T_init,
                                                        double* T, double* T_ref_tgt, double* mse_prev, double* mse, int* n_corr, int* n_iters,
                                                        int* status, int* done) {
  __shared__ double sum[kIcpRec];
  const int p = (int)blockIdx.x;
  if (done[p] != 0) return;
  if (threadIdx.x < kIcpRec) sum[threadIdx.x] = grid_sum_partials<kIcpRec>(part, chunk_start[p], chunk_start[p + 1]);
  __syncthreads();
  if (threadIdx.x == 0) {
    double s[kIcpRec], Tp[12], prev = mse_prev[p], m;
#pragma unroll
    for (int t = 0; t < kIcpRec; ++t) s[t] = sum[t];
#pragma unroll
    for (int t = 0; t < 12; ++t) Tp[t] = T[12 * p + t];
    int nc;
    const int st = icp_step(s, k, P, Tp, &prev, &m, &nc);
#pragma unroll
    for (int t = 0; t < 12; ++t) T[12 * p + t] = Tp[t];
    mse_prev[p] = prev;
    if (st != ICP_NOT_CONVERGED) {
      double Ti[12], out[12];
#pragma unroll
      for (int t = 0; t < 12; ++t) Ti[t] = T_init[12 * p + t];
      icp_inverse_times(Tp, Ti, out);
#pragma unroll
      for (int t = 0; t < 12; ++t) T_ref_tgt[12 * p + t] = out[t];
      mse[p] = m; n_corr[p] = nc; n_iters[p] = icp_iterations(st, k); status[p] = st;
      done[p] = 1;
    }
  }
}

void launch_register_scans(hipStream_t s, int n_pairs, int max_targets, int n_targets, int max_chunks, int n_tiles, const int* ref_start,
                           const double* ref, const int* tgt_start, const double* tgt, const double* T_init, const int* chunk_start,
                           const PointGrid* grids, double max_corr, const IcpParams& P, double* T, double* T_ref_tgt, double* mse, int* n_corr,
                           int* n_iters, int* status, double* tq, int* tcell, int* cells, int* tile_sum, double* rec, double* part,
                           double* mse_prev, int* done) {
  if (n_pairs <= 0) return;
  launch_point_grid_build(s, n_pairs, max_targets, n_targets, n_tiles, tgt_start, tgt, T_init, grids, tq, tcell, cells, tile_sum, rec);
  hipLaunchKernelGGL(icp_init_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, s, n_pairs, T, mse_prev, done);
  const double h2 = max_corr * max_corr;
  for (int k = 1; k <= P.max_iter; ++k) {
    if (max_chunks > 0)
      hipLaunchKernelGGL(icp_correspond_kernel, dim3(max_chunks, n_pairs), dim3(kGridChunk * kGridSub), 0, s, ref_start, ref, chunk_start, grids, cells, rec,
                         T, done, h2, part);
    hipLaunchKernelGGL(icp_update_kernel, dim3(n_pairs), dim3(64), 0, s, k, chunk_start, part, P, T_init, T, T_ref_tgt, mse_prev, mse, n_corr,
                       n_iters, status, done);
  }
}

}  // namespace bsg
