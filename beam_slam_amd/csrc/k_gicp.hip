// Generalized ICP for a batch of scan pairs (bsgpu_register_scans_gicp) — the matcher_->Match() of
// RelocCandidateSearchScanContext::AlignSubmapsFromScanMatches (bs_models/src/lib/reloc/reloc_candidate_search_scan_context.cpp:210-262)
// in its shipped GICP configuration.  The arithmetic of one pair is gicp.h, shared with the CPU tests.
// A call has few pairs of large clouds (two aggregates of 21 revolutions: 10^5 points each), so a pair is spread over many workgroups:
//   once per call         launch_point_grid_build  (k_point_grid.hip) the counting-sort grid of every cloud of the call: the targets
//                                                  under T_init, then the sources
//                         gicp_init_kernel         a pair's state: T = I; a cloud of fewer than k points ends it at once
//                         gicp_covariance_kernel   every point of every cloud: its k nearest (list in LDS), C'
//   per outer iteration   gicp_correspond_kernel   grid (chunk, pair): per source point j(i) and M_i stored, the chunk's kept count
//     up to max_inner x   gicp_sums_kernel         grid (chunk, pair): the chunk's partial record of 28 doubles
//                         gicp_step_kernel         one workgroup per pair: the partials in chunk order, the Gauss-Newton step, the criteria
//   once per call         gicp_finish_kernel       the pairs' outputs
// The workgroups of a pair that is done, or whose inner loop has stopped in this outer iteration, return at once.  The host reads the
// pairs' done words once per outer iteration (one small copy) and enqueues nothing for an outer iteration that no pair needs.  No
// workgroup waits for another inside a launch: no fences, no spinning.  No floating-point atomics: the sums have a fixed order
// (point_grid.h), so a pair's bits depend neither on the other pairs of the call nor on the launch geometry.
// The neighbour list of a point is indexed at run time, so it lives in LDS (entry j of thread t at [j * threads + t]: conflict-free),
// one lane per point; the correspondence search gives a point to kGridSub lanes.  Both searches are point_grid.h's own functions.
#include <vector>

#include "gicp.h"
#include "k_point_grid.h"

namespace bsg {

constexpr int kGicpCovThreads = 64;

__global__ __launch_bounds__(64) void gicp_init_kernel(int n_pairs, int k, const int* cloud_start, GicpState* state, int* done) {
  const int p = (int)(blockIdx.x * 64 + threadIdx.x);
  if (p >= n_pairs) return;
  const int n_tgt = cloud_start[p + 1] - cloud_start[p], n_src = cloud_start[n_pairs + p + 1] - cloud_start[n_pairs + p];
  GicpState st;
  gicp_state_init(n_src >= k && n_tgt >= k, &st);
  state[p] = st;
  done[p] = st.status != GICP_NOT_CONVERGED ? 1 : 0;
}

// grid (blocks of kGicpCovThreads points, cloud).  A cloud of fewer than k points has no covariances: zeros.
__global__ __launch_bounds__(kGicpCovThreads) void gicp_covariance_kernel(const int* cloud_start, const PointGrid* grids, const int* cells,
                                                                          const double* rec, const double* tq, int k, double epsilon,
                                                                          double* cov) {
  extern __shared__ double gicp_lists[];       // [2][k][kGicpCovThreads]: d^2, index
  const int c = (int)blockIdx.y, first = cloud_start[c], n = cloud_start[c + 1] - first;
  const int i = (int)(blockIdx.x * kGicpCovThreads + threadIdx.x);
  if (i >= n) return;
  double c6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (n >= k) {
    double* ld = gicp_lists + threadIdx.x;
    double* li = gicp_lists + (size_t)k * kGicpCovThreads + threadIdx.x;
    gicp_knn(grids[c], cells, rec, tq + 3 * (size_t)(first + i), k, ld, li, kGicpCovThreads);
    gicp_covariance(tq + 3 * (size_t)first, li, kGicpCovThreads, k, epsilon, c6);
  }
#pragma unroll
  for (int t = 0; t < 6; ++t) cov[6 * (size_t)(first + i) + t] = c6[t];
}

// kGridSub neighbouring lanes share a source point, as in icp_correspond_kernel: each visits every kGridSub-th record of a shell's
// ranges, their bests are merged after every shell (the lanes of a point take every decision of the search together), and the
// point's first lane forms M and stores.
__global__ __launch_bounds__(kGridChunk * kGridSub) void gicp_correspond_kernel(int n_pairs, const int* cloud_start, const int* chunk_start,
                                                                    const PointGrid* grids, const int* cells, const double* rec, const double* tq,
                                                                    const double* cov, const GicpState* state, const int* done, double mc2,
                                                                    int* corr, double* M, int* kept_part) {
  const int p = (int)blockIdx.y;
  const int c0 = chunk_start[p];
  if (done[p] != 0 || (int)blockIdx.x >= chunk_start[p + 1] - c0) return;
  const int sfirst = cloud_start[n_pairs + p], n = cloud_start[n_pairs + p + 1] - sfirst, qfirst = cloud_start[p];
  const int point = (int)threadIdx.x / kGridSub, sub = (int)threadIdx.x % kGridSub, i = (int)blockIdx.x * kGridChunk + point;
  bool kept = false;
  if (i < n) {
    double T[12], s[3];
    GridBest m;
#pragma unroll
    for (int t = 0; t < 12; ++t) T[t] = state[p].T[t];
    const size_t at = (size_t)(sfirst + i);
    grid_apply(T, tq + 3 * at, s);
    kept = grid_shell_nearest_part(grids[p], cells, rec, s, mc2, sub, kGridSub, GridSubMerge(), &m) && sub == 0;
    if (sub == 0) {
      double m6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      const int j = kept ? (int)m.idx : -1;
      if (kept) gicp_mahalanobis(T, cov + 6 * at, cov + 6 * (size_t)(qfirst + j), m6);
      corr[at] = j;
#pragma unroll
      for (int t = 0; t < 6; ++t) M[6 * at + t] = m6[t];
    }
  }
  const int count = __syncthreads_count(kept ? 1 : 0);
  if (threadIdx.x == 0) kept_part[c0 + (int)blockIdx.x] = count;
}

__global__ __launch_bounds__(kGridChunk) void gicp_sums_kernel(int k, int n_pairs, const int* cloud_start, const int* chunk_start, const double* tq,
                                                              const GicpState* state, const int* corr, const double* M, double* part) {
  const int p = (int)blockIdx.y;
  const int c0 = chunk_start[p];
  if (state[p].status != GICP_NOT_CONVERGED || state[p].stopped_at == k || (int)blockIdx.x >= chunk_start[p + 1] - c0) return;
  const int sfirst = cloud_start[n_pairs + p], n = cloud_start[n_pairs + p + 1] - sfirst, qfirst = cloud_start[p];
  const int i = (int)blockIdx.x * kGridChunk + (int)threadIdx.x;
  double r[kGicpRec];
#pragma unroll
  for (int t = 0; t < kGicpRec; ++t) r[t] = 0.0;
  if (i < n) {
    const size_t at = (size_t)(sfirst + i);
    const int j = corr[at];
    if (j >= 0) {
      double T[12], s[3], m6[6];
#pragma unroll
      for (int t = 0; t < 12; ++t) T[t] = state[p].T[t];
#pragma unroll
      for (int t = 0; t < 6; ++t) m6[t] = M[6 * at + t];
      grid_apply(T, tq + 3 * at, s);
      gicp_terms(true, s, tq + 3 * (size_t)(qfirst + j), m6, r);
    }
  }
  grid_chunk_reduce<kGicpRec>(r, part + (size_t)(c0 + (int)blockIdx.x) * kGicpRec);
}

__global__ __launch_bounds__(64) void gicp_step_kernel(int k, int it, const int* chunk_start, const double* part, const int* kept_part, GicpParams P,
                                                       GicpState* state, int* done) {
  __shared__ double sum[kGicpRec];
  __shared__ int kept;
  const int p = (int)blockIdx.x;
  if (state[p].status != GICP_NOT_CONVERGED || state[p].stopped_at == k) return;
  const int c0 = chunk_start[p], c1 = chunk_start[p + 1];
  if (threadIdx.x < kGicpRec) {
    sum[threadIdx.x] = grid_sum_partials<kGicpRec>(part, c0, c1);
  } else if (threadIdx.x == kGicpRec) {
    int n = 0;
    for (int c = c0; c < c1; ++c) n += kept_part[c];
    kept = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s[kGicpRec];
#pragma unroll
    for (int t = 0; t < kGicpRec; ++t) s[t] = sum[t];
    GicpState st = state[p];
    gicp_advance(s, kept, k, it, P, &st);
    state[p] = st;
    if (st.status != GICP_NOT_CONVERGED) done[p] = 1;
  }
}

__global__ __launch_bounds__(64) void gicp_finish_kernel(int n_pairs, const GicpState* state, const double* T_cloud, double* T, double* T_ref_tgt,
                                                         double* cost, int* n_corr, int* n_iters, int* n_inner, int* status) {
  const int p = (int)(blockIdx.x * 64 + threadIdx.x);
  if (p >= n_pairs) return;
  const GicpState st = state[p];
  double Ti[12], out[12];
#pragma unroll
  for (int t = 0; t < 12; ++t) Ti[t] = T_cloud[12 * p + t];
  icp_inverse_times(st.T, Ti, out);
#pragma unroll
  for (int t = 0; t < 12; ++t) { T[12 * p + t] = st.T[t]; T_ref_tgt[12 * p + t] = out[t]; }
  cost[p] = st.cost; n_corr[p] = st.n_corr; n_iters[p] = st.n_iters; n_inner[p] = st.n_inner; status[p] = st.status;
}

hipError_t launch_register_scans_gicp(hipStream_t s, int n_pairs, int n_live, int max_points, int n_points, int max_chunks, int n_tiles,
                                      const int* cloud_start, const double* pts, const double* T_cloud, const int* chunk_start,
                                      const PointGrid* grids, const GicpParams& P, double* T, double* T_ref_tgt, double* cost, int* n_corr,
                                      int* n_iters, int* n_inner, int* status, double* cov, double* tq, int* tcell, int* cells, int* tile_sum,
                                      double* rec, GicpState* state, int* done, int* corr, double* M, int* kept, double* part) {
  if (n_pairs <= 0) return hipSuccess;
  const int pair_blocks = (n_pairs + 63) / 64;
  launch_point_grid_build(s, 2 * n_pairs, max_points, n_points, n_tiles, cloud_start, pts, T_cloud, grids, tq, tcell, cells, tile_sum, rec);
  hipLaunchKernelGGL(gicp_init_kernel, dim3(pair_blocks), dim3(64), 0, s, n_pairs, P.k, cloud_start, state, done);
  if (max_points > 0)
    hipLaunchKernelGGL(gicp_covariance_kernel, dim3((max_points + kGicpCovThreads - 1) / kGicpCovThreads, 2 * n_pairs), dim3(kGicpCovThreads),
                       2 * sizeof(double) * (size_t)P.k * kGicpCovThreads, s, cloud_start, grids, cells, rec, tq, P.k, P.epsilon, cov);
  hipError_t e = hipSuccess;
  const double mc2 = P.max_corr * P.max_corr;
  std::vector<int> done_h((size_t)n_pairs, 0);
  for (int k = 1; k <= P.max_iter && n_live > 0 && max_chunks > 0 && e == hipSuccess; ++k) {
    hipLaunchKernelGGL(gicp_correspond_kernel, dim3(max_chunks, n_pairs), dim3(kGridChunk * kGridSub), 0, s, n_pairs, cloud_start, chunk_start, grids, cells, rec,
                       tq, cov, state, done, mc2, corr, M, kept);
    for (int it = 1; it <= P.max_inner; ++it) {
      hipLaunchKernelGGL(gicp_sums_kernel, dim3(max_chunks, n_pairs), dim3(kGridChunk), 0, s, k, n_pairs, cloud_start, chunk_start, tq, state, corr, M,
                         part);
      hipLaunchKernelGGL(gicp_step_kernel, dim3(n_pairs), dim3(64), 0, s, k, it, chunk_start, part, kept, P, state, done);
    }
    // the one copy per outer iteration: which pairs are done
    e = hipMemcpyAsync(done_h.data(), done, sizeof(int) * (size_t)n_pairs, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    n_live = 0;
    for (int d : done_h) n_live += d == 0 ? 1 : 0;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gicp_finish_kernel, dim3(pair_blocks), dim3(64), 0, s, n_pairs, state, T_cloud, T, T_ref_tgt, cost, n_corr, n_iters, n_inner,
                     status);
  return hipGetLastError();
}

}  // namespace bsg
