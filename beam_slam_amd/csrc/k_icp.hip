// Point-to-point ICP scan registration for a batch of scan pairs (bsgpu_register_scans) — the reference's matcher_->Match() of
// MultiScanRegistration::MatchScans (bs_models/src/lib/scan_registration/multi_scan_registration.cpp:451-487) in its shipped ICP
// configuration.  The arithmetic of one pair is icp.h, shared with the CPU tests.
// A call has few pairs (1-10) of large clouds (a VLP-16 revolution: 29 000 points), so a pair is spread over many workgroups:
//   once per call    icp_prepare_kernel   T_init onto the target, each point's grid cell, the cells' counts
//                    icp_scan_*           the exclusive scan of the counts of every pair's cells at once (tile sums, their scan, the tiles)
//                    icp_scatter_kernel   the counting sort: (x, y, z, index) records in cell order, starts -> ends
//   per iteration    icp_correspond_kernel  grid (chunk, pair): kIcpChunk source points, kIcpSub lanes each -> one partial record of 17 doubles
//                    icp_update_kernel      one workgroup per pair: the partials in chunk order, the step, the criteria, the done word
// All max_iter iterations are enqueued back to back; the workgroups of a pair that is done return at once.  No workgroup waits for
// another inside a launch: no fences, no spinning.  No floating-point atomics: the sums have a fixed order (icp.h), so a pair's bits
// depend neither on the other pairs of the call nor on the launch geometry.  The integer atomics of the counting sort decide only the
// order inside a cell, which the (d^2, index) comparison makes irrelevant.
#include "bsgpu_device.h"
#include "icp.h"

namespace bsg {

constexpr int kIcpPrepThreads = 256;
constexpr int kIcpScanThreads = 256;                 // x 4 cells per thread = kIcpScanTile (bsgpu_internal.h)
static_assert(kIcpScanTile == 4 * kIcpScanThreads, "a scan tile is one int4 per thread");

__global__ __launch_bounds__(kIcpPrepThreads) void icp_prepare_kernel(const int* tgt_start, const double* tgt, const double* T_init,
                                                                      const IcpGrid* grids, double* tq, int* tcell, int* cells, double* T,
                                                                      double* mse_prev, int* done) {
  const int p = (int)blockIdx.y, first = tgt_start[p], n = tgt_start[p + 1] - first;
  if (blockIdx.x == 0) {
    if (threadIdx.x < 12) T[12 * p + threadIdx.x] = threadIdx.x % 5 == 0 ? 1.0 : 0.0;
    if (threadIdx.x == 0) { mse_prev[p] = std::numeric_limits<double>::infinity(); done[p] = 0; }
  }
  const IcpGrid g = grids[p];
  for (int i = (int)(blockIdx.x * kIcpPrepThreads + threadIdx.x); i < n; i += (int)gridDim.x * kIcpPrepThreads) {
    const size_t t = (size_t)(first + i);
    double q[3];
    icp_apply(T_init + 12 * p, tgt + 3 * t, q);
    tq[3 * t] = q[0]; tq[3 * t + 1] = q[1]; tq[3 * t + 2] = q[2];
    const int c = icp_cell_of(g, q);          // clamped into the pair's cells
    tcell[t] = c;
    atomicAdd(&cells[c], 1);
  }
}

// inclusive scan of one value per thread over a workgroup of kIcpScanThreads; returns the workgroup's total through *total
__device__ __forceinline__ int icp_block_scan(int v, int* wave_tot, int* total) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off, 64);
    v += lane >= off ? o : 0;
  }
  if (lane == 63) wave_tot[wave] = v;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kIcpScanThreads / 64; ++w) { before += w < wave ? wave_tot[w] : 0; all += wave_tot[w]; }
  __syncthreads();
  *total = all;
  return v + before;
}

// the cells come in tiles of kIcpScanTile (the array is padded to whole tiles with empty cells)
__global__ __launch_bounds__(kIcpScanThreads) void icp_scan_sums_kernel(const int4* cells, int* tile_sum) {
  __shared__ int wave_tot[kIcpScanThreads / 64];
  const int4 c = cells[(size_t)blockIdx.x * kIcpScanThreads + threadIdx.x];
  int total;
  icp_block_scan(c.x + c.y + c.z + c.w, wave_tot, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
// one workgroup: tile_sum -> its exclusive scan, in place
__global__ __launch_bounds__(kIcpScanThreads) void icp_scan_tiles_kernel(int* tile_sum, int n_tiles) {
  __shared__ int wave_tot[kIcpScanThreads / 64];
  int carry = 0;
  for (int base = 0; base < n_tiles; base += kIcpScanThreads) {
    const int i = base + (int)threadIdx.x;
    const int v = i < n_tiles ? tile_sum[i] : 0;
    int total;
    const int incl = icp_block_scan(v, wave_tot, &total);
    if (i < n_tiles) tile_sum[i] = carry + incl - v;
    carry += total;
  }
}
// counts -> starts, in place
__global__ __launch_bounds__(kIcpScanThreads) void icp_scan_cells_kernel(int4* cells, const int* tile_off) {
  __shared__ int wave_tot[kIcpScanThreads / 64];
  const size_t at = (size_t)blockIdx.x * kIcpScanThreads + threadIdx.x;
  const int4 c = cells[at];
  const int mine = c.x + c.y + c.z + c.w;
  int total;
  const int start = tile_off[blockIdx.x] + icp_block_scan(mine, wave_tot, &total) - mine;
  cells[at] = make_int4(start, start + c.x, start + c.x + c.y, start + c.x + c.y + c.z);
}

// the counting sort's second pass: every cell's start becomes its end
__global__ __launch_bounds__(kIcpPrepThreads) void icp_scatter_kernel(const int* tgt_start, const double* tq, const int* tcell, int* cells,
                                                                      double* rec, int n_targets) {
  const int p = (int)blockIdx.y, first = tgt_start[p], n = tgt_start[p + 1] - first;
  for (int i = (int)(blockIdx.x * kIcpPrepThreads + threadIdx.x); i < n; i += (int)gridDim.x * kIcpPrepThreads) {
    const size_t t = (size_t)(first + i);
    const int pos = atomicAdd(&cells[tcell[t]], 1);
    if ((unsigned)pos < (unsigned)n_targets) {    // (always: the starts are the scan of the counts of these same cells)
      double4 r;
      r.x = tq[3 * t]; r.y = tq[3 * t + 1]; r.z = tq[3 * t + 2]; r.w = (double)i;
      reinterpret_cast<double4*>(rec)[pos] = r;
    }
  }
}

// kIcpSub neighbouring lanes share a source point: each visits every kIcpSub-th candidate of the point's 9 ranges (neighbouring
// lanes read neighbouring 32-byte records), their bests are merged by (d^2, index) through three shuffles, and the point's terms go to
// LDS; the first kIcpChunk threads then add them in the tree of icp_wave_tree.  (With one lane per point the launch had less than one
// wave per SIMD and nothing to hide its loads behind.)
__global__ __launch_bounds__(kIcpChunk * kIcpSub) void icp_correspond_kernel(const int* ref_start, const double* ref, const int* chunk_start,
                                                                             const IcpGrid* grids, const int* cells, const double* rec,
                                                                             const double* T, const int* done, double h2, double* part) {
  __shared__ double terms[kIcpChunk][kIcpRec];
  __shared__ double wave_sum[kIcpChunk / kIcpWave][kIcpRec];
  const int p = (int)blockIdx.y;
  const int c0 = chunk_start[p];
  if (done[p] != 0 || (int)blockIdx.x >= chunk_start[p + 1] - c0) return;
  const int first = ref_start[p], n = ref_start[p + 1] - first;
  const int point = (int)threadIdx.x / kIcpSub, sub = (int)threadIdx.x % kIcpSub, i = (int)blockIdx.x * kIcpChunk + point;
  double s[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0}, best = std::numeric_limits<double>::infinity(), bidx = best;
  if (i < n) {
    icp_apply(T + 12 * p, ref + 3 * (size_t)(first + i), s);
    icp_nearest_part(grids[p], cells, rec, s, sub, kIcpSub, &best, &bidx, q);
  }
#pragma unroll
  for (int m = 1; m < kIcpSub; m <<= 1) {
    const double ob = __shfl_xor(best, m, kIcpWave), oi = __shfl_xor(bidx, m, kIcpWave);
    const double ox = __shfl_xor(q[0], m, kIcpWave), oy = __shfl_xor(q[1], m, kIcpWave), oz = __shfl_xor(q[2], m, kIcpWave);
    const bool better = icp_better(ob, oi, best, bidx);
    best = better ? ob : best; bidx = better ? oi : bidx;
    q[0] = better ? ox : q[0]; q[1] = better ? oy : q[1]; q[2] = better ? oz : q[2];
  }
  if (sub == 0) {
    double r[kIcpRec];
    icp_record(best <= h2, s, q, best, r);
#pragma unroll
    for (int t = 0; t < kIcpRec; ++t) terms[point][t] = r[t];
  }
  __syncthreads();
  // lane 0 of each of the first kIcpChunk / 64 waves: the tree of icp_wave_tree over its 64 points
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (threadIdx.x < kIcpChunk) {
#pragma unroll
    for (int t = 0; t < kIcpRec; ++t) {
      double v = terms[threadIdx.x][t];
#pragma unroll
      for (int off = kIcpWave / 2; off >= 1; off >>= 1) v = v + __shfl_down(v, off, kIcpWave);
      if (lane == 0) wave_sum[wave][t] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < kIcpRec) {
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < kIcpChunk / kIcpWave; ++w) sum = sum + wave_sum[w][threadIdx.x];
    part[(size_t)(c0 + (int)blockIdx.x) * kIcpRec + threadIdx.x] = sum;
  }
}

__global__ __launch_bounds__(64) void icp_update_kernel(int k, const int* chunk_start, const double* part, IcpParams P, const double* T_init,
                                                        double* T, double* T_ref_tgt, double* mse_prev, double* mse, int* n_corr, int* n_iters,
                                                        int* status, int* done) {
  __shared__ double sum[kIcpRec];
  const int p = (int)blockIdx.x;
  if (done[p] != 0) return;
  if (threadIdx.x < kIcpRec) {
    const int c0 = chunk_start[p], c1 = chunk_start[p + 1];
    double s = 0.0;
    int c = c0;
    for (; c + 8 <= c1; c += 8) {       // eight loads in flight, added in chunk order
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(c + j) * kIcpRec + threadIdx.x];
#pragma unroll
      for (int j = 0; j < 8; ++j) s = s + v[j];
    }
    for (; c < c1; ++c) s = s + part[(size_t)c * kIcpRec + threadIdx.x];
    sum[threadIdx.x] = s;
  }
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

// The grids of n_pairs clouds (the once-per-call launches above), also for bsgpu_register_scans_gicp (k_gicp.hip), whose clouds are
// the targets and the sources of its pairs.
void launch_icp_grid_build(hipStream_t s, int n_pairs, int max_targets, int n_targets, int n_tiles, const int* tgt_start, const double* tgt,
                           const double* T_init, const IcpGrid* grids, double* tq, int* tcell, int* cells, int* tile_sum, double* rec, double* T,
                           double* mse_prev, int* done) {
  if (n_pairs <= 0) return;
  const int prep_x = std::max(1, std::min((max_targets + kIcpPrepThreads - 1) / kIcpPrepThreads, 1024));
  (void)hipMemsetAsync(cells, 0, sizeof(int) * (size_t)n_tiles * kIcpScanTile, s);
  hipLaunchKernelGGL(icp_prepare_kernel, dim3(prep_x, n_pairs), dim3(kIcpPrepThreads), 0, s, tgt_start, tgt, T_init, grids, tq, tcell, cells, T,
                     mse_prev, done);
  if (n_tiles > 0) {
    hipLaunchKernelGGL(icp_scan_sums_kernel, dim3(n_tiles), dim3(kIcpScanThreads), 0, s, reinterpret_cast<const int4*>(cells), tile_sum);
    hipLaunchKernelGGL(icp_scan_tiles_kernel, dim3(1), dim3(kIcpScanThreads), 0, s, tile_sum, n_tiles);
    hipLaunchKernelGGL(icp_scan_cells_kernel, dim3(n_tiles), dim3(kIcpScanThreads), 0, s, reinterpret_cast<int4*>(cells), tile_sum);
    hipLaunchKernelGGL(icp_scatter_kernel, dim3(prep_x, n_pairs), dim3(kIcpPrepThreads), 0, s, tgt_start, tq, tcell, cells, rec, n_targets);
  }
}

void launch_register_scans(hipStream_t s, int n_pairs, int max_targets, int n_targets, int max_chunks, int n_tiles, const int* ref_start,
                           const double* ref, const int* tgt_start, const double* tgt, const double* T_init, const int* chunk_start,
                           const IcpGrid* grids, double max_corr, const IcpParams& P, double* T, double* T_ref_tgt, double* mse, int* n_corr,
                           int* n_iters, int* status, double* tq, int* tcell, int* cells, int* tile_sum, double* rec, double* part,
                           double* mse_prev, int* done) {
  if (n_pairs <= 0) return;
  launch_icp_grid_build(s, n_pairs, max_targets, n_targets, n_tiles, tgt_start, tgt, T_init, grids, tq, tcell, cells, tile_sum, rec, T, mse_prev, done);
  const double h2 = max_corr * max_corr;
  for (int k = 1; k <= P.max_iter; ++k) {
    if (max_chunks > 0)
      hipLaunchKernelGGL(icp_correspond_kernel, dim3(max_chunks, n_pairs), dim3(kIcpChunk * kIcpSub), 0, s, ref_start, ref, chunk_start, grids, cells, rec,
                         T, done, h2, part);
    hipLaunchKernelGGL(icp_update_kernel, dim3(n_pairs), dim3(64), 0, s, k, chunk_start, part, P, T_init, T, T_ref_tgt, mse_prev, mse, n_corr,
                       n_iters, status, done);
  }
}

}  // namespace bsg
