// The dense grids of a batch of point clouds (point_grid.h), built once per call for the scan registrations (k_icp.hip: every pair's
// target; k_gicp.hip: every pair's target and source):
//   grid_prepare_kernel   every point under its cloud's transform, its grid cell, the cells' counts
//   grid_scan_*           the exclusive scan of the counts of every cloud's cells at once (tile sums, their scan, the tiles)
//   grid_scatter_kernel   the counting sort: (x, y, z, index) records in cell order, starts -> ends
// The integer atomics of the counting sort decide only the order inside a cell, which the (d^2, index) comparison of the searches
// makes irrelevant.
#include "bsgpu_device.h"
#include "point_grid.h"

namespace bsg {

constexpr int kGridPrepThreads = 256;
constexpr int kGridScanThreads = 256;                 // x 4 cells per thread = kGridScanTile (bsgpu_internal.h)
static_assert(kGridScanTile == 4 * kGridScanThreads, "a scan tile is one int4 per thread");

__global__ __launch_bounds__(kGridPrepThreads) void grid_prepare_kernel(const int* cloud_start, const double* pts, const double* T_cloud,
                                                                      const PointGrid* grids, double* tq, int* tcell, int* cells) {
  const int p = (int)blockIdx.y, first = cloud_start[p], n = cloud_start[p + 1] - first;
  const PointGrid g = grids[p];
  for (int i = (int)(blockIdx.x * kGridPrepThreads + threadIdx.x); i < n; i += (int)gridDim.x * kGridPrepThreads) {
    const size_t t = (size_t)(first + i);
    double q[3];
    grid_apply(T_cloud + 12 * p, pts + 3 * t, q);
    tq[3 * t] = q[0]; tq[3 * t + 1] = q[1]; tq[3 * t + 2] = q[2];
    const int c = grid_cell_of(g, q);          // clamped into the cloud's cells
    tcell[t] = c;
    atomicAdd(&cells[c], 1);
  }
}

// inclusive scan of one value per thread over a workgroup of kGridScanThreads; returns the workgroup's total through *total
__device__ __forceinline__ int grid_block_scan(int v, int* wave_tot, int* total) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off, 64);
    v += lane >= off ? o : 0;
  }
  if (lane == 63) wave_tot[wave] = v;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kGridScanThreads / 64; ++w) { before += w < wave ? wave_tot[w] : 0; all += wave_tot[w]; }
  __syncthreads();
  *total = all;
  return v + before;
}

// the cells come in tiles of kGridScanTile (the array is padded to whole tiles with empty cells)
__global__ __launch_bounds__(kGridScanThreads) void grid_scan_sums_kernel(const int4* cells, int* tile_sum) {
  __shared__ int wave_tot[kGridScanThreads / 64];
  const int4 c = cells[(size_t)blockIdx.x * kGridScanThreads + threadIdx.x];
  int total;
  grid_block_scan(c.x + c.y + c.z + c.w, wave_tot, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
// one workgroup: tile_sum -> its exclusive scan, in place
__global__ __launch_bounds__(kGridScanThreads) void grid_scan_tiles_kernel(int* tile_sum, int n_tiles) {
  __shared__ int wave_tot[kGridScanThreads / 64];
  int carry = 0;
  for (int base = 0; base < n_tiles; base += kGridScanThreads) {
    const int i = base + (int)threadIdx.x;
    const int v = i < n_tiles ? tile_sum[i] : 0;
    int total;
    const int incl = grid_block_scan(v, wave_tot, &total);
    if (i < n_tiles) tile_sum[i] = carry + incl - v;
    carry += total;
  }
}
// counts -> starts, in place
__global__ __launch_bounds__(kGridScanThreads) void grid_scan_cells_kernel(int4* cells, const int* tile_off) {
  __shared__ int wave_tot[kGridScanThreads / 64];
  const size_t at = (size_t)blockIdx.x * kGridScanThreads + threadIdx.x;
  const int4 c = cells[at];
  const int mine = c.x + c.y + c.z + c.w;
  int total;
  const int start = tile_off[blockIdx.x] + grid_block_scan(mine, wave_tot, &total) - mine;
  cells[at] = make_int4(start, start + c.x, start + c.x + c.y, start + c.x + c.y + c.z);
}

// the counting sort's second pass: every cell's start becomes its end
__global__ __launch_bounds__(kGridPrepThreads) void grid_scatter_kernel(const int* cloud_start, const double* tq, const int* tcell, int* cells,
                                                                      double* rec, int n_points) {
  const int p = (int)blockIdx.y, first = cloud_start[p], n = cloud_start[p + 1] - first;
  for (int i = (int)(blockIdx.x * kGridPrepThreads + threadIdx.x); i < n; i += (int)gridDim.x * kGridPrepThreads) {
    const size_t t = (size_t)(first + i);
    const int pos = atomicAdd(&cells[tcell[t]], 1);
    if ((unsigned)pos < (unsigned)n_points) {    // (always: the starts are the scan of the counts of these same cells)
      double4 r;
      r.x = tq[3 * t]; r.y = tq[3 * t + 1]; r.z = tq[3 * t + 2]; r.w = (double)i;
      reinterpret_cast<double4*>(rec)[pos] = r;
    }
  }
}

void launch_point_grid_build(hipStream_t s, int n_clouds, int max_points, int n_points, int n_tiles, const int* cloud_start, const double* pts,
                             const double* T_cloud, const PointGrid* grids, double* tq, int* tcell, int* cells, int* tile_sum, double* rec) {
  if (n_clouds <= 0) return;
  const int prep_x = std::max(1, std::min((max_points + kGridPrepThreads - 1) / kGridPrepThreads, 1024));
  if (n_tiles > 0) (void)hipMemsetAsync(cells, 0, sizeof(int) * (size_t)n_tiles * kGridScanTile, s);
  hipLaunchKernelGGL(grid_prepare_kernel, dim3(prep_x, n_clouds), dim3(kGridPrepThreads), 0, s, cloud_start, pts, T_cloud, grids, tq, tcell, cells);
  if (n_tiles > 0) {
    hipLaunchKernelGGL(grid_scan_sums_kernel, dim3(n_tiles), dim3(kGridScanThreads), 0, s, reinterpret_cast<const int4*>(cells), tile_sum);
    hipLaunchKernelGGL(grid_scan_tiles_kernel, dim3(1), dim3(kGridScanThreads), 0, s, tile_sum, n_tiles);
    hipLaunchKernelGGL(grid_scan_cells_kernel, dim3(n_tiles), dim3(kGridScanThreads), 0, s, reinterpret_cast<int4*>(cells), tile_sum);
    hipLaunchKernelGGL(grid_scatter_kernel, dim3(prep_x, n_clouds), dim3(kGridPrepThreads), 0, s, cloud_start, tq, tcell, cells, rec, n_points);
  }
}

}  // namespace bsg
