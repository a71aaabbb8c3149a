// The device half of point_grid.h for the kernels that search a grid or sum over a cloud (k_icp.hip, k_gicp.hip): the merge of the
// lanes that share a query, and the two halves of a sum in point_grid.h's fixed order — a chunk's partial record, then the partial
// records of a pair in chunk order.  grid_chunked_sums (point_grid.h) is the same sum on the host.
#pragma once
#include "bsgpu_device.h"
#include "point_grid.h"

namespace bsg {

// The bests of the kGridSub neighbouring lanes that share a query, merged by (d^2, index) through three shuffles: every lane of the
// group ends with the group's best.  (The Merge of grid_shell_nearest_part.)
struct GridSubMerge {
  __device__ __forceinline__ void operator()(GridBest* m) const {
#pragma unroll
    for (int s = 1; s < kGridSub; s <<= 1) {
      const double ob = __shfl_xor(m->d2, s, kGridWave), oi = __shfl_xor(m->idx, s, kGridWave);
      const double ox = __shfl_xor(m->x, s, kGridWave), oy = __shfl_xor(m->y, s, kGridWave), oz = __shfl_xor(m->z, s, kGridWave);
      const bool better = grid_better(ob, oi, m->d2, m->idx);
      m->d2 = better ? ob : m->d2; m->idx = better ? oi : m->idx;
      m->x = better ? ox : m->x; m->y = better ? oy : m->y; m->z = better ? oz : m->z;
    }
  }
};

// A chunk's partial record from the REC terms of each of its kGridChunk points: thread t < kGridChunk passes point t's terms; every
// thread of the workgroup calls.  Lane 0 of each of the first kGridChunk / 64 waves gets the tree of grid_wave_tree over its 64
// points, the waves are then added in order, and thread t < REC stores sum t to out[t].
template <int REC>
__device__ __forceinline__ void grid_chunk_reduce(const double* term, double* out) {
  __shared__ double wave_sum[kGridChunk / kGridWave][REC];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (threadIdx.x < kGridChunk) {
#pragma unroll
    for (int t = 0; t < REC; ++t) {
      double v = term[t];
#pragma unroll
      for (int off = kGridWave / 2; off >= 1; off >>= 1) v = v + __shfl_down(v, off, kGridWave);
      if (lane == 0) wave_sum[wave][t] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < REC) {
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < kGridChunk / kGridWave; ++w) sum = sum + wave_sum[w][threadIdx.x];
    out[threadIdx.x] = sum;
  }
}

// Sum t = threadIdx.x < REC of the partial records c0 .. c1 - 1, added in chunk order with eight loads in flight
template <int REC>
__device__ __forceinline__ double grid_sum_partials(const double* part, int c0, int c1) {
  double s = 0.0;
  int c = c0;
  for (; c + 8 <= c1; c += 8) {
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(c + j) * REC + threadIdx.x];
#pragma unroll
    for (int j = 0; j < 8; ++j) s = s + v[j];
  }
  for (; c < c1; ++c) s = s + part[(size_t)c * REC + threadIdx.x];
  return s;
}

}  // namespace bsg
