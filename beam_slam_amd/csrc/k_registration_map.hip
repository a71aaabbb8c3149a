// The reference clouds of scan-to-map registration for a batch of maps (bsgpu_build_registration_maps) — the merge and voxel filter of
// RegistrationMap::GetLoamCloudMap / GetPointCloudMap (bs_models/src/lib/scan_registration/registration_map.cpp:96-135).  The rules of
// one point and one voxel are registration_map.h, shared with the CPU tests.  A map's points are one contiguous range of the call's
// (its scans follow each other), cut into tiles of kMapSortTile positions; one workgroup of kMapThreads lanes per tile, the tiles of all
// maps in one launch (tile_map: a tile's map; tile_start: a map's first tile).
//   map_key_kernel        a lane per point of the call: its scan (a binary search of scan_start), the transformed point, the 63-bit key
//                         (the sentinel for a dropped point) and the index; sets the range flag.  Merge only: writes the outputs itself.
//   a stable LSD radix sort of (key, index) inside every map, 8 bits per pass, 8 passes:
//   map_hist_kernel       a tile's count of every digit (LDS integer counts), stored digit-major, tile-minor per map
//   map_scan_kernel       one workgroup of 1 024 lanes per map: the exclusive scan of its counts, in place
//   map_scatter_kernel    a tile's keys in rounds of a workgroup, in order: the rank among equal digits inside a wave from eight
//                         ballots (the peer mask) and a popcount of the lower lanes; the waves' counts through LDS in wave order; the
//                         digit's running base carried from round to round.  Every destination is computed, none is taken by an atomic.
//   map_heads_kernel      a tile's number of heads (a key that is no sentinel and differs from its predecessor's in the map)
//   map_scan_kernel       again, per map over its tiles' heads: a tile's first output slot, and the map's number of voxels
//   map_centroid_kernel   a head's slot from the workgroup scan; its lane walks the run in sorted order — input order, the sort being
//                         stable — and writes the centroid and the count
// No floating-point atomics; the only integer atomics count digits in LDS, and a count does not depend on the order of its increments;
// every output word has one writer (the range flag is only ever set to 1).  A map's bytes depend neither on its neighbours in the call
// nor on the tile size or the launch: the sort is stable and a voxel's sum is sequential.
// The outputs have fixed capacity — map m's voxels from its first input point's position — and the host packs them after the copy-out.
// This translation unit is compiled with floating-point contraction off (Makefile): the device must return the bits of the header on
// the host.
#include "bsgpu_internal.h"
#include "registration_map.h"

namespace bsg {

namespace {

constexpr int kMapThreads = 256;
constexpr int kMapWaves = kMapThreads / 64;
constexpr int kMapRounds = kMapSortTile / kMapThreads;
constexpr int kMapScanThreads = 1024;      // map_scan_kernel: one workgroup walks a whole map's counts, so it is as wide as a workgroup gets
static_assert(kMapSortTile % kMapThreads == 0, "a tile is whole rounds of a workgroup");

__global__ __launch_bounds__(kMapThreads) void map_key_kernel(int n_points, int n_scans, const int* __restrict__ scan_start, const double* __restrict__ pts,
                                                               const double* __restrict__ T, double v, double* __restrict__ tq,
                                                               unsigned long long* __restrict__ key, int* __restrict__ idx,
                                                               double* __restrict__ out_pts, int* __restrict__ out_cnt, int* __restrict__ range_flag) {
  const int i = (int)(blockIdx.x * (unsigned)kMapThreads + threadIdx.x);
  if (i >= n_points) return;
  // the last scan that starts at or before i (empty scans share a start with their successor)
  int lo = 0, hi = n_scans;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (scan_start[mid] <= i) lo = mid; else hi = mid;
  }
  const double p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
  double q[3];
  map_transform(T ? T + 12 * (size_t)lo : nullptr, p, q);
  if (v == kMapMergeOnly) {
    out_pts[3 * (size_t)i] = q[0]; out_pts[3 * (size_t)i + 1] = q[1]; out_pts[3 * (size_t)i + 2] = q[2];
    out_cnt[i] = 1;
    return;
  }
  tq[3 * (size_t)i] = q[0]; tq[3 * (size_t)i + 1] = q[1]; tq[3 * (size_t)i + 2] = q[2];
  int bad = 0;
  key[i] = map_point_key(q, v, &bad);
  idx[i] = i;
  if (bad) *range_flag = 1;
}

// merge only: a map's number of output points is its number of input points
__global__ __launch_bounds__(kMapThreads) void map_copy_counts_kernel(int n_maps, const int* __restrict__ pt_start, int* __restrict__ n_vox) {
  const int m = (int)(blockIdx.x * (unsigned)kMapThreads + threadIdx.x);
  if (m < n_maps) n_vox[m] = pt_start[m + 1] - pt_start[m];
}

// what a tile's workgroup knows of itself
struct MapTile {
  int base, n, t, tiles, first_tile;      // the map's first point and number of points; the tile within the map; the map's tiles
};
__device__ __forceinline__ MapTile map_tile(const int* tile_map, const int* tile_start, const int* pt_start) {
  const int m = tile_map[blockIdx.x];
  MapTile r;
  r.first_tile = tile_start[m];
  r.t = (int)blockIdx.x - r.first_tile;
  r.tiles = tile_start[m + 1] - r.first_tile;
  r.base = pt_start[m];
  r.n = pt_start[m + 1] - r.base;
  return r;
}

__global__ __launch_bounds__(kMapThreads) void map_hist_kernel(const int* __restrict__ tile_map, const int* __restrict__ tile_start,
                                                                const int* __restrict__ pt_start, const unsigned long long* __restrict__ key, int shift,
                                                                int* __restrict__ hist) {
  __shared__ int cnt[256];
  const MapTile M = map_tile(tile_map, tile_start, pt_start);
  const int tid = (int)threadIdx.x;
  cnt[tid] = 0;
  __syncthreads();
  for (int r = 0; r < kMapRounds; ++r) {
    const int i = M.t * kMapSortTile + r * kMapThreads + tid;
    if (i < M.n) atomicAdd(&cnt[(int)((key[(size_t)M.base + i] >> shift) & 255ull)], 1);
  }
  __syncthreads();
  hist[256 * (size_t)M.first_tile + (size_t)tid * M.tiles + M.t] = cnt[tid];
}

// inclusive scan of one value per thread over a workgroup of WAVES waves; the workgroup's total through *total
template <int WAVES>
__device__ __forceinline__ int map_block_scan(int v, int* wave_tot, int* total) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off, 64);
    v += lane >= off ? o : 0;
  }
  if (lane == 63) wave_tot[wave] = v;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) { before += w < wave ? wave_tot[w] : 0; all += wave_tot[w]; }
  __syncthreads();
  *total = all;
  return v + before;
}

// One workgroup per map: the exclusive scan of the map's per * (tile_start[m + 1] - tile_start[m]) values at data + per * tile_start[m],
// in place, four per lane and round; total (optional): the map's sum.
__global__ __launch_bounds__(kMapScanThreads) void map_scan_kernel(const int* __restrict__ tile_start, int per, int* __restrict__ data, int* __restrict__ total) {
  __shared__ int wave_tot[kMapScanThreads / 64];
  const int m = (int)blockIdx.x;
  const int len = per * (tile_start[m + 1] - tile_start[m]);
  int* d = data + (size_t)per * tile_start[m];
  int carry = 0;
  for (int base = 0; base < len; base += 4 * kMapScanThreads) {
    const int at = base + 4 * (int)threadIdx.x;
    int x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = at + k < len ? d[at + k] : 0;
    const int mine = x[0] + x[1] + x[2] + x[3];
    int all;
    int run = carry + map_block_scan<kMapScanThreads / 64>(mine, wave_tot, &all) - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (at + k < len) d[at + k] = run;
      run += x[k];
    }
    carry += all;
  }
  if (total && threadIdx.x == 0) total[m] = carry;
}

__global__ __launch_bounds__(kMapThreads) void map_scatter_kernel(const int* __restrict__ tile_map, const int* __restrict__ tile_start,
                                                                   const int* __restrict__ pt_start, const unsigned long long* __restrict__ key_in,
                                                                   const int* __restrict__ idx_in, int shift, const int* __restrict__ hist,
                                                                   unsigned long long* __restrict__ key_out, int* __restrict__ idx_out) {
  __shared__ int running[256];                 // where the next key of a digit goes, within the map
  __shared__ int wave_cnt[kMapWaves][256];     // a round's keys per wave and digit
  const MapTile M = map_tile(tile_map, tile_start, pt_start);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  running[tid] = hist[256 * (size_t)M.first_tile + (size_t)tid * M.tiles + M.t];
#pragma unroll
  for (int w = 0; w < kMapWaves; ++w) wave_cnt[w][tid] = 0;
  __syncthreads();
  for (int r = 0; r < kMapRounds; ++r) {
    const int i = M.t * kMapSortTile + r * kMapThreads + tid;
    const bool valid = i < M.n;
    const unsigned long long k = valid ? key_in[(size_t)M.base + i] : 0ull;
    const int payload = valid ? idx_in[(size_t)M.base + i] : 0;
    const int d = (int)((k >> shift) & 255ull);
    unsigned long long peer = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long with = __ballot(valid && bit);
      peer &= bit ? with : ~with;
    }
    const int lower = __popcll(peer & ((1ull << lane) - 1ull));
    if (valid && lower == 0) wave_cnt[wave][d] = __popcll(peer);
    __syncthreads();
    if (valid) {
      int pos = running[d] + lower;
#pragma unroll
      for (int w = 0; w < kMapWaves; ++w) pos += w < wave ? wave_cnt[w][d] : 0;
      if ((unsigned)pos < (unsigned)M.n) {      // (always: the bases are the scan of the counts of these same digits)
        key_out[(size_t)M.base + pos] = k;
        idx_out[(size_t)M.base + pos] = payload;
      }
    }
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int w = 0; w < kMapWaves; ++w) { add += wave_cnt[w][tid]; wave_cnt[w][tid] = 0; }
    running[tid] += add;
    __syncthreads();
  }
}

__device__ __forceinline__ bool map_is_head(const unsigned long long* key, const MapTile& M, int i) {
  if (i >= M.n) return false;
  const unsigned long long k = key[(size_t)M.base + i];
  return k != kMapDropped && (i == 0 || key[(size_t)M.base + i - 1] != k);
}

__global__ __launch_bounds__(kMapThreads) void map_heads_kernel(const int* __restrict__ tile_map, const int* __restrict__ tile_start,
                                                                 const int* __restrict__ pt_start, const unsigned long long* __restrict__ key,
                                                                 int* __restrict__ tile_heads) {
  __shared__ int wave_tot[kMapWaves];
  const MapTile M = map_tile(tile_map, tile_start, pt_start);
  int mine = 0;
  for (int r = 0; r < kMapRounds; ++r) mine += map_is_head(key, M, M.t * kMapSortTile + r * kMapThreads + (int)threadIdx.x) ? 1 : 0;
  int all;
  map_block_scan<kMapWaves>(mine, wave_tot, &all);
  if (threadIdx.x == 0) tile_heads[blockIdx.x] = all;
}

// tile_heads: scanned per map (a tile's first slot within its map)
__global__ __launch_bounds__(kMapThreads) void map_centroid_kernel(const int* __restrict__ tile_map, const int* __restrict__ tile_start,
                                                                    const int* __restrict__ pt_start, const unsigned long long* __restrict__ key,
                                                                    const int* __restrict__ idx, const double* __restrict__ tq,
                                                                    const int* __restrict__ tile_heads, double* __restrict__ out_pts,
                                                                    int* __restrict__ out_cnt) {
  __shared__ int wave_tot[kMapWaves];
  const MapTile M = map_tile(tile_map, tile_start, pt_start);
  int carry = tile_heads[blockIdx.x];
  for (int r = 0; r < kMapRounds; ++r) {
    const int i = M.t * kMapSortTile + r * kMapThreads + (int)threadIdx.x;
    const bool head = map_is_head(key, M, i);
    int all;
    const int slot = carry + map_block_scan<kMapWaves>(head ? 1 : 0, wave_tot, &all) - (head ? 1 : 0);
    carry += all;
    if (!head || slot >= M.n) continue;      // (a map has at most as many voxels as points)
    const unsigned long long k = key[(size_t)M.base + i];
    double s[3] = {0.0, 0.0, 0.0}, c[3];
    int count = 0;
    for (int j = i; j < M.n && key[(size_t)M.base + j] == k; ++j, ++count) {
      const size_t p = (size_t)idx[(size_t)M.base + j];
      const double q[3] = {tq[3 * p], tq[3 * p + 1], tq[3 * p + 2]};
      map_centroid_add(s, q);
    }
    map_centroid_div(s, count, c);
    const size_t o = (size_t)M.base + (size_t)slot;
    out_pts[3 * o] = c[0]; out_pts[3 * o + 1] = c[1]; out_pts[3 * o + 2] = c[2];
    out_cnt[o] = count;
  }
}

}  // namespace

void launch_build_registration_maps(hipStream_t s, int n_maps, int n_scans, int n_points, int n_tiles, const int* scan_start, const double* points,
                                    const double* T, double v, const int* pt_start, const int* tile_start, const int* tile_map, double* tq,
                                    unsigned long long* key_a, unsigned long long* key_b, int* idx_a, int* idx_b, int* hist, int* tile_heads,
                                    double* out_pts, int* out_cnt, int* n_vox, int* range_flag) {
  if (n_maps <= 0 || n_points <= 0) return;
  (void)hipMemsetAsync(range_flag, 0, sizeof(int), s);
  const dim3 block(kMapThreads);
  hipLaunchKernelGGL(map_key_kernel, dim3((unsigned)((n_points + kMapThreads - 1) / kMapThreads)), block, 0, s, n_points, n_scans, scan_start, points, T, v,
                     tq, key_a, idx_a, out_pts, out_cnt, range_flag);
  if (v == kMapMergeOnly) {
    hipLaunchKernelGGL(map_copy_counts_kernel, dim3((unsigned)((n_maps + kMapThreads - 1) / kMapThreads)), block, 0, s, n_maps, pt_start, n_vox);
    return;
  }
  const dim3 tiles((unsigned)n_tiles), maps((unsigned)n_maps);
  for (int pass = 0; pass < 8; ++pass) {
    hipLaunchKernelGGL(map_hist_kernel, tiles, block, 0, s, tile_map, tile_start, pt_start, key_a, 8 * pass, hist);
    hipLaunchKernelGGL(map_scan_kernel, maps, dim3(kMapScanThreads), 0, s, tile_start, 256, hist, (int*)nullptr);
    hipLaunchKernelGGL(map_scatter_kernel, tiles, block, 0, s, tile_map, tile_start, pt_start, key_a, idx_a, 8 * pass, hist, key_b, idx_b);
    std::swap(key_a, key_b);
    std::swap(idx_a, idx_b);
  }
  hipLaunchKernelGGL(map_heads_kernel, tiles, block, 0, s, tile_map, tile_start, pt_start, key_a, tile_heads);
  hipLaunchKernelGGL(map_scan_kernel, maps, dim3(kMapScanThreads), 0, s, tile_start, 1, tile_heads, n_vox);
  hipLaunchKernelGGL(map_centroid_kernel, tiles, block, 0, s, tile_map, tile_start, pt_start, key_a, idx_a, tq, tile_heads, out_pts, out_cnt);
}

}  // namespace bsg
