// Scan Context place recognition (bsgpu_scan_context_describe, bsgpu_scan_context_match) — the descriptors and the search of
// RelocCandidateSearchScanContext::FindRelocCandidates (bs_models/src/lib/reloc/reloc_candidate_search_scan_context.cpp:117-150).
// The arithmetic is scan_context.h, shared with the CPU tests.
//   describe   sc_bin_kernel     grid (member, chunk): kScChunk points of a member's scan through its transform into a 1 200-bin table of
//                                integer keys in LDS (atomic max); the touched bins then into the aggregate's table (atomic max)
//              sc_keys_kernel    one workgroup per aggregate: the table as doubles, the ring key, the sector key, n_binned
//   match      sc_select_kernel  (only with a pre-selection) one workgroup per query: the ring-key distances of its set, K rounds of a
//                                (d, index) minimum, a flag per chosen candidate
//              sc_match_kernel   grid (query, block of 4 candidates): the query's descriptor, sector key and column norms in LDS; one wave
//                                per candidate, lane = the candidate's column; (distance, shift) per pair
//              sc_best_kernel    one workgroup per query: the (distance, index) minimum over its compared candidates
// No workgroup waits for another: no fences, no spinning.  The only atomics are integer maxima and one integer count per aggregate,
// whose results no order of arrival can change; every floating-point sum has the fixed order of scan_context.h.
#include "bsgpu_device.h"
#include "scan_context.h"

namespace bsg {

constexpr int kScThreads = 256;
constexpr int kScWaves = kScThreads / 64;
constexpr int kScPerLane = kScChunk / kScThreads;

// the 60-term sum: every lane of the wave gets the tree of sc_tree64 (lanes 60 .. 63 pass 0)
__device__ __forceinline__ double sc_wave_tree(double v) {
  BSG_SC_EXACT
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(kScThreads) void sc_bin_kernel(const int* scan_start, const double* points, const int* member_scan,
                                                            const int* member_agg, const double* member_T, double lidar_height,
                                                            double max_radius, unsigned long long* table, int* count) {
  __shared__ unsigned long long bins[kScBins];
  __shared__ int kept_all;
  const int m = (int)blockIdx.x, sc = member_scan[m], a = member_agg[m];
  const size_t first = (size_t)scan_start[sc];
  const int n = scan_start[sc + 1] - scan_start[sc], c0 = (int)blockIdx.y * kScChunk;   // (the host refuses a scan of more than 65 535 chunks)
  if (c0 >= n) return;
  double T[12];
#pragma unroll
  for (int t = 0; t < 12; ++t) T[t] = member_T[12 * (size_t)m + t];
  for (int b = (int)threadIdx.x; b < kScBins; b += kScThreads) bins[b] = 0ull;
  if (threadIdx.x == 0) kept_all = 0;
  __syncthreads();
  int kept = 0;
#pragma unroll 4
  for (int k = 0; k < kScPerLane; ++k) {
    const int i = c0 + k * kScThreads + (int)threadIdx.x;
    if (i < n) {
      const double* p = points + 3 * (first + (size_t)i);
      const double xyz[3] = {p[0], p[1], p[2]};
      double q[3], v;
      sc_transform(T, xyz, q);
      const int b = sc_bin(q[0], q[1], max_radius);
      if (b >= 0 && sc_point_value(q[2], lidar_height, &v)) {
        atomicMax(&bins[b], sc_key_of(v));
        ++kept;
      }
    }
  }
  __syncthreads();
  for (int b = (int)threadIdx.x; b < kScBins; b += kScThreads) {
    const unsigned long long k = bins[b];
    if (k != 0ull) atomicMax(&table[(size_t)a * kScBins + b], k);
  }
  if (kept != 0) atomicAdd(&kept_all, kept);
  __syncthreads();
  if (threadIdx.x == 0 && kept_all != 0) atomicAdd(&count[a], kept_all);
}

__global__ __launch_bounds__(kScThreads) void sc_keys_kernel(const unsigned long long* table, const int* count, double* desc, double* ring_key,
                                                             double* sector_key, int* n_binned) {
  BSG_SC_EXACT
  __shared__ double d[kScBins];
  const size_t a = blockIdx.x;
  for (int b = (int)threadIdx.x; b < kScBins; b += kScThreads) {
    const double v = sc_value_of(table[a * kScBins + b]);
    d[b] = v;
    desc[a * kScBins + b] = v;
  }
  __syncthreads();
  if (threadIdx.x < kScSectors) sector_key[a * kScSectors + threadIdx.x] = sc_mean20(d + threadIdx.x, kScSectors);
  if (threadIdx.x == 64) n_binned[a] = count[a];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int r = wave; r < kScRings; r += kScWaves) {
    const double s = sc_wave_tree(lane < kScSectors ? d[r * kScSectors + lane] : 0.0);
    if (lane == 0) ring_key[a * kScRings + r] = s / (double)kScSectors;
  }
}

// d2 / take: one entry per (query, candidate of its set), from pair_start[q]
__global__ __launch_bounds__(kScThreads) void sc_select_kernel(const int* query_set, const long long* pair_start, const double* query_desc,
                                                               const int* cand_start, const double* cand_desc, int K, double* d2,
                                                               int* take) {
  BSG_SC_EXACT
  __shared__ double qrk[kScRings];
  __shared__ double wd[kScWaves];
  __shared__ int wi[kScWaves];
  const int q = (int)blockIdx.x, s = query_set[q], c0 = cand_start[s], nc = cand_start[s + 1] - c0;
  if (K >= nc) return;                         // (the host launches this kernel only when some set is larger than K)
  const long long p0 = pair_start[q];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const double* qd = query_desc + (size_t)q * kScBins;
  for (int r = wave; r < kScRings; r += kScWaves) {
    const double t = sc_wave_tree(lane < kScSectors ? qd[r * kScSectors + lane] : 0.0);
    if (lane == 0) qrk[r] = t / (double)kScSectors;
  }
  __syncthreads();
  for (int c = wave; c < nc; c += kScWaves) {
    const double* cd = cand_desc + (size_t)(c0 + c) * kScBins;
    double acc = 0.0;
    for (int r = 0; r < kScRings; ++r) {
      const double ck = sc_wave_tree(lane < kScSectors ? cd[r * kScSectors + lane] : 0.0) / (double)kScSectors;
      acc = acc + sc_sq_diff(qrk[r], ck);
    }
    if (lane == 0) { d2[p0 + c] = sc_orderable(acc); take[p0 + c] = 0; }
  }
  __syncthreads();
  // K rounds: the least (d2, index) above the last one chosen
  const double inf = std::numeric_limits<double>::infinity();
  double last_d = -inf;
  long long last_i = -1;
  for (int k = 0; k < K; ++k) {
    double bd = inf;
    long long bi = (long long)nc;                // (above every index: what an empty lane holds)
    for (int c = (int)threadIdx.x; c < nc; c += kScThreads) {
      const double v = d2[p0 + c];
      if (sc_less(last_d, last_i, v, c) && sc_less(v, c, bd, bi)) { bd = v; bi = c; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double od = __shfl_xor(bd, off, 64);
      const long long oi = __shfl_xor(bi, off, 64);
      if (sc_less(od, oi, bd, bi)) { bd = od; bi = oi; }
    }
    if (lane == 0) { wd[wave] = bd; wi[wave] = (int)bi; }
    __syncthreads();
    bd = wd[0]; bi = wi[0];
#pragma unroll
    for (int w = 1; w < kScWaves; ++w) if (sc_less(wd[w], wi[w], bd, bi)) { bd = wd[w]; bi = wi[w]; }
    __syncthreads();
    if (bi >= nc) break;                         // (never: K < nc candidates in a total order, sc_orderable)
    if (threadIdx.x == 0) take[p0 + bi] = 1;
    last_d = bd; last_i = bi;
  }
}

__global__ __launch_bounds__(kScThreads) void sc_match_kernel(const int* query_set, const long long* pair_start, const double* query_desc,
                                                              const int* cand_start, const double* cand_desc, int K, int R, const int* take,
                                                              double* dist_all, int* shift_all) {
  BSG_SC_EXACT
  __shared__ double qd[kScBins];
  __shared__ double qk[kScSectors];
  __shared__ double qn[kScSectors];
  const int q = (int)blockIdx.x, s = query_set[q], c0 = cand_start[s], nc = cand_start[s + 1] - c0;
  if ((int)blockIdx.y * kScWaves >= nc) return;
  for (int b = (int)threadIdx.x; b < kScBins; b += kScThreads) qd[b] = query_desc[(size_t)q * kScBins + b];
  __syncthreads();
  if (threadIdx.x < kScSectors) {
    qk[threadIdx.x] = sc_mean20(qd + threadIdx.x, kScSectors);
    qn[threadIdx.x] = sc_norm20(qd + threadIdx.x, kScSectors);
  }
  __syncthreads();
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, c = (int)blockIdx.y * kScWaves + wave;
  if (c >= nc) return;
  const long long pair = pair_start[q] + c;
  const double inf = std::numeric_limits<double>::infinity();
  if (K > 0 && K < nc && take[pair] == 0) {      // left out by the pre-selection
    if (lane == 0) { dist_all[pair] = inf; shift_all[pair] = 0; }
    return;
  }
  const bool col = lane < kScSectors;
  const int i = col ? lane : 0;
  double cv[kScRings];
#pragma unroll
  for (int r = 0; r < kScRings; ++r) cv[r] = cand_desc[(size_t)(c0 + c) * kScBins + r * kScSectors + i];
  const double ck = sc_mean20(cv, 1), cn = sc_norm20(cv, 1);
  // the key alignment: the first minimum over all 60 shifts
  double best = inf;
  int shift0 = 0;
  for (int sh = 0; sh < kScSectors; ++sh) {
    const double n2 = sc_orderable(sc_wave_tree(col ? sc_sq_diff(qk[sc_wrap(i + sh)], ck) : 0.0));
    if (n2 < best) { best = n2; shift0 = sh; }
  }
  // the refinement: the window's shifts in ascending order
  double bd = inf;
  int bs = -1;
  for (int sh = 0; sh < kScSectors; ++sh) {
    if (!sc_in_window(sh, shift0, R)) continue;
    if (bs < 0) bs = sh;
    const int j = sc_wrap(i + sh);
    const double qnj = qn[j];
    const bool both = col && qnj != 0.0 && cn != 0.0;
    const double dot = sc_dot20(qd + j, kScSectors, cv, 1);
    const double sum = sc_wave_tree(both ? sc_cosine(dot, qnj, cn) : 0.0);
    const int n = __popcll(__ballot(both));
    const double d = sc_orderable(sc_shift_distance(sum, n));
    if (d < bd) { bd = d; bs = sh; }
  }
  if (lane == 0) { dist_all[pair] = bd; shift_all[pair] = bs; }
}

__global__ __launch_bounds__(kScThreads) void sc_best_kernel(const int* query_set, const long long* pair_start, const int* cand_start, int K,
                                                             double dist_thres, const int* take, const double* dist_all,
                                                             const int* shift_all, int* best_cand, double* best_dist, int* best_shift,
                                                             double* yaw) {
  BSG_SC_EXACT
  __shared__ double wd[kScWaves];
  __shared__ int wi[kScWaves];
  const int q = (int)blockIdx.x, s = query_set[q], nc = cand_start[s + 1] - cand_start[s];
  const long long p0 = pair_start[q];
  const bool select = K > 0 && K < nc;
  const double inf = std::numeric_limits<double>::infinity();
  double bd = inf;
  long long bi = (long long)nc;                  // (above every index: no compared candidate yet)
  for (int c = (int)threadIdx.x; c < nc; c += kScThreads) {
    if (select && take[p0 + c] == 0) continue;
    const double v = dist_all[p0 + c];
    if (sc_less(v, c, bd, bi)) { bd = v; bi = c; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double od = __shfl_xor(bd, off, 64);
    const long long oi = __shfl_xor(bi, off, 64);
    if (sc_less(od, oi, bd, bi)) { bd = od; bi = oi; }
  }
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (lane == 0) { wd[wave] = bd; wi[wave] = (int)bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    bd = wd[0]; bi = wi[0];
#pragma unroll
    for (int w = 1; w < kScWaves; ++w) if (sc_less(wd[w], wi[w], bd, bi)) { bd = wd[w]; bi = wi[w]; }
    const bool any = bi < nc;
    const int sh = any ? shift_all[p0 + bi] : 0;
    best_cand[q] = any && bd < dist_thres ? (int)bi : -1;
    best_dist[q] = bd;
    best_shift[q] = sh;
    yaw[q] = (double)sh * kScYawStep;
  }
}

void launch_scan_context_describe(hipStream_t s, int n_aggregates, int n_members, int max_chunks, const int* scan_start, const double* points,
                                  const int* member_scan, const int* member_agg, const double* member_T, double lidar_height,
                                  double max_radius, double* desc, double* ring_key, double* sector_key, int* n_binned,
                                  unsigned long long* table, int* count) {
  if (n_aggregates <= 0) return;
  (void)hipMemsetAsync(table, 0, sizeof(unsigned long long) * kScBins * (size_t)n_aggregates, s);
  (void)hipMemsetAsync(count, 0, sizeof(int) * (size_t)n_aggregates, s);
  if (n_members > 0 && max_chunks > 0)
    hipLaunchKernelGGL(sc_bin_kernel, dim3(n_members, max_chunks), dim3(kScThreads), 0, s, scan_start, points, member_scan,
                       member_agg, member_T, lidar_height, max_radius, table, count);
  hipLaunchKernelGGL(sc_keys_kernel, dim3(n_aggregates), dim3(kScThreads), 0, s, table, count, desc, ring_key, sector_key, n_binned);
}

void launch_scan_context_match(hipStream_t s, int n_queries, int max_cands, bool any_select, const int* query_set, const long long* pair_start,
                               const double* query_desc, const int* cand_start, const double* cand_desc, int K, int R, double dist_thres,
                               int* best_cand, double* best_dist, int* best_shift, double* yaw, double* dist_all, int* shift_all, double* d2,
                               int* take) {
  if (n_queries <= 0) return;
  if (any_select)
    hipLaunchKernelGGL(sc_select_kernel, dim3(n_queries), dim3(kScThreads), 0, s, query_set, pair_start, query_desc, cand_start, cand_desc, K, d2,
                       take);
  if (max_cands > 0)
    hipLaunchKernelGGL(sc_match_kernel, dim3(n_queries, (max_cands + kScWaves - 1) / kScWaves), dim3(kScThreads), 0, s, query_set, pair_start,
                       query_desc, cand_start, cand_desc, K, R, take, dist_all, shift_all);
  hipLaunchKernelGGL(sc_best_kernel, dim3(n_queries), dim3(kScThreads), 0, s, query_set, pair_start, cand_start, K, dist_thres, take, dist_all,
                     shift_all, best_cand, best_dist, best_shift, yaw);
}

}  // namespace bsg
