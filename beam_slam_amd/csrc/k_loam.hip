// LOAM feature registration for a batch of scan pairs (bsgpu_register_scans_loam) — the matcher_->Match() of
// MultiScanLoamRegistration::MatchScans (bs_models/src/lib/scan_registration/multi_scan_registration.cpp:497-531), ScanToMapLoamRegistration,
// RelocRefinementLoamRegistration and the submap alignments, from feature clouds.  The arithmetic of one pair is loam.h, shared with the
// CPU tests.
// A scan has a few hundred features and a local map a few thousand, so the shape is localize_kernel's, not k_gicp.hip's:
//   once per call   launch_point_grid_build  (k_point_grid.hip) the grids of every pair's two reference clouds
//                   loam_kernel              ONE workgroup of kGridChunk lanes per pair runs loam_run: every outer iteration's
//                                            correspondences and every Levenberg-Marquardt iteration of its inner solve
// The host reads nothing in between.  Correspondences: a lane per target feature, its 2- or 3-entry neighbour list in LDS (grid_knn
// indexes it at run time), the kept neighbours' indices to the pair's region of the call's scratch allocation.  Evaluation: a lane per
// measurement of a chunk, the chunk's partial record through grid_chunk_reduce, the partials added in chunk order by the lane that
// owns the sum, the 28 sums then broadcast through LDS.  The 6 x 6 part of the loop runs redundantly in every lane on those identical
// sums, so no lane waits on another except in the reductions.  Workgroups never wait on each other: no fences, no spinning; no
// floating-point atomics (the kept counts are integer LDS atomics).
// This translation unit is compiled with floating-point contraction off (Makefile): frame_lm.h's helpers have no pragma of their own,
// and the device must return the bits of the header on the host.
#include "k_point_grid.h"
#include "loam.h"

namespace bsg {

namespace {

constexpr int kLoamThreads = kGridChunk;

// loam_run's back-end of one workgroup.  Target feature i of the pair: i < n_edge the edge at te0 + i, else the surface at
// ts0 + i - n_edge (indices into the call's packed target array); lane t takes the features i = t (mod kLoamThreads), here and in the
// evaluator, so a lane reads back only what it stored itself.
struct LoamBlock {
  LoamParams P;
  int n_edge, n_surf, te0, ts0;
  const double *edges, *surfs;            // the pair's reference clouds
  const PointGrid *GE, *GS;               // their grids (in global memory: a lane picks one by the kind of its feature)
  const int* cells;
  const double* rec;
  const double* tq;                       // the call's target features under T_init
  int* corr;                              // 3 per target feature of the call
  double *ld, *li;                        // this lane's neighbour list in LDS, stride kLoamThreads
  double* total;                          // kFlmSums, LDS
  int* kept;                              // 2, LDS

  __device__ __forceinline__ size_t at(int i) const { return (size_t)(i < n_edge ? te0 + i : ts0 + (i - n_edge)); }

  __device__ void correspond(const double q[4], const double p[3], int* kept_edges, int* kept_surfs) {
    double T[12];
    loam_pose_matrix(q, p, T);
    if (threadIdx.x < 2) kept[threadIdx.x] = 0;
    __syncthreads();
    int mine_e = 0, mine_s = 0;
    for (int i = (int)threadIdx.x; i < n_edge + n_surf; i += kLoamThreads) {
      const bool edge = i < n_edge;
      const size_t f = at(i);
      double x[3];
      int c[3] = {-1, -1, -1};
      grid_apply(T, tq + 3 * f, x);
      grid_knn(*(edge ? GE : GS), cells, rec, x, edge ? kLoamEdgeK : kLoamSurfaceK, ld, li, kLoamThreads);
      const bool keep = edge ? loam_keep_edge(edges, ld, li, kLoamThreads, P.mc2, c) : loam_keep_surface(surfs, ld, li, kLoamThreads, P.mc2, c);
      corr[3 * f] = keep ? c[0] : -1; corr[3 * f + 1] = c[1]; corr[3 * f + 2] = c[2];
      mine_e += keep && edge ? 1 : 0;
      mine_s += keep && !edge ? 1 : 0;
    }
    if (mine_e) atomicAdd(&kept[0], mine_e);
    if (mine_s) atomicAdd(&kept[1], mine_s);
    __syncthreads();
    *kept_edges = kept[0]; *kept_surfs = kept[1];
    __syncthreads();      // (the next call clears the counts)
  }

  template <int REC>
  __device__ __forceinline__ void sums(const double* T, FlmSums& s) {
    __shared__ double part[REC];
    double acc = 0.0;
    for (int c = 0; c < n_edge + n_surf; c += kGridChunk) {
      const int i = c + (int)threadIdx.x;
      double t[REC];
#pragma unroll
      for (int k = 0; k < REC; ++k) t[k] = 0.0;
      if (i < n_edge + n_surf) {
        const size_t f = at(i);
        const bool edge = i < n_edge;
        const int cr[3] = {corr[3 * f], corr[3 * f + 1], corr[3 * f + 2]};
        loam_feature_term(edge, T, tq + 3 * f, cr, edge ? edges : surfs, P.loss_kind, P.loss_a, REC > 1, t);
      }
      grid_chunk_reduce<REC>(t, part);
      if (threadIdx.x < REC) acc = acc + part[threadIdx.x];      // (its own store)
      __syncthreads();                                           // (the next chunk overwrites the waves' sums)
    }
    if (threadIdx.x < REC) total[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < REC; ++k) s.v[k] = total[k];
    __syncthreads();
  }
  __device__ void operator()(const double q[4], const double p[3], bool with_J, FlmSums& s) {
    double T[12];
    loam_pose_matrix(q, p, T);
#pragma unroll
    for (int k = 0; k < kFlmSums; ++k) s.v[k] = 0.0;
    if (with_J) sums<kFlmSums>(T, s);
    else sums<1>(T, s);
  }
};

// cloud_start (2 n_pairs + 1) over the packed reference clouds [every pair's edges | every pair's surfaces], feat_start the same over
// the packed target features; out kLoamOutStride doubles per pair [T_refest_ref 12 | T_ref_tgt 12 | cov 36 | cost], out_i 5 per pair
// [n_edge, n_surf, n_iters, n_inner, status]
__global__ __launch_bounds__(kLoamThreads) void loam_kernel(int n_pairs, const int* __restrict__ cloud_start, const double* __restrict__ ref,
                                                            const int* __restrict__ feat_start, const double* __restrict__ tgt,
                                                            const double* __restrict__ T_init, const PointGrid* __restrict__ grids,
                                                            const int* __restrict__ cells, const double* __restrict__ rec, const LoamParams P,
                                                            double* __restrict__ tq, int* __restrict__ corr, double* __restrict__ out,
                                                            int* __restrict__ out_i) {
  __shared__ double lists[2 * kLoamSurfaceK * kLoamThreads];
  __shared__ double total[kFlmSums];
  __shared__ int kept[2];
  const int p = (int)blockIdx.x;
  LoamBlock b;
  b.P = P;
  b.te0 = feat_start[p]; b.n_edge = feat_start[p + 1] - b.te0;
  b.ts0 = feat_start[n_pairs + p]; b.n_surf = feat_start[n_pairs + p + 1] - b.ts0;
  b.edges = ref + 3 * (size_t)cloud_start[p]; b.surfs = ref + 3 * (size_t)cloud_start[n_pairs + p];
  b.GE = grids + p; b.GS = grids + n_pairs + p;
  b.cells = cells; b.rec = rec; b.tq = tq; b.corr = corr;
  b.ld = lists + threadIdx.x; b.li = lists + kLoamSurfaceK * kLoamThreads + threadIdx.x;
  b.total = total; b.kept = kept;
  double Ti[12];
#pragma unroll
  for (int t = 0; t < 12; ++t) Ti[t] = T_init[12 * p + t];
  // the target features under T_init, once
  for (int i = (int)threadIdx.x; i < b.n_edge + b.n_surf; i += kLoamThreads) {
    const size_t f = b.at(i);
    double x[3];
    grid_apply(Ti, tgt + 3 * f, x);
    tq[3 * f] = x[0]; tq[3 * f + 1] = x[1]; tq[3 * f + 2] = x[2];
  }
  __syncthreads();
  LoamResult res;
  loam_run(P, b, res);
  if (threadIdx.x == 0) {
    double* o = out + (size_t)kLoamOutStride * p;
    double A[12], B[12];
    loam_outputs(res.q, res.p, Ti, A, B);
#pragma unroll
    for (int t = 0; t < 12; ++t) { o[t] = A[t]; o[12 + t] = B[t]; }
#pragma unroll
    for (int t = 0; t < 36; ++t) o[24 + t] = res.cov[t];
    o[60] = res.cost;
    int* oi = out_i + 5 * p;
    oi[0] = res.n_edge; oi[1] = res.n_surf; oi[2] = res.n_iters; oi[3] = res.n_inner; oi[4] = res.status;
  }
}

}  // namespace

void launch_register_scans_loam(hipStream_t s, int n_pairs, int max_points, int n_points, int n_tiles, const int* cloud_start, const double* ref,
                                const double* T_cloud, const PointGrid* grids, const int* feat_start, const double* tgt, const double* T_init,
                                const LoamParams& P, double* out, int* out_i, double* rq, int* tcell, int* cells, int* tile_sum, double* rec,
                                double* tq, int* corr) {
  if (n_pairs <= 0) return;
  launch_point_grid_build(s, 2 * n_pairs, max_points, n_points, n_tiles, cloud_start, ref, T_cloud, grids, rq, tcell, cells, tile_sum, rec);
  hipLaunchKernelGGL(loam_kernel, dim3(n_pairs), dim3(kLoamThreads), 0, s, n_pairs, cloud_start, ref, feat_start, tgt, T_init, grids, cells, rec, P,
                     tq, corr, out, out_i);
}

}  // namespace bsg
