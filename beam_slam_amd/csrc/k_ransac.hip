// Five-point RANSAC track screening for a batch of match sets (bsgpu_essential_ransac): the cv::findEssentialMat call of
// VisualOdometry::AddMeasurementsToContainer (bs_models/src/visual_odometry.cpp:481-527), five_point.h's loop on the device.
//
// One launch, one 256-thread workgroup per match set, every RANSAC round inside the kernel.  A round evaluates kRsSamples = 16
// consecutive samples, one per group of 16 lanes, all of whose working memory is LDS (five_point.h's blocks take pointers):
//   1. lane 0 of the group draws the sample, normalises its five matches and builds the orthonormal null-space basis;
//   2. lanes 0..9 each form one row of the 10 x 20 constraint system in registers and eliminate it across the group — the pivot is
//      found by a butterfly, the pivot row travels by __shfl — once per choice of the hidden coordinate; the smallest result is kept;
//   3. lane 0 expands det B(z); lanes 0..10 fill the derivative table;
//   4. ten levels of derivative bracketing, an interval per lane; the roots are compacted in lane order through a ballot;
//   5. a root per lane is back-substituted and polished; the solutions are ranked by E[0] into the round's hypothesis table.
// All 256 threads then score every hypothesis of the round against the set's matches (a match per thread, inlier counts by ballot
// and integer LDS atomics, so the counts do not depend on any order), and thread 0 applies the round's improving updates in sample
// order, ignoring the samples at or past the iteration bound then in force: the serial loop of the contract, whatever the round size.
// Workgroups never wait on each other: a set's results are the same bits alone or in a batch.
#include "bsgpu_device.h"
#include "five_point.h"

namespace bsg {

namespace {

constexpr int kRsThreads = 256;
constexpr int kRsGroup = 16;
constexpr int kRsSamples = kRsThreads / kRsGroup;
constexpr int kRsWork = kFprWork + 1;   // odd stride: the groups' rows start on different banks

struct RsShared {
  double work[kRsSamples][kRsWork];
  double hyp[kRsSamples][kFprMaxSol * 9];
  double key[kRsSamples][kRsGroup];
  double best_E[9];
  int idx[kRsSamples][5];
  int ok[kRsSamples], cyc[kRsSamples], nsol[kRsSamples];
  int count[kRsSamples * kFprMaxSol];
  int best_idx[5];
  int niters, best, consumed;
};

// Gauss-Jordan on the first ten columns with a row per lane (lanes 0..9 of a 16-lane group): pivot_col is the column the lane's row
// ends up leading.  false (group-uniform): a zero or non-finite pivot.
__device__ __forceinline__ bool rs_eliminate(double (&row)[20], int l, int& pivot_col) {
  bool good = true;
  pivot_col = -1;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    double bv = (l < 10 && pivot_col < 0) ? fabs(row[k]) : -1.0;
    int bl = l;
#pragma unroll
    for (int o = kRsGroup / 2; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o, kRsGroup);
      const int ol = __shfl_xor(bl, o, kRsGroup);
      if (ov > bv || (ov == bv && ol < bl)) { bv = ov; bl = ol; }
    }
    good = good && bv > 0.0 && isfinite(bv);
    const double inv = 1.0 / __shfl(row[k], bl, kRsGroup);
    const double f = row[k];
    const bool mine = l == bl;
    if (mine) pivot_col = k;
#pragma unroll
    for (int j = k; j < 20; ++j) {
      const double p = __shfl(row[j], bl, kRsGroup) * inv;
      row[j] = mine ? p : fma(-f, p, row[j]);
    }
  }
  return good;
}

__global__ void __launch_bounds__(kRsThreads) ransac_kernel(const int* __restrict__ match_start, const double2* __restrict__ px_prev,
                                                            const double2* __restrict__ px_cur, const double* __restrict__ Ks,
                                                            double prob, double threshold_px, int max_iters, unsigned long long seed,
                                                            unsigned char* __restrict__ mask, double* __restrict__ out_E,
                                                            int* __restrict__ out_i) {
  __shared__ RsShared sh;
  const int set = blockIdx.x, tid = threadIdx.x, g = tid / kRsGroup, l = tid % kRsGroup;
  const int m0 = match_start[set], n = match_start[set + 1] - m0;
  const double K[4] = {Ks[4 * set], Ks[4 * set + 1], Ks[4 * set + 2], Ks[4 * set + 3]};
  int* oi = out_i + kRansacOutInts * set;
  if (n < 5) {   // no model: "erase nothing"
    for (int i = tid; i < n; i += kRsThreads) mask[m0 + i] = 1;
    if (tid < 9) out_E[9 * set + tid] = 0.0;
    if (tid == 0) { oi[0] = 0; oi[1] = 0; oi[7] = FPR_TOO_FEW; }
    if (tid < 5) oi[2 + tid] = -1;
    return;
  }
  const double thr2 = fpr_threshold_sq(K, threshold_px);
  if (tid == 0) { sh.niters = max_iters; sh.best = 0; sh.consumed = 0; }
  if (tid < 9) sh.best_E[tid] = 0.0;
  if (tid < 5) sh.best_idx[tid] = -1;
  __syncthreads();
  double* w = sh.work[g];
  const double* Eb = w + kFprQ + 45;
  for (int base = 0;; base += kRsSamples) {
    const int niters = sh.niters;
    if (base >= niters) break;
    const int s = base + g;
    // 1. the sample and its null space
    if (l == 0) {
      bool ok = false;
      if (s < niters) {
        fpr_sample(seed, (uint64_t)set, (uint64_t)s, n, sh.idx[g]);
        for (int k = 0; k < 5; ++k) {
          const double2 a = px_prev[m0 + sh.idx[g][k]], b = px_cur[m0 + sh.idx[g][k]];
          const double pa[2] = {a.x, a.y}, pb[2] = {b.x, b.y};
          double m[4];
          fpr_normalize(K, pa, pb, m);
          fpr_epipolar_row(m, w + kFprQ + 9 * k);
        }
        ok = fpr_nullspace(w + kFprQ);
      }
      sh.ok[g] = ok ? 1 : 0;
    }
    __syncthreads();
    // 2. the constraint rows and their elimination, for each choice of the hidden coordinate
    {
      const bool ok = sh.ok[g] != 0;
      double keep[10], growth = INFINITY;
      int keep_col = -1, cyc = -1;
#pragma unroll 1
      for (int v = 0; v < 3; ++v) {
        double row[20];
        if (ok && l < 10) {
          fpr_constraint_row(Eb, v, l, row);
        } else {
#pragma unroll
          for (int j = 0; j < 20; ++j) row[j] = 0.0;
        }
        int col;
        const bool good = rs_eliminate(row, l, col);
        double gv = 0.0;
        if (col >= 4) {
#pragma unroll
          for (int j = 10; j < 20; ++j) gv = fpr_growth(gv, row[j]);
        }
#pragma unroll
        for (int o = kRsGroup / 2; o > 0; o >>= 1) gv = fmax(gv, __shfl_xor(gv, o, kRsGroup));   // (inf wins; a NaN cannot arise)
        if (!good || !ok) gv = INFINITY;
        if (gv < growth) {
          growth = gv; cyc = v; keep_col = col;
#pragma unroll
          for (int j = 0; j < 10; ++j) keep[j] = row[10 + j];
        }
      }
      if (cyc >= 0 && keep_col >= 4) {
#pragma unroll
        for (int j = 0; j < 10; ++j) w[kFprR + 10 * (keep_col - 4) + j] = keep[j];
      }
      if (l == 0) sh.cyc[g] = cyc;
    }
    __syncthreads();
    // 3. det B(z) and the derivative table
    const int cyc = sh.cyc[g];
    if (l == 0) {
      const bool ok = cyc >= 0 && fpr_det_poly(w + kFprR, w + kFprB, w + kFprRoots);
      sh.ok[g] = ok ? 1 : 0;
      if (ok) w[kFprRoots + 11] = fpr_root_bound(w + kFprRoots);
    }
    __syncthreads();
    const bool ok = sh.ok[g] != 0;
    const double ci = ok && l < 11 ? w[kFprRoots + l] : 0.0;
    const double bound = ok ? w[kFprRoots + 11] : 0.0;
    if (ok && l < 11) fpr_deriv_column(ci, l, w + kFprD);
    __syncthreads();
    // 4. the real roots, level by level
    int n_roots = 0, buf = 0;
    const int shift = kRsGroup * ((tid & 63) / kRsGroup);
#pragma unroll 1
    for (int k = 9; k >= 0; --k) {
      const double* prev = w + kFprRoots + 12 * buf;
      double* cur = w + kFprRoots + 12 * (buf ^ 1);
      bool found = false;
      double r = 0.0;
      if (ok && l <= n_roots) {
        const double lo = l == 0 ? -bound : prev[l - 1], hi = l == n_roots ? bound : prev[l];
        found = fpr_interval_root(w + kFprD + fpr_level(k), 10 - k, lo, hi, &r);
      }
      const unsigned bits = (unsigned)((__ballot(found) >> shift) & 0xFFFFull);
      if (found) cur[__popc(bits & ((1u << l) - 1u))] = r;
      n_roots = __popc(bits);
      buf ^= 1;
      __syncthreads();
    }
    // 5. a solution per root, ranked by E[0]
    {
      double E[9];
      bool has = false;
      if (ok && l < n_roots) has = fpr_backsub(w + kFprB, Eb, cyc, w[kFprRoots + 12 * buf + l], E);
      const double key = has ? E[0] : INFINITY;
      sh.key[g][l] = key;
      for (int i = tid; i < kRsSamples * kFprMaxSol; i += kRsThreads) sh.count[i] = 0;
      __syncthreads();
      int rank = 0;
#pragma unroll
      for (int j = 0; j < kRsGroup; ++j) {
        const double kj = sh.key[g][j];
        rank += (kj < key || (kj == key && j < l)) ? 1 : 0;
      }
      if (has) {
#pragma unroll
        for (int e = 0; e < 9; ++e) sh.hyp[g][9 * rank + e] = E[e];
      }
      const unsigned bits = (unsigned)((__ballot(has) >> shift) & 0xFFFFull);
      if (l == 0) sh.nsol[g] = s < niters ? __popc(bits) : 0;
    }
    __syncthreads();
    // the round's hypotheses against every match
    for (int i0 = 0; i0 < n; i0 += kRsThreads) {
      const int i = i0 + tid;
      const bool valid = i < n;
      double m[4] = {0.0, 0.0, 0.0, 0.0};
      if (valid) {
        const double2 a = px_prev[m0 + i], b = px_cur[m0 + i];
        const double pa[2] = {a.x, a.y}, pb[2] = {b.x, b.y};
        fpr_normalize(K, pa, pb, m);
      }
      for (int sg = 0; sg < kRsSamples; ++sg) {
        const int ns = sh.nsol[sg];
        for (int h = 0; h < ns; ++h) {
          const bool inl = valid && fpr_sampson_sq(sh.hyp[sg] + 9 * h, m[0], m[1], m[2], m[3]) <= thr2;
          const int cnt = __popcll(__ballot(inl));
          if ((tid & 63) == 0 && cnt > 0) atomicAdd(&sh.count[sg * kFprMaxSol + h], cnt);
        }
      }
    }
    __syncthreads();
    // the improving updates, in sample order
    if (tid == 0) {
      int nit = niters, best = sh.best, consumed = sh.consumed, pick = -1;
      for (int sg = 0; sg < kRsSamples && base + sg < nit; ++sg) {
        consumed = base + sg + 1;
        for (int h = 0; h < sh.nsol[sg]; ++h) {
          const int c = sh.count[sg * kFprMaxSol + h];
          if (c > (best > 4 ? best : 4)) {
            best = c; pick = sg * kFprMaxSol + h;
            nit = fpr_update_niters(prob, (double)(n - c) / (double)n, nit);
          }
        }
      }
      if (pick >= 0) {
        const int sg = pick / kFprMaxSol, h = pick % kFprMaxSol;
        for (int e = 0; e < 9; ++e) sh.best_E[e] = sh.hyp[sg][9 * h + e];
        for (int k = 0; k < 5; ++k) sh.best_idx[k] = sh.idx[sg][k];
      }
      sh.niters = nit; sh.best = best; sh.consumed = consumed;
    }
    __syncthreads();
  }
  // the best model's inlier set; without a model "erase nothing"
  const int best = sh.best;
  double E[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] = sh.best_E[e];
  for (int i = tid; i < n; i += kRsThreads) {
    unsigned char keep = 1;
    if (best > 0) {
      const double2 a = px_prev[m0 + i], b = px_cur[m0 + i];
      const double pa[2] = {a.x, a.y}, pb[2] = {b.x, b.y};
      double m[4];
      fpr_normalize(K, pa, pb, m);
      keep = fpr_sampson_sq(E, m[0], m[1], m[2], m[3]) <= thr2 ? 1 : 0;
    }
    mask[m0 + i] = keep;
  }
  if (tid < 9) out_E[9 * set + tid] = sh.best_E[tid];
  if (tid < 5) oi[2 + tid] = sh.best_idx[tid];
  if (tid == 0) { oi[0] = best; oi[1] = sh.consumed; oi[7] = best > 0 ? FPR_OK : FPR_NO_MODEL; }
}

}  // namespace

void launch_essential_ransac(hipStream_t s, int n_sets, const int* match_start, const double2* px_prev, const double2* px_cur,
                             const double* K, double prob, double threshold_px, int max_iters, uint64_t seed, unsigned char* mask,
                             double* out_E, int* out_i) {
  if (n_sets <= 0) return;
  hipLaunchKernelGGL(ransac_kernel, dim3(n_sets), dim3(kRsThreads), 0, s, match_start, px_prev, px_cur, K, prob, threshold_px, max_iters,
                     (unsigned long long)seed, mask, out_E, out_i);
}

}  // namespace bsg
