// Batched marginal covariance requests (bsgpu_covariance_requests, fuse_core::Graph::getCovariance(requests, matrices)) for any block.
// With H = [[A, W^T], [W, V]] (V block-diagonal over the eliminated landmarks), S = A - W^T V^-1 W = L L^T the reduced system and
// G_l^T = V_l^-1 W_l the border rows of an eliminated landmark l:
//   pose-side block p:   z_p = L^-1 e_p                       Sigma(p, p') = z_p^T z_p'
//   eliminated l:        y_l = L^-1 G_l                       Sigma(l, p)  = -y_l^T z_p
//                                                             Sigma(l, l') = [l == l'] V_l^-1 + y_l^T y_l'
// The rows e_p / G_l^T are written into the rhs tile of S (cov_rows), forward-substituted by the factorisation with the tile, copied
// out per pass, and every requested block is formed from the kept rows in one launch (cov_gram).
//   cov_rows   one wave per entry: a unit entry, a Euclidean landmark (3 rows: Linv^T Linv sum_f B_f^T A_f over its factors, read from
//              the robustified J / JB the undamped assembly's evaluation left) or an inverse-depth scalar (1 row: linv u_v over its
//              views, from IdpElim::U).  A landmark owns its rows: no atomics.
//   cov_gram   one wave per request: ta x tb dot products over the kept rows, reduced across the wave with DPP row operations.
#include "bsgpu_device.h"

namespace bsg {

__global__ __launch_bounds__(64) void cov_rows_kernel(double* __restrict__ S, int ld, int rhs_row, const CovRow* __restrict__ rows,
                                                      const int* __restrict__ dpos, const int* __restrict__ lm_start, const double* __restrict__ J, int ja,
                                                      const double* __restrict__ JB, const int* __restrict__ cam_pose, const int* __restrict__ cp_tq,
                                                      const int* __restrict__ cp_tp, const double* __restrict__ Linv, const int* __restrict__ view_start,
                                                      const int* __restrict__ view_cp, const int* __restrict__ icp_tq, const int* __restrict__ icp_tp,
                                                      const double* __restrict__ U, const double* __restrict__ idp_linv) {
  const CovRow e = rows[blockIdx.x];
  const int lane = threadIdx.x;
  if (e.kind == kCovUnit) {
    if (lane == 0) S[(size_t)(rhs_row + e.row) * ld + e.index] = 1.0;
    return;
  }
  if (e.kind == kCovIdp) {
    // V^-1 W = linv^2 sum_f w_f^T A_f = linv u_v per view; lane j of the first 6 takes the views in order (two camera poses of one
    // orientation add to the same entry from the same lane)
    if (lane >= 6) return;
    const double li = idp_linv[e.index];
    double* out = S + (size_t)(rhs_row + e.row) * ld;
    for (int v = view_start[e.index]; v < view_start[e.index + 1]; ++v) {
      const int cp = view_cp[v];
      const int tb = lane < 3 ? icp_tq[cp] : icp_tp[cp];
      if (tb < 0) continue;
      out[dpos[tb + (lane % 3)]] += li * U[(size_t)v * 8 + lane];
    }
    return;
  }
  // Euclidean landmark: lane (i, j) of the first 18 owns entry j of the camera-pose part of row i; the factors are taken in order, so
  // two factors of one camera pose (or two camera poses of one orientation) add to the same entry from the same lane
  if (lane >= 18) return;
  const int i = lane / 6, j = lane % 6;
  const double* Li = Linv + (size_t)e.index * kLmRec;   // lower triangular: Li0 | Li1 Li2 | Li3 Li4 Li5
  const double L[3][3] = {{Li[0], 0.0, 0.0}, {Li[1], Li[2], 0.0}, {Li[3], Li[4], Li[5]}};
  double vi[3];   // row i of V^-1 = Linv^T Linv
#pragma unroll
  for (int b = 0; b < 3; ++b) vi[b] = L[0][i] * L[0][b] + L[1][i] * L[1][b] + L[2][i] * L[2][b];
  double* out = S + (size_t)(rhs_row + e.row + i) * ld;
  const int beg = lm_start[e.index], end = lm_start[e.index + 1];
  for (int f = beg; f < end; ++f) {
    const int cp = cam_pose[f];
    const int tb = j < 3 ? cp_tq[cp] : cp_tp[cp];
    if (tb < 0) continue;
    const double* B = JB + (size_t)f * 6;        // [B row 0 | B row 1]
    const double s0 = vi[0] * B[0] + vi[1] * B[1] + vi[2] * B[2];
    const double s1 = vi[0] * B[3] + vi[1] * B[4] + vi[2] * B[5];
    double* o = out + dpos[tb + (j % 3)];
    *o += s0 * pose_part_entry(J, JB, ja, f, 0, j) + s1 * pose_part_entry(J, JB, ja, f, 1, j);
  }
}

void launch_cov_rows(hipStream_t s, double* S, int ld, int rhs_row, const CovRow* rows, int n_rows, const int* dpos, const Visual& v, const IdpElim& e) {
  (void)hipMemsetAsync(S + (size_t)rhs_row * ld, 0, sizeof(double) * 64 * (size_t)ld, s);
  if (n_rows <= 0) return;
  hipLaunchKernelGGL(cov_rows_kernel, dim3(n_rows), dim3(64), 0, s, S, ld, rhs_row, rows, dpos, v.lm_start, v.J, v.ja, v.JB, v.cam_pose, v.cp_tq, v.cp_tp,
                     v.Linv, e.view_start, e.view_cp, e.cp_tq, e.cp_tp, e.U, e.linv);
}

// sum over the 64 lanes: within each row of 16 by DPP (quad_perm xor 1, xor 2, then row_ror 4 and 8), across the four rows by two swaps
BSG_DEV double wave_sum_dpp(double v) {
  v += __builtin_amdgcn_update_dpp(0.0, v, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0.0, v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0.0, v, 0x124, 0xf, 0xf, false);  // row_ror:4
  v += __builtin_amdgcn_update_dpp(0.0, v, 0x128, 0xf, 0xf, false);  // row_ror:8
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// one wave per request (4 to a workgroup): every lane keeps the <= 4 x 4 partial dot products of its columns
__global__ __launch_bounds__(256) void cov_gram_kernel(const CovReq* __restrict__ req, int n_req, const double* __restrict__ Y, int ldy, int n_cols,
                                                       const double* __restrict__ lm_linv, const double* __restrict__ idp_linv, double* __restrict__ out) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= n_req) return;
  const CovReq q = req[w];
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  const double* ya = Y + (size_t)q.ra * ldy;
  const double* yb = Y + (size_t)q.rb * ldy;
  for (int k = lane; k < n_cols; k += 64) {
    double a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = i < q.ta ? ya[(size_t)i * ldy + k] : 0.0;
      b[i] = i < q.tb ? yb[(size_t)i * ldy + k] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = wave_sum_dpp(acc[i][j]);
  if (lane != 0) return;
  double vinv[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (q.lm_kind == kCovLandmark) {
    const double* Li = lm_linv + (size_t)q.lm_index * kLmRec;
    const double L[3][3] = {{Li[0], 0.0, 0.0}, {Li[1], Li[2], 0.0}, {Li[3], Li[4], Li[5]}};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) vinv[i][j] = L[0][i] * L[0][j] + L[1][i] * L[1][j] + L[2][i] * L[2][j];
  } else if (q.lm_kind == kCovIdp) {
    const double li = idp_linv[q.lm_index];
    vinv[0][0] = li * li;
  }
  double* o = out + q.out;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i < q.ta && j < q.tb) o[i * q.tb + j] = q.sign * acc[i][j] + (i < 3 && j < 3 ? vinv[i][j] : 0.0);
}

void launch_cov_gram(hipStream_t s, const CovReq* req, int n_req, const double* Y, int ldy, int n_cols, const double* lm_linv, const double* idp_linv,
                     double* out) {
  if (n_req <= 0) return;
  hipLaunchKernelGGL(cov_gram_kernel, dim3((n_req + 3) / 4), dim3(256), 0, s, req, n_req, Y, ldy, n_cols, lm_linv, idp_linv, out);
}

}  // namespace bsg
