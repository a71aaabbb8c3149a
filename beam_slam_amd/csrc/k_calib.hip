// Online calibration of the camera extrinsics on gfx950: a window whose BSGPU_F_REPROJ_ONLINE_CALIB factors name ONE free pair
// (q_BASELINK_CAM, p_BASELINK_CAM).  The pair's up to six tangent columns e are pose-side columns that every such factor touches:
// a border of the reduced camera system.
//   calib_refresh      the pair's derived camera entries (R_cb, t_cb) from the value vector the next reprojection launch reads
//   calib_E            per factor the robustified 2x6 block E = d r / d e (calib_body.h)                          HBM-bound
//   calib_border       per landmark G = sum C^T E, per factor E~ = E - C G; S(e,e), rhs(e), g_e, diag(H)_e      HBM-bound
//   calib_pose         per camera pose i: S(i,e) = sum A^T E~
//   calib_backsub_mcc  landmark back-substitution and model cost change with the E y_e terms
// Everything that shares a destination is summed on chip before it touches memory.  S(e,e), rhs(e), g_e and diag(H)_e, which every
// workgroup adds to, leave as one row of partials per workgroup and are summed in a fixed order (as mcc_part is): the same bits from
// run to run; S(i,e) takes one FP64 atomic per segment (<= 256 factors of one camera pose) and entry.
#include "bsgpu_device.h"
#include "calib_body.h"

namespace bsg {

__global__ void calib_refresh_kernel(Calib cb, const double* __restrict__ x, DevCamera* __restrict__ cams) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= cb.n_cam) return;
  const double q[4] = {x[cb.xq], x[cb.xq + 1], x[cb.xq + 2], x[cb.xq + 3]};
  const double p[3] = {x[cb.xp], x[cb.xp + 1], x[cb.xp + 2]};
  double R[9], t[3];
  calib_camera(q, p, R, t);
  DevCamera& d = cams[cb.cam_id[i]];
#pragma unroll
  for (int k = 0; k < 9; ++k) d.R[k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) d.t[k] = t[k];
}
void launch_calib_refresh(hipStream_t s, const Calib& cb, const double* x, DevCamera* cams) {
  if (!cb.on || cb.n_cam <= 0) return;
  hipLaunchKernelGGL(calib_refresh_kernel, dim3((cb.n_cam + 63) / 64), dim3(64), 0, s, cb, x, cams);
}

// One factor per lane; the wave's 64 rows of 12 doubles leave through LDS as contiguous 16-byte-per-lane stores.
// Algorithmic bytes per factor: 16 (idx + meta) + 16 (pixel) + 8 (w) + 1 (flag) streamed in, 96 (E) out = 137, and 80 gathered from x
// (q 32, t 24, P 24: every parameter block once in distinct bytes) plus the camera (128) and loss (16) entries, a handful of lines.
__global__ __launch_bounds__(256) void calib_E_kernel(Calib cb, int n, const int4* __restrict__ fac, const double2* __restrict__ pix,
                                                      const double* __restrict__ wgt, const double* __restrict__ x,
                                                      const DevCamera* __restrict__ cams, const DevLoss* __restrict__ losses) {
  __shared__ __attribute__((aligned(16))) double sE[4 * 64 * 12];
  const int f = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double E[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) E[i] = 0.0;
  if (f < n && cb.has[f]) {
    const int4 fc = fac[f];
    const double2 z = pix[f];
    const int cam_id = fc.w & ((1 << kMetaCamBits) - 1);
    const int loss_id = (fc.w >> kMetaCamBits) & ((1 << kMetaLossBits) - 1);
    const DevCamera cam = cams[cam_id];
    const DevLoss L = losses[loss_id];
    const double q[4] = {x[fc.x], x[fc.x + 1], x[fc.x + 2], x[fc.x + 3]};
    const double t[3] = {x[fc.y], x[fc.y + 1], x[fc.y + 2]};
    const double P[3] = {x[fc.z], x[fc.z + 1], x[fc.z + 2]};
    calib_E(q, t, P, cam.R, cam.t, cam.fx, cam.fy, cam.cx, cam.cy, z.x, z.y, wgt[f], L.kind, L.a, cb.tq >= 0, cb.tp >= 0, E);
  }
  double* sw = sE + wave * (64 * 12);
#pragma unroll
  for (int i = 0; i < 12; ++i) sw[lane * 12 + i] = E[i];
  __syncthreads();
  const int fb = blockIdx.x * 256 + wave * 64;
  const int cnt = min(64, n - fb);
  if (cnt > 0) {
    double2* dst = reinterpret_cast<double2*>(cb.E + (size_t)fb * 12);
    const double2* src = reinterpret_cast<const double2*>(sw);
#pragma unroll
    for (int it = 0; it < 6; ++it) {
      const int e = it * 64 + lane;
      if (e < cnt * 6) dst[e] = src[e];
    }
  }
}
void launch_calib_E(hipStream_t s, const Visual& v, const Calib& cb, const double* x, const DevCamera* cams, const DevLoss* losses) {
  if (!cb.on || v.n <= 0) return;
  hipLaunchKernelGGL(calib_E_kernel, dim3((v.n + 255) / 256), dim3(256), 0, s, cb, v.n, v.fac, v.pix, v.w, x, cams, losses);
}

// tangent index of border column c (0..2: theta, 3..5: p), -1 when that block is constant
BSG_DEV int calib_col(const Calib& cb, int c) { return c < 3 ? (cb.tq < 0 ? -1 : cb.tq + c) : (cb.tp < 0 ? -1 : cb.tp + c - 3); }

BSG_DEV void calib_load_row12(const double* __restrict__ p, double (&o)[12]) {
  const double2* p2 = reinterpret_cast<const double2*>(p);
#pragma unroll
  for (int i = 0; i < 6; ++i) { const double2 v = p2[i]; o[2 * i] = v.x; o[2 * i + 1] = v.y; }
}

// what one factor adds to the border's own sums: [0, 21) lower triangle of E^T E~, [21, 27) E~^T r, [27, 33) E^T r, [33, 39) diag(E^T E)
constexpr int kCalibSums = 39;
static_assert(kCalibSums <= kCalibPartStride, "a row of partials holds every sum");
BSG_DEV void calib_accumulate(const double (&E)[12], const double (&Et)[12], const double2 rf, double (&acc)[kCalibSums]) {
  int q = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c <= a; ++c) acc[q++] += E[a] * Et[c] + E[6 + a] * Et[6 + c];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    acc[21 + c] += Et[c] * rf.x + Et[6 + c] * rf.y;
    acc[27 + c] += E[c] * rf.x + E[6 + c] * rf.y;
    acc[33 + c] += E[c] * E[c] + E[6 + c] * E[6 + c];
  }
}

// Workgroups [0, lm_blocks): 8 lanes per eliminated landmark (as landmark_kernel): G_l = sum_f C_f^T E_f (3x6; C = B L^-T from the C rows),
// then E~_f = E_f - C_f G_l.  Workgroups behind them: the factors of constant landmarks, one per lane (G = 0, E~ = E).
// The 39 sums of a workgroup meet in LDS and leave as one row of cb.part; calib_border_sum_kernel adds the rows up.
// Algorithmic bytes per factor: 48 (C of the C row) + 96 (E) + 16 (r) in, 96 (E~) out = 256 (C and E are read again by the second pass,
// from cache: a landmark's rows were just touched by the same lanes); 320 per workgroup of partials.
__global__ __launch_bounds__(256) void calib_border_kernel(Calib cb, int n_lm, int lm_blocks, int n_elim, int n, const int* __restrict__ lm_start,
                                                           const double2* __restrict__ r, const double* __restrict__ CR) {
  __shared__ double ssum[4][kCalibSums + 1];
  double acc[kCalibSums];
#pragma unroll
  for (int i = 0; i < kCalibSums; ++i) acc[i] = 0.0;
  if ((int)blockIdx.x < lm_blocks) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int l = gid >> 3, sub = gid & 7;
    int beg = 0, end = 0;
    if (l < n_lm) { beg = lm_start[l]; end = lm_start[l + 1]; }
    double G[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) G[i] = 0.0;
    for (int f = beg + sub; f < end; f += 8) {
      const double2* C2 = reinterpret_cast<const double2*>(CR + (size_t)f * 8);
      const double2 ca = C2[0], cb2 = C2[1], cc = C2[2];
      const double C[6] = {ca.x, ca.y, cb2.x, cb2.y, cc.x, cc.y};
      double E[12];
      calib_load_row12(cb.E + (size_t)f * 12, E);
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 6; ++c) G[j * 6 + c] += C[j] * E[c] + C[3 + j] * E[6 + c];
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1)
#pragma unroll
      for (int i = 0; i < 18; ++i) G[i] += __shfl_xor(G[i], o, 8);
    for (int f = beg + sub; f < end; f += 8) {
      const double2* C2 = reinterpret_cast<const double2*>(CR + (size_t)f * 8);
      const double2 ca = C2[0], cb2 = C2[1], cc = C2[2];
      const double C[6] = {ca.x, ca.y, cb2.x, cb2.y, cc.x, cc.y};
      double E[12], Et[12];
      calib_load_row12(cb.E + (size_t)f * 12, E);
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int c = 0; c < 6; ++c) Et[6 * k + c] = E[6 * k + c] - (C[3 * k] * G[c] + C[3 * k + 1] * G[6 + c] + C[3 * k + 2] * G[12 + c]);
      double2* o2 = reinterpret_cast<double2*>(cb.Et + (size_t)f * 12);
#pragma unroll
      for (int i = 0; i < 6; ++i) o2[i] = make_double2(Et[2 * i], Et[2 * i + 1]);
      calib_accumulate(E, Et, r[f], acc);
    }
  } else {
    const int f = n_elim + ((int)blockIdx.x - lm_blocks) * 256 + (int)threadIdx.x;
    if (f < n) {
      double E[12];
      calib_load_row12(cb.E + (size_t)f * 12, E);
      double2* o2 = reinterpret_cast<double2*>(cb.Et + (size_t)f * 12);
#pragma unroll
      for (int i = 0; i < 6; ++i) o2[i] = make_double2(E[2 * i], E[2 * i + 1]);
      calib_accumulate(E, E, r[f], acc);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kCalibSums; ++i) {
    const double t = wave_sum(acc[i]);
    if (lane == 0) ssum[wave][i] = t;
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i < kCalibSums) cb.part[(size_t)blockIdx.x * kCalibPartStride + i] = ssum[0][i] + ssum[1][i] + ssum[2][i] + ssum[3][i];
}

// Workgroup i adds up sum i of every workgroup of calib_border_kernel, in a fixed order, and adds it where it belongs: S(e,e) (the lower
// triangle, mirrored), the rhs row, the raw gradient, diag(H) — through the plan's permutation like every other writer of S.  One add per
// destination: nothing else of this launch writes there.  grad_only: the S(e,e) entries are skipped (no factorisation follows).
__global__ __launch_bounds__(256) void calib_border_sum_kernel(Calib cb, int n_part, double* __restrict__ S, int ld, int rhs_row,
                                                               double* __restrict__ grad, double* __restrict__ hdiag,
                                                               const int* __restrict__ perm, int grad_only) {
  __shared__ double sred[4];
  const int i = blockIdx.x;
  if (grad_only && i < 21) return;
  double v = 0.0;
  for (int b = threadIdx.x; b < n_part; b += 256) v += cb.part[(size_t)b * kCalibPartStride + i];
  const double tot = block_sum_256(v, sred);
  if (threadIdx.x != 0) return;
  if (i < 21) {
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= i) ++a;
    const int c = i - a * (a + 1) / 2;
    const int ra = calib_col(cb, a), rc = calib_col(cb, c);
    if (ra < 0 || rc < 0) return;
    const int sa = perm[ra], sc = perm[rc];
    atomicAdd(&S[(size_t)sa * ld + sc], tot);
    if (a != c) atomicAdd(&S[(size_t)sc * ld + sa], tot);
  } else {
    const int c = (i - 21) % 6, which = (i - 21) / 6;
    const int rc = calib_col(cb, c);
    if (rc < 0) return;
    if (which == 0) atomicAdd(&S[(size_t)rhs_row * ld + perm[rc]], tot);
    else if (which == 1) atomicAdd(&grad[rc], tot);
    else atomicAdd(&hdiag[rc], tot);
  }
}

// One wave per segment: up to 256 factors seen from one camera pose i; S(i,e) += sum A_f^T E~_f (6x6), both triangles of S.
// Algorithmic bytes per factor: 4 (index) + 96 (pose part of J) + 96 (E~) = 196.
__global__ __launch_bounds__(64) void calib_pose_kernel(Calib cb, const double* __restrict__ J, const int* __restrict__ cp_tq,
                                                        const int* __restrict__ cp_tp, double* __restrict__ S, int ld,
                                                        const int* __restrict__ perm) {
  const int seg = blockIdx.x;
  if (seg >= cb.n_seg) return;
  const int lane = threadIdx.x;
  const int cp = cb.seg_cp[seg], beg = cb.seg_start[seg], end = cb.seg_start[seg + 1];
  double v[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) v[i] = 0.0;
  for (int i = beg + lane; i < end; i += 64) {
    const int f = cb.seg_fac[i];
    double A[12], Et[12];
    calib_load_row12(J + (size_t)f * kJAStride, A);
    calib_load_row12(cb.Et + (size_t)f * 12, Et);
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = 0; c < 6; ++c) v[a * 6 + c] += A[a] * Et[c] + A[6 + a] * Et[6 + c];
  }
  wave_sum_transpose64(v);
  const double total = v[0];
  if (lane >= 36) return;
  const int a = lane / 6, c = lane % 6;
  const int tq = cp_tq[cp], tp = cp_tp[cp];
  const int row = (a < 3) ? (tq < 0 ? -1 : tq + a) : (tp < 0 ? -1 : tp + a - 3);
  const int col = calib_col(cb, c);
  if (row < 0 || col < 0) return;
  const int sr = perm[row], sc = perm[col];
  atomicAdd(&S[(size_t)sr * ld + sc], total);
  atomicAdd(&S[(size_t)sc * ld + sr], total);
}

int calib_border_blocks(const Visual& v) { return (v.n_lm * 8 + 255) / 256 + (v.n - v.n_elim + 255) / 256; }
void launch_calib_border(hipStream_t s, const Visual& v, const Calib& cb, double* S, int ld, int rhs_row, double* grad, double* hdiag, const int* perm,
                         bool grad_only) {
  if (!cb.on || v.n <= 0) return;
  const int lm_blocks = (v.n_lm * 8 + 255) / 256, tail_blocks = (v.n - v.n_elim + 255) / 256;
  if (lm_blocks + tail_blocks > 0) {   // (= calib_border_blocks(v): the rows of cb.part)
    hipLaunchKernelGGL(calib_border_kernel, dim3(lm_blocks + tail_blocks), dim3(256), 0, s, cb, v.n_lm, lm_blocks, v.n_elim, v.n, v.lm_start, v.r, v.CR);
    hipLaunchKernelGGL(calib_border_sum_kernel, dim3(kCalibSums), dim3(256), 0, s, cb, lm_blocks + tail_blocks, S, ld, rhs_row, grad, hdiag, perm,
                       grad_only ? 1 : 0);
  }
  // (gradient only — the end of a solve: no factorisation follows, the S(i,e) blocks are not wanted, as launch_pairs skips its own)
  if (cb.n_seg > 0 && !grad_only) hipLaunchKernelGGL(calib_pose_kernel, dim3(cb.n_seg), dim3(64), 0, s, cb, v.J, v.cp_tq, v.cp_tp, S, ld, perm);
}

// ---------------------------------------------------------------------------------------------------
// backsub_mcc_kernel's landmark and constant-landmark workgroups (k_reproj.hip) with J delta = -(A y_cam + E y_e + B y_l): the landmark
// step gains -L^-T G_l y_e through sum_f C_f^T (A_f y_cam + E_f y_e), the model cost change its E_f y_e term.  Full layout of J, C rows
// kept; the same workgroup-per-partial layout of mcc_part, so the step's reduction adds the same array in the same order.
// ---------------------------------------------------------------------------------------------------
BSG_DEV void calib_pose_ext_part(const double* __restrict__ Jf_row, const double* __restrict__ Ef_row, int tq, int tp, const Calib& cb,
                                 const double* __restrict__ y_pose, const double (&ye)[6], double& j0, double& j1) {
  double A[12], E[12];
  calib_load_row12(Jf_row, A);
  calib_load_row12(Ef_row, E);
  j0 = 0.0; j1 = 0.0;
  if (tq >= 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double yv = y_pose[tq + k]; j0 += A[k] * yv; j1 += A[6 + k] * yv; }
  }
  if (tp >= 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double yv = y_pose[tp + k]; j0 += A[3 + k] * yv; j1 += A[9 + k] * yv; }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) { j0 += E[k] * ye[k]; j1 += E[6 + k] * ye[k]; }
}
__global__ __launch_bounds__(256) void calib_backsub_mcc_kernel(Calib cb, int n_lm, int n_lm_groups, int n_elim, int n, const int* __restrict__ lm_start,
                                                                const double* __restrict__ J, const double* __restrict__ JB,
                                                                const double2* __restrict__ r, const double* __restrict__ CR,
                                                                const int* __restrict__ cam_pose, const int* __restrict__ cp_tq,
                                                                const int* __restrict__ cp_tp, const double* __restrict__ Linv,
                                                                const double* __restrict__ z, int n_pose, const double* __restrict__ y_pose,
                                                                double* __restrict__ delta, double* __restrict__ mcc_part) {
  __shared__ double sred[4];
  double ye[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) { const int t = calib_col(cb, k); ye[k] = t >= 0 ? y_pose[t] : 0.0; }
  double acc = 0.0;
  const int bx = blockIdx.x;
  if (bx < n_lm_groups) {
    const int gid = bx * 256 + threadIdx.x;
    const int l = gid >> 3, sub = gid & 7;
    const bool valid = l < n_lm;
    int beg = 0, end = 0;
    if (valid) { beg = lm_start[l]; end = lm_start[l + 1]; }
    const int lc = valid ? l : 0;
    const double* Li = Linv + (size_t)lc * kLmRec;
    const double Li0 = Li[0], Li1 = Li[1], Li2 = Li[2], Li3 = Li[3], Li4 = Li[4], Li5 = Li[5];
    const double* zl = z + (size_t)lc * kLmRec;
    const double zl0 = zl[0], zl1 = zl[1], zl2 = zl[2];
    double a0 = 0, a1 = 0, a2 = 0;
    for (int f = beg + sub; f < end; f += 8) {
      const double2* C2 = reinterpret_cast<const double2*>(CR + (size_t)f * 8);
      const double2 ca = C2[0], cb2 = C2[1], cc = C2[2];
      const double C[6] = {ca.x, ca.y, cb2.x, cb2.y, cc.x, cc.y};
      const int cp = cam_pose[f];
      double j0, j1;
      calib_pose_ext_part(J + (size_t)f * kJAStride, cb.E + (size_t)f * 12, cp_tq[cp], cp_tp[cp], cb, y_pose, ye, j0, j1);
      a0 += C[0] * j0 + C[3] * j1; a1 += C[1] * j0 + C[4] * j1; a2 += C[2] * j0 + C[5] * j1;
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) { a0 += __shfl_xor(a0, o, 8); a1 += __shfl_xor(a1, o, 8); a2 += __shfl_xor(a2, o, 8); }
    if (valid) {
      const double w0 = zl0 - a0, w1 = zl1 - a1, w2 = zl2 - a2;
      const double y0 = Li0 * w0 + Li1 * w1 + Li3 * w2;
      const double y1 = Li2 * w1 + Li4 * w2;
      const double y2 = Li5 * w2;
      if (sub == 0) {
        const int to = n_pose + 3 * l;
        delta[to] = -y0; delta[to + 1] = -y1; delta[to + 2] = -y2;
      }
      for (int f = beg + sub; f < end; f += 8) {
        const double2* B2 = reinterpret_cast<const double2*>(JB + (size_t)f * 6);
        const double2 ba = B2[0], bb = B2[1], bc = B2[2];
        const double Bf[6] = {ba.x, ba.y, bb.x, bb.y, bc.x, bc.y};
        const int cp = cam_pose[f];
        double j0, j1;
        calib_pose_ext_part(J + (size_t)f * kJAStride, cb.E + (size_t)f * 12, cp_tq[cp], cp_tp[cp], cb, y_pose, ye, j0, j1);
        const double d0 = -(j0 + Bf[0] * y0 + Bf[1] * y1 + Bf[2] * y2), d1 = -(j1 + Bf[3] * y0 + Bf[4] * y1 + Bf[5] * y2);
        const double2 rf = r[f];
        acc -= d0 * (rf.x + 0.5 * d0) + d1 * (rf.y + 0.5 * d1);
      }
    }
  } else {
    const int f = n_elim + (bx - n_lm_groups) * 256 + (int)threadIdx.x;
    if (f < n) {
      const int cp = cam_pose[f];
      double j0, j1;
      calib_pose_ext_part(J + (size_t)f * kJAStride, cb.E + (size_t)f * 12, cp_tq[cp], cp_tp[cp], cb, y_pose, ye, j0, j1);
      const double2 rf = r[f];
      acc = -((-j0) * (rf.x - 0.5 * j0) + (-j1) * (rf.y - 0.5 * j1));
    }
  }
  const double tot = block_sum_256(acc, sred);
  if (threadIdx.x == 0) mcc_part[bx] = tot;
}
void launch_calib_backsub_mcc(hipStream_t s, const Visual& v, const Calib& cb, int n_pose, const double* y_pose, double* delta, double* mcc_part) {
  const int g_lm = (v.n_lm * 8 + 255) / 256, grid = g_lm + (v.n - v.n_elim + 255) / 256;   // (= backsub_mcc_groups(v): the partials the reduction sums)
  if (!cb.on || grid == 0) return;
  hipLaunchKernelGGL(calib_backsub_mcc_kernel, dim3(grid), dim3(256), 0, s, cb, v.n_lm, g_lm, v.n_elim, v.n, v.lm_start, v.J, v.JB, v.r, v.CR, v.cam_pose,
                     v.cp_tq, v.cp_tp, v.Linv, v.z, n_pose, y_pose, delta, mcc_part);
}

}  // namespace bsg
