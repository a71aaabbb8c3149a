// The front-end entry points of the C-ABI (include/bsgpu.h): bsgpu_preintegrate, bsgpu_inertial_alignment, bsgpu_register_scans,
// bsgpu_register_scans_gicp, bsgpu_register_scans_loam, bsgpu_extract_loam_features, bsgpu_build_registration_maps, bsgpu_scan_context_describe, bsgpu_scan_context_match, bsgpu_triangulate, bsgpu_localize_frames and the three RANSACs.  Each checks its arguments, describes its arrays as a StageLayout (staging.h:
// [inputs | outputs | scratch] in one device allocation), runs its kernels between one copy in and one copy out, and hands the
// results to the caller's arrays: nothing is written to them unless the call succeeds.
#include <algorithm>
#include <cmath>
#include <string>

#include "bsgpu_ctx.h"
#include "gicp.h"
#include "icp.h"
#include "point_grid.h"
#include "inertial_align.h"
#include "loam.h"
#include "loam_features.h"
#include "registration_map.h"
#include "scan_context.h"
#include "staging.h"

using namespace bsg;

namespace {
thread_local std::string g_register_scans_error;   // what this thread's last failed bsgpu_register_scans objected to (it has no context to keep it)
thread_local std::string g_scan_context_error;     // the same for bsgpu_scan_context_describe and bsgpu_scan_context_match

// ---- what bsgpu_register_scans and bsgpu_register_scans_gicp share: a table of scan pairs, the grids of its clouds, its chunks ----------
const double kEye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
int refuse_scans(int code, const char* prefix, const std::string& why) { g_register_scans_error = std::string(prefix) + ": " + why; return code; }

// The pair table of a call: the two start tables, in check_start_table's order, an item bad when one of its points is not finite (a
// NaN would choose a grid cell); init (12 per pair) <- T_init, the identity without one, which must be finite.  BSGPU_OK, or the
// refusal with its message under the caller's prefix.  names (optional): what the messages call the two tables and the two clouds.
int check_pair_table(const char* prefix, int n_pairs, const int32_t* ref_start, const double* ref_points, const int32_t* tgt_start,
                     const double* tgt_points, const double* T_init, double* init, const char* const* names = nullptr) {
  static const char* const plain[4] = {"ref_start", "reference", "tgt_start", "target"};
  if (!names) names = plain;
  const struct { const int32_t* start; const double* pts; const char *table, *cloud; } sides[2] = {{ref_start, ref_points, names[0], names[1]},
                                                                                                    {tgt_start, tgt_points, names[2], names[3]}};
  for (const auto& side : sides) {
    const int32_t* start = side.start;
    const double* pts = side.pts;
    const auto finite_item = [start, pts](int k) {
      if (start[k + 1] > start[k] && !pts) return false;
      for (size_t i = 3 * (size_t)start[k]; i < 3 * (size_t)start[k + 1]; ++i) if (!std::isfinite(pts[i])) return false;
      return true;
    };
    switch (check_start_table(start, n_pairs, INT_MAX, finite_item)) {
      case kStartNotZero: return refuse_scans(BSGPU_ERR_INVALID, prefix, std::string(side.table) + "[0] must be 0");
      case kStartDecreasing: return refuse_scans(BSGPU_ERR_INVALID, prefix, std::string(side.table) + " must be non-decreasing");
      case kStartBadItem: return refuse_scans(BSGPU_ERR_INVALID, prefix, std::string("null or non-finite ") + side.cloud + " points");
      default: break;
    }
  }
  for (size_t i = 0; i < 12 * (size_t)n_pairs; ++i) {
    init[i] = T_init ? T_init[i] : kEye[i % 12];
    if (!std::isfinite(init[i])) return refuse_scans(BSGPU_ERR_INVALID, prefix, "non-finite T_init");
  }
  return BSGPU_OK;
}

// The grids of n_clouds clouds, cloud c under the transform T + 12 c, with cell edge h: the bounding box of every cloud in the frame it
// is searched in, by the arithmetic the device will use (point_grid.h); the clouds' cells follow one another in the call's cell array.
// A grid may have BSGPU_ICP_MAX_CELLS cells, the call 16 times as many.  `one`: what the caller's messages call a cloud.
struct GridsPlan {
  std::vector<PointGrid> grids;
  double cells = 0.0;          // of all grids
  int n_tiles = 0;             // the cell array in scan tiles
  int max_points = 0;          // the largest cloud
};
int plan_grids(const char* prefix, const char* one, size_t n_clouds, const int32_t* start, const double* pts, const double* T, double h, GridsPlan* out) {
  out->grids.resize(n_clouds);
  for (size_t c = 0; c < n_clouds; ++c) {
    const int n = start[c + 1] - start[c];
    double here;
    out->max_points = std::max(out->max_points, n);
    switch (grid_plan(n, pts + 3 * (size_t)start[c], T + 12 * c, h, (int)out->cells, (double)BSGPU_ICP_MAX_CELLS, &out->grids[c], &here)) {
      case kGridNotFinite: return refuse_scans(BSGPU_ERR_INVALID, prefix, "T_init takes a target point out of range");
      case kGridTooManyCells: return refuse_scans(BSGPU_ERR_UNSUPPORTED, prefix, std::string("a ") + one + "'s grid exceeds BSGPU_ICP_MAX_CELLS cells");
      default: break;
    }
    out->cells += here;
    if (out->cells > 16.0 * BSGPU_ICP_MAX_CELLS) return refuse_scans(BSGPU_ERR_UNSUPPORTED, prefix, "the call's grids exceed 16 x BSGPU_ICP_MAX_CELLS cells");
  }
  out->n_tiles = (int)(((size_t)out->cells + kGridScanTile - 1) / kGridScanTile);
  return BSGPU_OK;
}

// chunk_start (n_pairs + 1): a pair's partial records, one per kGridChunk source points; returns the most chunks of one pair
int plan_chunks(size_t n_pairs, const int32_t* ref_start, std::vector<int32_t>* chunk_start) {
  int max_chunks = 0;
  chunk_start->assign(n_pairs + 1, 0);
  for (size_t p = 0; p < n_pairs; ++p) {
    const int chunks = (ref_start[p + 1] - ref_start[p] + kGridChunk - 1) / kGridChunk;
    (*chunk_start)[p + 1] = (*chunk_start)[p] + chunks;
    max_chunks = std::max(max_chunks, chunks);
  }
  return max_chunks;
}
}

extern "C" {

int bsgpu_preintegrate(int device, int32_t n, const int32_t* sample_start, const double* t, const double* w, const double* a,
                       const double* t_end, const double* bg, const double* ba, const double* cov_w, const double* cov_a,
                       const double* cov_bg, const double* cov_ba, double info_weight, double* consts_out) try {
  if (n < 0) return BSGPU_ERR_INVALID;
  if (n == 0) return BSGPU_OK;
  if (!sample_start || !t_end || !bg || !ba || !cov_w || !cov_a || !cov_bg || !cov_ba || !consts_out) return BSGPU_ERR_INVALID;
  // an interval may hold no samples (it stays the identity); the kernel indexes the samples by this table, so it is checked here
  // (it may start above 0, so it is not check_start_table's)
  if (sample_start[0] < 0) return BSGPU_ERR_INVALID;
  for (int i = 0; i < n; ++i) if (sample_start[i + 1] < sample_start[i]) return BSGPU_ERR_INVALID;
  const size_t ns = (size_t)sample_start[n], ni = (size_t)n;
  if (ns > 0 && (!t || !w || !a)) return BSGPU_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return BSGPU_ERR_DEVICE;
  double covs[36];
  std::memcpy(&covs[0], cov_w, 72); std::memcpy(&covs[9], cov_a, 72); std::memcpy(&covs[18], cov_bg, 72); std::memcpy(&covs[27], cov_ba, 72);
  StageLayout L;
  const int s_ss = L.in(sample_start, 4 * (ni + 1)), s_t = L.in(t, 8 * ns), s_w = L.in(w, 24 * ns), s_a = L.in(a, 24 * ns), s_te = L.in(t_end, 8 * ni),
            s_bg = L.in(bg, 24 * ni), s_ba = L.in(ba, 24 * ni), s_cov = L.in(covs, sizeof(covs)), s_out = L.out(consts_out, 8 * 287 * ni);
  DeviceStage D(L);
  if (!D) return BSGPU_ERR_DEVICE;
  const hipError_t e = D.run(nullptr, [&] {
    launch_preintegrate(nullptr, n, D.ptr<int>(s_ss), D.ptr<double>(s_t), D.ptr<double>(s_w), D.ptr<double>(s_a), D.ptr<double>(s_te),
                        D.ptr<double>(s_bg), D.ptr<double>(s_ba), D.ptr<double>(s_cov), info_weight, D.ptr<double>(s_out));
  });
  if (e != hipSuccess) { (void)hipGetLastError(); return BSGPU_ERR_DEVICE; }
  L.scatter();
  return BSGPU_OK;
} catch (...) { return api_exception(nullptr); }

int bsgpu_inertial_alignment(int device, int32_t n_paths, const int32_t* frame_start, const double* t_frame, const double* q_frame,
                             const double* p_frame, const int32_t* imu_range, const double* t, const double* w, const double* a,
                             int32_t bridge_gap, double min_excitation, int32_t apply_scale, double scale_min, double scale_max,
                             double rank_tol, double* gravity, double* bg, double* scale, double* excitation, int32_t* gyro_rank,
                             double* velocity, double* q_out, double* p_out, double* v_out, int32_t* status) try {
  if (n_paths < 0) return BSGPU_ERR_INVALID;
  if (n_paths == 0) return BSGPU_OK;
  if (!frame_start || !imu_range || !gravity || !bg || !scale || !excitation || !gyro_rank || !status) return BSGPU_ERR_INVALID;
  size_t ns = 0;
  const auto range_ok = [&](int k) {
    if (imu_range[2 * k] < 0 || imu_range[2 * k + 1] < imu_range[2 * k]) return false;
    ns = std::max(ns, (size_t)imu_range[2 * k + 1]);
    return true;
  };
  if (check_start_table(frame_start, n_paths, INT_MAX, range_ok) != kStartOk) return BSGPU_ERR_INVALID;
  const size_t nf = (size_t)frame_start[n_paths], np = (size_t)n_paths;
  if (nf > 0 && (!t_frame || !q_frame || !p_frame || !velocity || !q_out || !p_out || !v_out)) return BSGPU_ERR_INVALID;
  if (ns > 0 && (!t || !w || !a)) return BSGPU_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return BSGPU_ERR_DEVICE; }
  StageLayout L;
  const int s_fs = L.in(frame_start, 4 * (np + 1)), s_rng = L.in(imu_range, 8 * np), s_tf = L.in(t_frame, 8 * nf), s_qf = L.in(q_frame, 32 * nf),
            s_pf = L.in(p_frame, 24 * nf), s_t = L.in(t, 8 * ns), s_w = L.in(w, 24 * ns), s_a = L.in(a, 24 * ns);
  const int s_g = L.out(gravity, 24 * np), s_bg = L.out(bg, 24 * np), s_sc = L.out(scale, 8 * np), s_ex = L.out(excitation, 8 * np),
            s_rk = L.out(gyro_rank, 4 * np), s_st = L.out(status, 4 * np), s_vel = L.out(velocity, 24 * nf), s_qo = L.out(q_out, 32 * nf),
            s_po = L.out(p_out, 24 * nf), s_vo = L.out(v_out, 24 * nf);
  // the kernel's own working arrays (uninitialised): frame owners, per-frame and per-path doubles
  const int s_own = L.scratch(4 * (nf + np)), s_fsc = L.scratch(8 * nf * kAlignFrameScratch), s_psc = L.scratch(8 * np * kAlignPathScratch);
  DeviceStage D(L, 256);
  if (!D) return BSGPU_ERR_DEVICE;
  const auto F = [&](int s) { return D.ptr<double>(s); };
  const auto I = [&](int s) { return D.ptr<int>(s); };
  const hipError_t e = D.run(nullptr, [&] {
    launch_inertial_alignment(nullptr, n_paths, I(s_fs), F(s_tf), F(s_qf), F(s_pf), I(s_rng), F(s_t), F(s_w), F(s_a), bridge_gap, min_excitation,
                              apply_scale, scale_min, scale_max, rank_tol, F(s_g), F(s_bg), F(s_sc), F(s_ex), I(s_rk), F(s_vel), F(s_qo), F(s_po),
                              F(s_vo), I(s_st), I(s_own), F(s_fsc), F(s_psc));
  });
  if (e != hipSuccess) { (void)hipGetLastError(); return BSGPU_ERR_DEVICE; }
  L.scatter();
  return BSGPU_OK;
} catch (...) { return api_exception(nullptr); }

const char* bsgpu_register_scans_error(void) { return g_register_scans_error.c_str(); }

int bsgpu_register_scans(int device, int32_t n_pairs, const int32_t* ref_start, const double* ref_points, const int32_t* tgt_start,
                         const double* tgt_points, const double* T_init, double max_corr, int32_t max_iter, double t_eps, double fit_eps,
                         double rotation_threshold, double rel_mse_eps, double* T_refest_ref, double* T_ref_tgt, double* mse,
                         int32_t* n_corr, int32_t* n_iters, int32_t* status) try {
  const auto refuse = [](int code, const char* why) { g_register_scans_error = why; return code; };
  if (n_pairs < 0 || !ref_start || !tgt_start || !T_refest_ref || !status) return refuse(BSGPU_ERR_INVALID, "register_scans: null argument");
  if (!(max_corr > 0.0) || !std::isfinite(max_corr)) return refuse(BSGPU_ERR_INVALID, "register_scans: max_corr must be positive and finite");
  if (max_iter < 1) return refuse(BSGPU_ERR_INVALID, "register_scans: max_iter must be at least 1");
  if (!(t_eps >= 0.0) || !(fit_eps >= 0.0) || !(rel_mse_eps >= 0.0) || rotation_threshold != rotation_threshold)
    return refuse(BSGPU_ERR_INVALID, "register_scans: t_eps, fit_eps and rel_mse_eps must not be negative, no tolerance NaN");
  if (max_iter > BSGPU_ICP_MAX_ITER) return refuse(BSGPU_ERR_UNSUPPORTED, "register_scans: max_iter exceeds BSGPU_ICP_MAX_ITER");
  const size_t np = (size_t)n_pairs;
  std::vector<double> init(12 * np);
  if (const int rc = check_pair_table("register_scans", n_pairs, ref_start, ref_points, tgt_start, tgt_points, T_init, init.data())) return rc;
  // the grids of the targets under their T_init, cell edge max_corr
  GridsPlan G;
  if (const int rc = plan_grids("register_scans", "pair", np, tgt_start, tgt_points, init.data(), max_corr, &G)) return rc;
  std::vector<int32_t> chunk_start;
  const int max_chunks = plan_chunks(np, ref_start, &chunk_start);
  if (n_pairs == 0) return BSGPU_OK;
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "register_scans: hipSetDevice failed"); }
  const size_t n_ref = (size_t)ref_start[n_pairs], n_tgt = (size_t)tgt_start[n_pairs], n_chunks = (size_t)chunk_start[n_pairs];
  StageLayout L;
  const int s_rs = L.in(ref_start, 4 * (np + 1)), s_ref = L.in(ref_points, 24 * n_ref), s_ts = L.in(tgt_start, 4 * (np + 1)),
            s_tgt = L.in(tgt_points, 24 * n_tgt), s_ti = L.in(init.data(), 96 * np), s_cs = L.in(chunk_start.data(), 4 * (np + 1)),
            s_gr = L.in(G.grids.data(), sizeof(PointGrid) * np);
  const int s_T = L.out(T_refest_ref, 96 * np), s_Trt = L.out(T_ref_tgt, 96 * np), s_mse = L.out(mse, 8 * np), s_nc = L.out(n_corr, 4 * np),
            s_ni = L.out(n_iters, 4 * np), s_st = L.out(status, 4 * np);
  // the kernels' working arrays (uninitialised: the launch clears the cells, icp_init_kernel sets the per-pair words): the transformed targets and their
  // cells, the grids' cells and their tile sums, the sorted records, the partial records, mse_prev and the done words
  const int s_tq = L.scratch(24 * n_tgt), s_tc = L.scratch(4 * n_tgt), s_cells = L.scratch(4 * (size_t)G.n_tiles * kGridScanTile),
            s_tile = L.scratch(4 * (size_t)G.n_tiles), s_rec = L.scratch(32 * n_tgt), s_part = L.scratch(8 * kIcpRec * n_chunks),
            s_prev = L.scratch(8 * np), s_done = L.scratch(4 * np);
  DeviceStage D(L);
  if (!D) return refuse(BSGPU_ERR_DEVICE, "register_scans: out of device memory");
  const IcpParams P{max_iter, t_eps, fit_eps, rotation_threshold, rel_mse_eps};
  const auto F = [&](int s) { return D.ptr<double>(s); };
  const auto I = [&](int s) { return D.ptr<int>(s); };
  const hipError_t e = D.run(nullptr, [&] {
    launch_register_scans(nullptr, n_pairs, G.max_points, (int)n_tgt, max_chunks, G.n_tiles, I(s_rs), F(s_ref), I(s_ts), F(s_tgt), F(s_ti), I(s_cs),
                          D.ptr<PointGrid>(s_gr), max_corr, P, F(s_T), F(s_Trt), F(s_mse), I(s_nc), I(s_ni), I(s_st), F(s_tq), I(s_tc), I(s_cells),
                          I(s_tile), F(s_rec), F(s_part), F(s_prev), I(s_done));
  });
  if (e != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "register_scans: device error"); }
  L.scatter();
  return BSGPU_OK;
} catch (...) {
  try { g_register_scans_error = "register_scans: out of host memory"; } catch (...) {}
  return api_exception(nullptr);
}

int bsgpu_register_scans_gicp(int device, int32_t n_pairs, const int32_t* ref_start, const double* ref_points, const int32_t* tgt_start,
                              const double* tgt_points, const double* T_init, int32_t k_neighbors, double gicp_epsilon, double max_corr,
                              int32_t max_iter, double r_eps, double t_eps, int32_t max_inner, double inner_eps, double grid_cell,
                              double* T_refest_ref, double* T_ref_tgt, double* cost, int32_t* n_corr, int32_t* n_iters, int32_t* n_inner,
                              int32_t* status, double* ref_cov, double* tgt_cov) try {
  const auto refuse = [](int code, const char* why) { g_register_scans_error = why; return code; };
  if (n_pairs < 0 || !ref_start || !tgt_start || !T_refest_ref || !status) return refuse(BSGPU_ERR_INVALID, "register_scans_gicp: null argument");
  if (k_neighbors < 1) return refuse(BSGPU_ERR_INVALID, "register_scans_gicp: k_neighbors must be at least 1");
  if (!(gicp_epsilon > 0.0) || !(gicp_epsilon <= 1.0)) return refuse(BSGPU_ERR_INVALID, "register_scans_gicp: gicp_epsilon must lie in (0, 1]");
  if (!(max_corr > 0.0) || !std::isfinite(max_corr)) return refuse(BSGPU_ERR_INVALID, "register_scans_gicp: max_corr must be positive and finite");
  if (!(grid_cell > 0.0) || !std::isfinite(grid_cell)) return refuse(BSGPU_ERR_INVALID, "register_scans_gicp: grid_cell must be positive and finite");
  if (max_iter < 1) return refuse(BSGPU_ERR_INVALID, "register_scans_gicp: max_iter must be at least 1");
  if (max_inner < 1) return refuse(BSGPU_ERR_INVALID, "register_scans_gicp: max_inner must be at least 1");
  if (!(r_eps >= 0.0) || !(t_eps >= 0.0) || !(inner_eps >= 0.0))
    return refuse(BSGPU_ERR_INVALID, "register_scans_gicp: r_eps, t_eps and inner_eps must not be negative or NaN");
  if (k_neighbors > BSGPU_GICP_MAX_K) return refuse(BSGPU_ERR_UNSUPPORTED, "register_scans_gicp: k_neighbors exceeds BSGPU_GICP_MAX_K");
  if (max_iter > BSGPU_ICP_MAX_ITER) return refuse(BSGPU_ERR_UNSUPPORTED, "register_scans_gicp: max_iter exceeds BSGPU_ICP_MAX_ITER");
  if (max_inner > BSGPU_GICP_MAX_INNER) return refuse(BSGPU_ERR_UNSUPPORTED, "register_scans_gicp: max_inner exceeds BSGPU_GICP_MAX_INNER");
  static_assert(BSGPU_GICP_MAX_K == kGicpMaxK && BSGPU_GICP_MAX_INNER == kGicpMaxInner, "the header's caps are gicp.h's");
  const size_t np = (size_t)n_pairs;
  std::vector<double> T_cloud(24 * np);
  if (const int rc = check_pair_table("register_scans_gicp", n_pairs, ref_start, ref_points, tgt_start, tgt_points, T_init, T_cloud.data())) return rc;
  const size_t n_ref = (size_t)ref_start[n_pairs], n_tgt = (size_t)tgt_start[n_pairs], n_pts = n_ref + n_tgt;
  if (n_pts > (size_t)INT_MAX) return refuse(BSGPU_ERR_UNSUPPORTED, "register_scans_gicp: more than 2^31 - 1 points in one call");
  // the call's clouds as one packed array: the targets of all pairs, then the sources; a source's transform is the identity
  std::vector<double> pts(3 * n_pts);
  std::vector<int32_t> cloud_start(2 * np + 1, 0);
  for (size_t i = 0; i < 12 * np; ++i) T_cloud[12 * np + i] = kEye[i % 12];
  if (n_tgt) std::memcpy(pts.data(), tgt_points, 24 * n_tgt);
  if (n_ref) std::memcpy(pts.data() + 3 * n_tgt, ref_points, 24 * n_ref);
  int n_live = 0;
  for (size_t p = 0; p < np; ++p) {
    cloud_start[p + 1] = tgt_start[p + 1];
    cloud_start[np + p + 1] = (int32_t)n_tgt + ref_start[p + 1];
    n_live += ref_start[p + 1] - ref_start[p] >= k_neighbors && tgt_start[p + 1] - tgt_start[p] >= k_neighbors ? 1 : 0;
  }
  // the grids of every cloud in the frame it is searched in, cell edge grid_cell
  GridsPlan G;
  if (const int rc = plan_grids("register_scans_gicp", "cloud", 2 * np, cloud_start.data(), pts.data(), T_cloud.data(), grid_cell, &G)) return rc;
  std::vector<int32_t> chunk_start;
  const int max_chunks = plan_chunks(np, ref_start, &chunk_start);
  if (n_pairs == 0) return BSGPU_OK;
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "register_scans_gicp: hipSetDevice failed"); }
  const size_t n_chunks = (size_t)chunk_start[n_pairs];
  StageLayout L;
  const int s_cs = L.in(cloud_start.data(), 4 * (2 * np + 1)), s_pts = L.in(pts.data(), 24 * n_pts), s_tc = L.in(T_cloud.data(), 192 * np),
            s_ch = L.in(chunk_start.data(), 4 * (np + 1)), s_gr = L.in(G.grids.data(), sizeof(PointGrid) * 2 * np);
  const int s_T = L.out(T_refest_ref, 96 * np), s_Trt = L.out(T_ref_tgt, 96 * np), s_cost = L.out(cost, 8 * np), s_nc = L.out(n_corr, 4 * np),
            s_ni = L.out(n_iters, 4 * np), s_nn = L.out(n_inner, 4 * np), s_st = L.out(status, 4 * np),
            s_cov = L.out(nullptr, ref_cov || tgt_cov ? 48 * n_pts : 0);
  // the kernels' working arrays (uninitialised): the grid build's, the covariances when nobody asked for them, the pairs' states and
  // done words, j(i) and M_i per point, the chunks' kept counts and partial records
  const int s_tq = L.scratch(24 * n_pts), s_cell = L.scratch(4 * n_pts), s_cells = L.scratch(4 * (size_t)G.n_tiles * kGridScanTile),
            s_tile = L.scratch(4 * (size_t)G.n_tiles), s_rec = L.scratch(32 * n_pts), s_cov2 = L.scratch(ref_cov || tgt_cov ? 0 : 48 * n_pts),
            s_state = L.scratch(sizeof(GicpState) * np), s_done = L.scratch(4 * np), s_corr = L.scratch(4 * n_pts), s_M = L.scratch(48 * n_pts), s_kept = L.scratch(4 * n_chunks),
            s_part = L.scratch(8 * kGicpRec * n_chunks);
  DeviceStage D(L);
  if (!D) return refuse(BSGPU_ERR_DEVICE, "register_scans_gicp: out of device memory");
  const GicpParams P{k_neighbors, gicp_epsilon, max_corr, max_iter, r_eps, t_eps, max_inner, inner_eps};
  const auto F = [&](int s) { return D.ptr<double>(s); };
  const auto I = [&](int s) { return D.ptr<int>(s); };
  hipError_t le = hipSuccess;
  const hipError_t e = D.run(nullptr, [&] {
    le = launch_register_scans_gicp(nullptr, n_pairs, n_live, G.max_points, (int)n_pts, max_chunks, G.n_tiles, I(s_cs), F(s_pts), F(s_tc), I(s_ch),
                                    D.ptr<PointGrid>(s_gr), P, F(s_T), F(s_Trt), F(s_cost), I(s_nc), I(s_ni), I(s_nn), I(s_st),
                                    F(ref_cov || tgt_cov ? s_cov : s_cov2), F(s_tq), I(s_cell), I(s_cells), I(s_tile), F(s_rec),
                                    D.ptr<GicpState>(s_state), I(s_done), I(s_corr), F(s_M), I(s_kept), F(s_part));
  });
  if (e != hipSuccess || le != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "register_scans_gicp: device error"); }
  L.scatter();
  if (ref_cov || tgt_cov) {
    const double* cov = L.out_image<double>(s_cov);
    if (tgt_cov && n_tgt) std::memcpy(tgt_cov, cov, 48 * n_tgt);
    if (ref_cov && n_ref) std::memcpy(ref_cov, cov + 6 * n_tgt, 48 * n_ref);
  }
  return BSGPU_OK;
} catch (...) {
  try { g_register_scans_error = "register_scans_gicp: out of host memory"; } catch (...) {}
  return api_exception(nullptr);
}

int bsgpu_register_scans_loam(int device, int32_t n_pairs, const int32_t* ref_edge_start, const double* ref_edges, const int32_t* ref_surf_start,
                              const double* ref_surfs, const int32_t* tgt_edge_start, const double* tgt_edges, const int32_t* tgt_surf_start,
                              const double* tgt_surfs, const double* T_init, double max_corr, int32_t min_measurements, int32_t max_outer,
                              double conv_translation_m, double conv_rotation_deg, const bsgpu_options* inner, int32_t loss_kind, double loss_a,
                              double grid_cell, double* T_refest_ref, double* T_ref_tgt, double* cov, double* cost, int32_t* n_edge,
                              int32_t* n_surf, int32_t* n_iters, int32_t* n_inner, int32_t* status) try {
  const char* const me = "register_scans_loam";
  const auto refuse = [me](int code, const char* why) { return refuse_scans(code, me, why); };
  if (n_pairs < 0 || !ref_edge_start || !ref_surf_start || !tgt_edge_start || !tgt_surf_start || !inner || !T_refest_ref || !status)
    return refuse(BSGPU_ERR_INVALID, "null argument");
  if (!(max_corr > 0.0) || !std::isfinite(max_corr)) return refuse(BSGPU_ERR_INVALID, "max_corr must be positive and finite");
  if (!(grid_cell > 0.0) || !std::isfinite(grid_cell)) return refuse(BSGPU_ERR_INVALID, "grid_cell must be positive and finite");
  if (min_measurements < 1) return refuse(BSGPU_ERR_INVALID, "min_measurements must be at least 1");
  if (max_outer < 1) return refuse(BSGPU_ERR_INVALID, "max_outer must be at least 1");
  if (!(conv_translation_m >= 0.0) || !(conv_rotation_deg >= 0.0))
    return refuse(BSGPU_ERR_INVALID, "conv_translation_m and conv_rotation_deg must not be negative or NaN");
  if (!(conv_rotation_deg < 180.0)) return refuse(BSGPU_ERR_INVALID, "conv_rotation_deg must be below 180");
  if (loss_kind < BSGPU_LOSS_TRIVIAL || loss_kind > BSGPU_LOSS_HUBER) return refuse(BSGPU_ERR_INVALID, "unknown loss kind");
  if (loss_kind == BSGPU_LOSS_HUBER && (!(loss_a > 0.0) || !std::isfinite(loss_a)))
    return refuse(BSGPU_ERR_INVALID, "loss_a must be positive and finite for the Huber loss");
  if (loss_kind == BSGPU_LOSS_CAUCHY) return refuse(BSGPU_ERR_UNSUPPORTED, "the Cauchy loss is not supported (its logarithm differs between host and device)");
  if (inner->trust_region_strategy_type != BSGPU_TR_LEVENBERG_MARQUARDT)
    return refuse(BSGPU_ERR_UNSUPPORTED, "its in-kernel loop is Levenberg-Marquardt only (trust_region_strategy_type must be 0)");
  if (max_outer > BSGPU_LOAM_MAX_OUTER) return refuse(BSGPU_ERR_UNSUPPORTED, "max_outer exceeds BSGPU_LOAM_MAX_OUTER");
  if (inner->max_num_iterations > BSGPU_LOAM_MAX_INNER) return refuse(BSGPU_ERR_UNSUPPORTED, "inner->max_num_iterations exceeds BSGPU_LOAM_MAX_INNER");
  static_assert(BSGPU_LOAM_MAX_OUTER == kLoamMaxOuter && BSGPU_LOAM_MAX_INNER == kLoamMaxInner && BSGPU_LOAM_MAX_FEATURES == kLoamMaxFeatures,
                "the header's caps are loam.h's");
  static_assert(BSGPU_LOAM_MAX_ITERATIONS == LOAM_MAX_ITERATIONS && BSGPU_LOAM_TRANSFORM == LOAM_TRANSFORM &&
                BSGPU_LOAM_TOO_FEW_MEASUREMENTS == LOAM_TOO_FEW_MEASUREMENTS && BSGPU_LOAM_SOLVER_FAILED == LOAM_SOLVER_FAILED, "the header's status values are loam.h's");
  const size_t np = (size_t)n_pairs;
  std::vector<double> init(12 * np);
  static const char* const edge_names[4] = {"ref_edge_start", "reference edge", "tgt_edge_start", "target edge"};
  static const char* const surf_names[4] = {"ref_surf_start", "reference surface", "tgt_surf_start", "target surface"};
  if (const int rc = check_pair_table(me, n_pairs, ref_edge_start, ref_edges, tgt_edge_start, tgt_edges, T_init, init.data(), edge_names)) return rc;
  if (const int rc = check_pair_table(me, n_pairs, ref_surf_start, ref_surfs, tgt_surf_start, tgt_surfs, T_init, init.data(), surf_names)) return rc;
  const size_t n_re = (size_t)ref_edge_start[n_pairs], n_rs = (size_t)ref_surf_start[n_pairs], n_te = (size_t)tgt_edge_start[n_pairs],
               n_ts = (size_t)tgt_surf_start[n_pairs], n_ref = n_re + n_rs, n_tgt = n_te + n_ts;
  if (n_ref > (size_t)INT_MAX || n_tgt > (size_t)INT_MAX) return refuse(BSGPU_ERR_UNSUPPORTED, "more than 2^31 - 1 points in one call");
  // the call's reference clouds as one packed array, every pair's edges and then every pair's surfaces, each its own cloud with its own
  // grid (the identity as its transform); the target features packed likewise
  std::vector<double> ref(3 * n_ref), tgt(3 * n_tgt), T_cloud(24 * np);
  std::vector<int32_t> cloud_start(2 * np + 1, 0), feat_start(2 * np + 1, 0);
  if (n_re) std::memcpy(ref.data(), ref_edges, 24 * n_re);
  if (n_rs) std::memcpy(ref.data() + 3 * n_re, ref_surfs, 24 * n_rs);
  if (n_te) std::memcpy(tgt.data(), tgt_edges, 24 * n_te);
  if (n_ts) std::memcpy(tgt.data() + 3 * n_te, tgt_surfs, 24 * n_ts);
  for (size_t i = 0; i < 24 * np; ++i) T_cloud[i] = kEye[i % 12];
  for (size_t p = 0; p < np; ++p) {
    cloud_start[p + 1] = ref_edge_start[p + 1]; cloud_start[np + p + 1] = (int32_t)n_re + ref_surf_start[p + 1];
    feat_start[p + 1] = tgt_edge_start[p + 1]; feat_start[np + p + 1] = (int32_t)n_te + tgt_surf_start[p + 1];
    if ((tgt_edge_start[p + 1] - tgt_edge_start[p]) + (size_t)(tgt_surf_start[p + 1] - tgt_surf_start[p]) > (size_t)BSGPU_LOAM_MAX_FEATURES)
      return refuse(BSGPU_ERR_UNSUPPORTED, "a pair has more than BSGPU_LOAM_MAX_FEATURES target features");
  }
  GridsPlan G;
  if (const int rc = plan_grids(me, "reference cloud", 2 * np, cloud_start.data(), ref.data(), T_cloud.data(), grid_cell, &G)) return rc;
  if (n_pairs == 0) return BSGPU_OK;
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "hipSetDevice failed"); }
  LoamParams P;
  P.mc2 = max_corr * max_corr; P.min_measurements = min_measurements; P.max_outer = max_outer;
  P.conv_translation = conv_translation_m; P.cos_rotation = loam_cos_bound(conv_rotation_deg);
  P.loss_kind = loss_kind; P.loss_a = loss_a; P.inner = *inner;
  StageLayout L;
  const int s_cs = L.in(cloud_start.data(), 4 * (2 * np + 1)), s_ref = L.in(ref.data(), 24 * n_ref), s_tc = L.in(T_cloud.data(), 192 * np),
            s_gr = L.in(G.grids.data(), sizeof(PointGrid) * 2 * np), s_fs = L.in(feat_start.data(), 4 * (2 * np + 1)), s_tgt = L.in(tgt.data(), 24 * n_tgt),
            s_ti = L.in(init.data(), 96 * np);
  // per-pair records, split below: kLoamOutStride doubles and 5 ints (bsgpu_internal.h)
  const int s_od = L.out(nullptr, 8 * kLoamOutStride * np), s_oi = L.out(nullptr, 4 * 5 * np);
  // the kernels' working arrays (uninitialised): the grid build's over the reference clouds, the target features under T_init, the
  // measurements (three neighbour indices per target feature)
  const int s_rq = L.scratch(24 * n_ref), s_cell = L.scratch(4 * n_ref), s_cells = L.scratch(4 * (size_t)G.n_tiles * kGridScanTile),
            s_tile = L.scratch(4 * (size_t)G.n_tiles), s_rec = L.scratch(32 * n_ref), s_tq = L.scratch(24 * n_tgt), s_corr = L.scratch(12 * n_tgt);
  DeviceStage D(L);
  if (!D) return refuse(BSGPU_ERR_DEVICE, "out of device memory");
  const auto F = [&](int s) { return D.ptr<double>(s); };
  const auto I = [&](int s) { return D.ptr<int>(s); };
  const hipError_t e = D.run(nullptr, [&] {
    launch_register_scans_loam(nullptr, n_pairs, G.max_points, (int)n_ref, G.n_tiles, I(s_cs), F(s_ref), F(s_tc), D.ptr<PointGrid>(s_gr), I(s_fs),
                               F(s_tgt), F(s_ti), P, F(s_od), I(s_oi), F(s_rq), I(s_cell), I(s_cells), I(s_tile), F(s_rec), F(s_tq), I(s_corr));
  });
  if (e != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "device error"); }
  const double* od = L.out_image<double>(s_od);
  const int32_t* oi = L.out_image<int32_t>(s_oi);
  for (size_t p = 0; p < np; ++p) {
    const double* r = od + kLoamOutStride * p;
    std::memcpy(T_refest_ref + 12 * p, r, 12 * sizeof(double));
    if (T_ref_tgt) std::memcpy(T_ref_tgt + 12 * p, r + 12, 12 * sizeof(double));
    if (cov) std::memcpy(cov + 36 * p, r + 24, 36 * sizeof(double));
    if (cost) cost[p] = r[60];
    if (n_edge) n_edge[p] = oi[5 * p];
    if (n_surf) n_surf[p] = oi[5 * p + 1];
    if (n_iters) n_iters[p] = oi[5 * p + 2];
    if (n_inner) n_inner[p] = oi[5 * p + 3];
    status[p] = oi[5 * p + 4];
  }
  return BSGPU_OK;
} catch (...) {
  try { g_register_scans_error = "register_scans_loam: out of host memory"; } catch (...) {}
  return api_exception(nullptr);
}

int bsgpu_extract_loam_features(int device, int32_t n_scans, const int32_t* scan_start, const double* points, const int32_t* ring,
                                int32_t number_of_beams, double fov_deg, int32_t vertical_axis, int32_t n_feature_regions,
                                int32_t curvature_region, int32_t max_corner_sharp, int32_t max_corner_less_sharp, int32_t max_surface_flat,
                                double surface_curvature_threshold, int32_t downsample_less_flat_features, int32_t* edge_start,
                                int32_t* edge_index, double* edge_points, int32_t* surf_start, int32_t* surf_index, double* surf_points,
                                int32_t* weak_edge_start, int32_t* weak_edge_index, double* weak_edge_points, int32_t* weak_surf_start,
                                int32_t* weak_surf_index, double* weak_surf_points, int32_t* label, double* curvature) try {
  const char* const me = "extract_loam_features";
  const auto refuse = [me](int code, const char* why) { return refuse_scans(code, me, why); };
  const bool weak = weak_edge_start || weak_edge_index || weak_edge_points || weak_surf_start || weak_surf_index || weak_surf_points;
  if (n_scans < 0 || !scan_start || !edge_start || !edge_index || !surf_start || !surf_index) return refuse(BSGPU_ERR_INVALID, "null argument");
  if (weak && (!weak_edge_start || !weak_edge_index || !weak_surf_start || !weak_surf_index))
    return refuse(BSGPU_ERR_INVALID, "the weak clouds come as a group: both start tables and both index arrays, or none");
  if (number_of_beams < 1) return refuse(BSGPU_ERR_INVALID, "number_of_beams must be at least 1");
  if (n_feature_regions < 1) return refuse(BSGPU_ERR_INVALID, "n_feature_regions must be at least 1");
  if (curvature_region < 1) return refuse(BSGPU_ERR_INVALID, "curvature_region must be at least 1");
  if (max_corner_sharp < 0 || max_corner_less_sharp < 0 || max_surface_flat < 0)
    return refuse(BSGPU_ERR_INVALID, "max_corner_sharp, max_corner_less_sharp and max_surface_flat must not be negative");
  if (!(fov_deg > 0.0) || !(fov_deg < 180.0)) return refuse(BSGPU_ERR_INVALID, "fov_deg must lie in (0, 180)");
  if (!std::isfinite(surface_curvature_threshold)) return refuse(BSGPU_ERR_INVALID, "surface_curvature_threshold must be finite");
  if (vertical_axis < BSGPU_AXIS_X || vertical_axis > BSGPU_AXIS_Z) return refuse(BSGPU_ERR_INVALID, "unknown vertical_axis");
  if (number_of_beams > BSGPU_LOAM_MAX_RINGS) return refuse(BSGPU_ERR_UNSUPPORTED, "number_of_beams exceeds BSGPU_LOAM_MAX_RINGS");
  if (curvature_region > BSGPU_LOAM_MAX_CURVATURE_REGION) return refuse(BSGPU_ERR_UNSUPPORTED, "curvature_region exceeds BSGPU_LOAM_MAX_CURVATURE_REGION");
  if (n_feature_regions > BSGPU_LOAM_MAX_REGIONS) return refuse(BSGPU_ERR_UNSUPPORTED, "n_feature_regions exceeds BSGPU_LOAM_MAX_REGIONS");
  if (downsample_less_flat_features != 0)
    return refuse(BSGPU_ERR_UNSUPPORTED, "downsample_less_flat_features is not supported (a voxel grid over features that every shipped matcher ignores)");
  static_assert(BSGPU_LOAM_MAX_RINGS == kLoamMaxRings && BSGPU_LOAM_MAX_RING_POINTS == kLoamMaxRingPoints &&
                BSGPU_LOAM_MAX_CURVATURE_REGION == kLoamMaxCurvatureRegion && BSGPU_LOAM_MAX_REGIONS == kLoamMaxRegions, "the header's caps are loam_features.h's");
  static_assert(BSGPU_LOAM_DROPPED == LOAM_FEAT_DROPPED && BSGPU_LOAM_LESS_FLAT == LOAM_FEAT_LESS_FLAT && BSGPU_LOAM_FLAT == LOAM_FEAT_FLAT &&
                BSGPU_LOAM_LESS_SHARP == LOAM_FEAT_LESS_SHARP && BSGPU_LOAM_SHARP == LOAM_FEAT_SHARP, "the header's labels are loam_features.h's");
  switch (check_start_table(scan_start, n_scans, INT_MAX, [&](int k) { return scan_start[k + 1] == scan_start[k] || points; })) {
    case kStartNotZero: return refuse(BSGPU_ERR_INVALID, "scan_start[0] must be 0");
    case kStartDecreasing: return refuse(BSGPU_ERR_INVALID, "scan_start must be non-decreasing");
    case kStartBadItem: return refuse(BSGPU_ERR_INVALID, "null points");
    default: break;
  }
  if (n_scans == 0) return BSGPU_OK;
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "hipSetDevice failed"); }
  const size_t ns = (size_t)n_scans, np = (size_t)scan_start[n_scans], beams = (size_t)number_of_beams, regions = (size_t)n_feature_regions;
  LoamFeatParams P;
  P.beams = number_of_beams; P.regions = n_feature_regions; P.c = curvature_region;
  P.max_sharp = max_corner_sharp; P.max_less_sharp = max_corner_less_sharp; P.max_flat = max_surface_flat;
  P.axis = vertical_axis; P.threshold = surface_curvature_threshold;
  std::vector<double> bound(beams + 1);
  loam_feat_bounds(number_of_beams, fov_deg, bound.data());
  // a ring's picks are distinct positions, so they are at most its points
  const size_t per_region = (size_t)std::min(max_corner_less_sharp, kLoamMaxRingPoints) + (size_t)std::min(max_surface_flat, kLoamMaxRingPoints);
  const size_t pick_cap = std::min((size_t)kLoamMaxRingPoints, regions * per_region);
  StageLayout L;
  const int s_ss = L.in(scan_start, 4 * (ns + 1)), s_pts = L.in(points, 24 * np), s_ring = L.in(ring, ring ? 4 * np : 0), s_bd = L.in(bound.data(), 8 * (beams + 1));
  // per point: ring, label, curvature; per (scan, ring): the picks and two counts per region; the overflow flag.  The host packs below.
  const int s_rid = L.out(nullptr, 4 * np), s_lab = L.out(label, 4 * np), s_cv = L.out(curvature, 8 * np), s_pk = L.out(nullptr, 4 * ns * beams * pick_cap),
            s_cnt = L.out(nullptr, 8 * ns * beams * regions), s_of = L.out(nullptr, 4);
  DeviceStage D(L);
  if (!D) return refuse(BSGPU_ERR_DEVICE, "out of device memory");
  const auto I = [&](int s) { return D.ptr<int>(s); };
  const hipError_t e = D.run(nullptr, [&] {
    launch_extract_loam_features(nullptr, n_scans, (int)np, I(s_ss), D.ptr<double>(s_pts), ring ? I(s_ring) : nullptr, P, D.ptr<double>(s_bd),
                                 (int)pick_cap, I(s_rid), I(s_lab), D.ptr<double>(s_cv), I(s_pk), I(s_cnt), I(s_of));
  });
  if (e != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "device error"); }
  if (*L.out_image<int32_t>(s_of) != 0) return refuse(BSGPU_ERR_UNSUPPORTED, "a ring has more than BSGPU_LOAM_MAX_RING_POINTS points");
  const int32_t *rid = L.out_image<int32_t>(s_rid), *lab = L.out_image<int32_t>(s_lab), *pk = L.out_image<int32_t>(s_pk), *cnt = L.out_image<int32_t>(s_cnt);
  L.scatter();      // label and curvature
  // The packing: within a scan ring, then region, then pick order; LESS_FLAT by ring and position.
  struct Cloud { int32_t *start, *index; double* pts; int32_t n; };
  Cloud sharp{edge_start, edge_index, edge_points, 0}, flat{surf_start, surf_index, surf_points, 0},
        less_sharp{weak_edge_start, weak_edge_index, weak_edge_points, 0}, less_flat{weak_surf_start, weak_surf_index, weak_surf_points, 0};
  const auto put = [&](Cloud& C, size_t scan, int32_t i) {
    C.index[C.n] = i;
    if (C.pts) std::memcpy(C.pts + 3 * (size_t)C.n, points + 3 * ((size_t)scan_start[scan] + (size_t)i), 24);
    ++C.n;
  };
  std::vector<int32_t> at(beams + 1);
  sharp.start[0] = 0; flat.start[0] = 0;
  if (weak) { less_sharp.start[0] = 0; less_flat.start[0] = 0; }
  for (size_t s = 0; s < ns; ++s) {
    for (size_t r = 0; r < beams; ++r) {
      const int32_t* p = pk + (s * beams + r) * pick_cap;
      for (size_t j = 0; j < regions; ++j) {
        const int32_t ne = cnt[2 * ((s * beams + r) * regions + j)], nf = cnt[2 * ((s * beams + r) * regions + j) + 1];
        for (int32_t k = 0; k < ne; ++k, ++p) {
          if (k < max_corner_sharp) put(sharp, s, *p);
          else if (weak) put(less_sharp, s, *p);
        }
        for (int32_t k = 0; k < nf; ++k, ++p) put(flat, s, *p);
      }
    }
    sharp.start[s + 1] = sharp.n; flat.start[s + 1] = flat.n;
    if (!weak) continue;
    less_sharp.start[s + 1] = less_sharp.n;
    // a stable partition of the scan's LESS_FLAT points by ring
    const size_t s0 = (size_t)scan_start[s], s1 = (size_t)scan_start[s + 1];
    std::fill(at.begin(), at.end(), 0);
    for (size_t i = s0; i < s1; ++i) if (lab[i] == LOAM_FEAT_LESS_FLAT) ++at[(size_t)rid[i] + 1];
    for (size_t r = 0; r < beams; ++r) at[r + 1] += at[r];
    const int32_t base = less_flat.n;
    for (size_t i = s0; i < s1; ++i) {
      if (lab[i] != LOAM_FEAT_LESS_FLAT) continue;
      const int32_t k = base + at[(size_t)rid[i]]++;
      less_flat.index[k] = (int32_t)(i - s0);
      if (less_flat.pts) std::memcpy(less_flat.pts + 3 * (size_t)k, points + 3 * i, 24);
    }
    less_flat.n = base + at[beams - 1];
    less_flat.start[s + 1] = less_flat.n;
  }
  return BSGPU_OK;
} catch (...) {
  try { g_register_scans_error = "extract_loam_features: out of host memory"; } catch (...) {}
  return api_exception(nullptr);
}

int bsgpu_build_registration_maps(int device, int32_t n_maps, const int32_t* map_scan_start, const int32_t* scan_start, const double* points,
                                  const double* T_map_scan, double voxel_size, int32_t* map_start, double* map_points, int32_t* map_count) try {
  const char* const me = "build_registration_maps";
  const auto refuse = [me](int code, const char* why) { return refuse_scans(code, me, why); };
  static_assert(BSGPU_MAP_MAX_POINTS == kMapMaxPoints && BSGPU_MAP_SORT_TILE == kMapSortTile, "the header's constants are registration_map.h's");
  if (n_maps < 0 || !map_scan_start || !scan_start || !map_start || !map_points) return refuse(BSGPU_ERR_INVALID, "null argument");
  if (!(voxel_size == kMapMergeOnly) && !(voxel_size > 0.0 && std::isfinite(voxel_size)))
    return refuse(BSGPU_ERR_INVALID, "voxel_size must be -1 (merge only) or positive and finite");
  switch (check_start_table(map_scan_start, n_maps)) {
    case kStartNotZero: return refuse(BSGPU_ERR_INVALID, "map_scan_start[0] must be 0");
    case kStartDecreasing: return refuse(BSGPU_ERR_INVALID, "map_scan_start must be non-decreasing");
    default: break;
  }
  const int32_t n_scans = map_scan_start[n_maps];
  switch (check_start_table(scan_start, n_scans, INT_MAX, [&](int k) { return scan_start[k + 1] == scan_start[k] || points; })) {
    case kStartNotZero: return refuse(BSGPU_ERR_INVALID, "scan_start[0] must be 0");
    case kStartDecreasing: return refuse(BSGPU_ERR_INVALID, "scan_start must be non-decreasing");
    case kStartBadItem: return refuse(BSGPU_ERR_INVALID, "null points");
    default: break;
  }
  if (T_map_scan)
    for (size_t i = 0; i < 12 * (size_t)n_scans; ++i) if (!std::isfinite(T_map_scan[i])) return refuse(BSGPU_ERR_INVALID, "non-finite T_map_scan");
  if (scan_start[n_scans] > BSGPU_MAP_MAX_POINTS) return refuse(BSGPU_ERR_UNSUPPORTED, "the call holds more than BSGPU_MAP_MAX_POINTS points");
  if (n_maps == 0) return BSGPU_OK;
  const size_t nm = (size_t)n_maps, ns = (size_t)n_scans, np = (size_t)scan_start[n_scans];
  if (np == 0) {
    std::fill(map_start, map_start + nm + 1, 0);
    return BSGPU_OK;
  }
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "hipSetDevice failed"); }
  // a map's points are one range of the call's; its tiles of kMapSortTile positions follow those of the maps before it
  std::vector<int32_t> pt_start(nm + 1), tile_start(nm + 1, 0), tile_map;
  for (size_t m = 0; m <= nm; ++m) pt_start[m] = scan_start[map_scan_start[m]];
  for (size_t m = 0; m < nm; ++m) {
    const int32_t tiles = (pt_start[m + 1] - pt_start[m] + kMapSortTile - 1) / kMapSortTile;
    tile_start[m + 1] = tile_start[m] + tiles;
    tile_map.insert(tile_map.end(), (size_t)tiles, (int32_t)m);
  }
  const size_t nt = tile_map.size();
  const bool sorted = voxel_size != kMapMergeOnly;
  StageLayout L;
  const int s_ss = L.in(scan_start, 4 * (ns + 1)), s_pts = L.in(points, 24 * np), s_T = L.in(T_map_scan, T_map_scan ? 96 * ns : 0),
            s_ps = L.in(pt_start.data(), 4 * (nm + 1)), s_ts = L.in(tile_start.data(), 4 * (nm + 1)), s_tm = L.in(tile_map.data(), 4 * nt);
  // fixed capacity: map m's voxels from the position of its first input point; the host packs below
  const int s_op = L.out(nullptr, 24 * np), s_oc = L.out(nullptr, 4 * np), s_nv = L.out(nullptr, 4 * nm), s_rf = L.out(nullptr, 4);
  const size_t sn = sorted ? np : 0, st = sorted ? nt : 0;
  const int s_tq = L.scratch(24 * sn), s_ka = L.scratch(8 * sn), s_kb = L.scratch(8 * sn), s_ia = L.scratch(4 * sn), s_ib = L.scratch(4 * sn),
            s_h = L.scratch(4 * 256 * st), s_th = L.scratch(4 * st);
  DeviceStage D(L);
  if (!D) return refuse(BSGPU_ERR_DEVICE, "out of device memory");
  const auto I = [&](int s) { return D.ptr<int>(s); };
  const hipError_t e = D.run(nullptr, [&] {
    launch_build_registration_maps(nullptr, n_maps, n_scans, (int)np, (int)nt, I(s_ss), D.ptr<double>(s_pts), T_map_scan ? D.ptr<double>(s_T) : nullptr,
                                   voxel_size, I(s_ps), I(s_ts), I(s_tm), D.ptr<double>(s_tq), D.ptr<unsigned long long>(s_ka),
                                   D.ptr<unsigned long long>(s_kb), I(s_ia), I(s_ib), I(s_h), I(s_th), D.ptr<double>(s_op), I(s_oc), I(s_nv), I(s_rf));
  });
  if (e != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "device error"); }
  if (*L.out_image<int32_t>(s_rf) != 0) return refuse(BSGPU_ERR_UNSUPPORTED, "a transformed coordinate has |q / voxel_size| >= 2^20");
  const double* op = L.out_image<double>(s_op);
  const int32_t *oc = L.out_image<int32_t>(s_oc), *nv = L.out_image<int32_t>(s_nv);
  for (size_t m = 0; m < nm; ++m) if (nv[m] < 0 || nv[m] > pt_start[m + 1] - pt_start[m]) return refuse(BSGPU_ERR_DEVICE, "device error");
  map_start[0] = 0;
  for (size_t m = 0; m < nm; ++m) {
    const size_t at = (size_t)map_start[m], from = (size_t)pt_start[m], k = (size_t)nv[m];
    if (k) {
      std::memcpy(map_points + 3 * at, op + 3 * from, 24 * k);
      if (map_count) std::memcpy(map_count + at, oc + from, 4 * k);
    }
    map_start[m + 1] = (int32_t)(at + k);
  }
  return BSGPU_OK;
} catch (...) {
  try { g_register_scans_error = "build_registration_maps: out of host memory"; } catch (...) {}
  return api_exception(nullptr);
}

const char* bsgpu_scan_context_error(void) { return g_scan_context_error.c_str(); }

int bsgpu_scan_context_describe(int device, int32_t n_scans, const int32_t* scan_start, const double* points, int32_t n_aggregates,
                                const int32_t* member_start, const int32_t* member_scan, const double* member_T, double lidar_height,
                                double max_radius, double* desc, double* ring_key, double* sector_key, int32_t* n_binned) try {
  const auto refuse = [](int code, const char* why) { g_scan_context_error = why; return code; };
  if (n_scans < 0 || n_aggregates < 0 || !scan_start || !member_start || !desc) return refuse(BSGPU_ERR_INVALID, "scan_context_describe: null argument");
  if (!(max_radius > 0.0) || !std::isfinite(max_radius)) return refuse(BSGPU_ERR_INVALID, "scan_context_describe: max_radius must be positive and finite");
  if (!std::isfinite(lidar_height)) return refuse(BSGPU_ERR_INVALID, "scan_context_describe: lidar_height must be finite");
  const auto finite_scan = [&](int k) {
    if (scan_start[k + 1] > scan_start[k] && !points) return false;
    for (size_t i = 3 * (size_t)scan_start[k]; i < 3 * (size_t)scan_start[k + 1]; ++i) if (!std::isfinite(points[i])) return false;
    return true;
  };
  switch (check_start_table(scan_start, n_scans, kScMaxScanPoints)) {     // (the table alone first: a scan too long is refused before a point is read)
    case kStartNotZero: return refuse(BSGPU_ERR_INVALID, "scan_context_describe: scan_start[0] must be 0");
    case kStartDecreasing: return refuse(BSGPU_ERR_INVALID, "scan_context_describe: scan_start must be non-decreasing");
    case kStartTooLong: return refuse(BSGPU_ERR_UNSUPPORTED, "scan_context_describe: a scan holds more than BSGPU_SC_MAX_SCAN_POINTS points");
    default: break;
  }
  if (check_start_table(scan_start, n_scans, INT_MAX, finite_scan) != kStartOk)
    return refuse(BSGPU_ERR_INVALID, "scan_context_describe: null or non-finite points");
  const auto members_ok = [&](int a) {
    if (member_start[a + 1] > member_start[a] && !member_scan) return false;
    for (int m = member_start[a]; m < member_start[a + 1]; ++m) if (member_scan[m] < 0 || member_scan[m] >= n_scans) return false;
    return true;
  };
  switch (check_start_table(member_start, n_aggregates, INT_MAX, members_ok)) {
    case kStartNotZero: return refuse(BSGPU_ERR_INVALID, "scan_context_describe: member_start[0] must be 0");
    case kStartDecreasing: return refuse(BSGPU_ERR_INVALID, "scan_context_describe: member_start must be non-decreasing");
    case kStartBadItem: return refuse(BSGPU_ERR_INVALID, "scan_context_describe: null member_scan or a member index out of range");
    default: break;
  }
  if (n_aggregates == 0) return BSGPU_OK;
  const size_t na = (size_t)n_aggregates, nm = (size_t)member_start[n_aggregates], np = (size_t)scan_start[n_scans];
  static const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  std::vector<double> T(12 * nm);
  for (size_t i = 0; i < T.size(); ++i) {
    T[i] = member_T ? member_T[i] : eye[i % 12];
    if (!std::isfinite(T[i])) return refuse(BSGPU_ERR_INVALID, "scan_context_describe: non-finite member_T");
  }
  std::vector<int32_t> member_agg(nm);
  int max_chunks = 0;
  for (int a = 0; a < n_aggregates; ++a)
    for (int m = member_start[a]; m < member_start[a + 1]; ++m) {
      member_agg[m] = a;
      const int n = scan_start[member_scan[m] + 1] - scan_start[member_scan[m]];
      max_chunks = std::max(max_chunks, (int)(((int64_t)n + kScChunk - 1) / kScChunk));
    }
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "scan_context_describe: hipSetDevice failed"); }
  StageLayout L;
  const int s_ss = L.in(scan_start, 4 * ((size_t)n_scans + 1)), s_pts = L.in(points, 24 * np), s_ms = L.in(member_scan, 4 * nm),
            s_ma = L.in(member_agg.data(), 4 * nm), s_T = L.in(T.data(), 96 * nm);
  const int s_desc = L.out(desc, 8 * kScBins * na), s_rk = L.out(ring_key, 8 * kScRings * na), s_sk = L.out(sector_key, 8 * kScSectors * na),
            s_nb = L.out(n_binned, 4 * na);
  // the kernels' working arrays (the launch clears them): every aggregate's table of integer keys, its count of kept points
  const int s_tab = L.scratch(8 * kScBins * na), s_cnt = L.scratch(4 * na);
  DeviceStage D(L);
  if (!D) return refuse(BSGPU_ERR_DEVICE, "scan_context_describe: out of device memory");
  const auto F = [&](int s) { return D.ptr<double>(s); };
  const auto I = [&](int s) { return D.ptr<int>(s); };
  const hipError_t e = D.run(nullptr, [&] {
    launch_scan_context_describe(nullptr, n_aggregates, (int)nm, max_chunks, I(s_ss), F(s_pts), I(s_ms), I(s_ma), F(s_T), lidar_height, max_radius,
                                 F(s_desc), F(s_rk), F(s_sk), I(s_nb), D.ptr<unsigned long long>(s_tab), I(s_cnt));
  });
  if (e != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "scan_context_describe: device error"); }
  L.scatter();
  return BSGPU_OK;
} catch (...) {
  try { g_scan_context_error = "scan_context_describe: out of host memory"; } catch (...) {}
  return api_exception(nullptr);
}

int bsgpu_scan_context_match(int device, int32_t n_sets, const int32_t* query_start, const double* query_desc, const int32_t* cand_start,
                             const double* cand_desc, int32_t n_tree_candidates, double search_ratio, double dist_thres, int32_t* best_cand,
                             double* best_dist, int32_t* best_shift, double* yaw, double* dist_all, int32_t* shift_all) try {
  const auto refuse = [](int code, const char* why) { g_scan_context_error = why; return code; };
  if (n_sets < 0 || !query_start || !cand_start || !best_cand || !best_dist || !best_shift)
    return refuse(BSGPU_ERR_INVALID, "scan_context_match: null argument");
  if (!(search_ratio >= 0.0)) return refuse(BSGPU_ERR_INVALID, "scan_context_match: search_ratio must not be negative or NaN");
  if (!(dist_thres >= 0.0)) return refuse(BSGPU_ERR_INVALID, "scan_context_match: dist_thres must not be negative or NaN");
  const auto finite_items = [](const int32_t* start, const double* d) {
    return [start, d](int k) {
      if (start[k + 1] > start[k] && !d) return false;
      for (size_t i = (size_t)kScBins * start[k]; i < (size_t)kScBins * start[k + 1]; ++i) if (!std::isfinite(d[i])) return false;
      return true;
    };
  };
  switch (check_start_table(query_start, n_sets, INT_MAX, finite_items(query_start, query_desc))) {
    case kStartNotZero: return refuse(BSGPU_ERR_INVALID, "scan_context_match: query_start[0] must be 0");
    case kStartDecreasing: return refuse(BSGPU_ERR_INVALID, "scan_context_match: query_start must be non-decreasing");
    case kStartBadItem: return refuse(BSGPU_ERR_INVALID, "scan_context_match: null or non-finite query descriptors");
    default: break;
  }
  switch (check_start_table(cand_start, n_sets, kScMaxCandidates)) {     // (the table alone first: a set too long is refused before a descriptor is read)
    case kStartNotZero: return refuse(BSGPU_ERR_INVALID, "scan_context_match: cand_start[0] must be 0");
    case kStartDecreasing: return refuse(BSGPU_ERR_INVALID, "scan_context_match: cand_start must be non-decreasing");
    case kStartTooLong: return refuse(BSGPU_ERR_UNSUPPORTED, "scan_context_match: a set holds more than BSGPU_SC_MAX_CANDIDATES candidates");
    default: break;
  }
  if (check_start_table(cand_start, n_sets, INT_MAX, finite_items(cand_start, cand_desc)) != kStartOk)
    return refuse(BSGPU_ERR_INVALID, "scan_context_match: null or non-finite candidate descriptors");
  if (n_tree_candidates > kScMaxTree) return refuse(BSGPU_ERR_UNSUPPORTED, "scan_context_match: n_tree_candidates exceeds BSGPU_SC_MAX_TREE_CANDIDATES");
  const size_t nq = n_sets > 0 ? (size_t)query_start[n_sets] : 0;
  if (nq == 0) return BSGPU_OK;
  const size_t ncand = (size_t)cand_start[n_sets];
  const int K = n_tree_candidates > 0 ? n_tree_candidates : 0;
  std::vector<int32_t> query_set(nq);
  std::vector<int64_t> pair_start(nq);
  int64_t pairs = 0;
  int max_cands = 0;
  bool any_select = false;
  for (int s = 0; s < n_sets; ++s) {
    const int nc = cand_start[s + 1] - cand_start[s];
    if (query_start[s + 1] > query_start[s]) { max_cands = std::max(max_cands, nc); any_select = any_select || (K > 0 && K < nc); }
    for (int q = query_start[s]; q < query_start[s + 1]; ++q) { query_set[q] = s; pair_start[q] = pairs; pairs += nc; }
  }
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "scan_context_match: hipSetDevice failed"); }
  const size_t n_pairs = (size_t)pairs;
  StageLayout L;
  const int s_qs = L.in(query_set.data(), 4 * nq), s_ps = L.in(pair_start.data(), 8 * nq), s_qd = L.in(query_desc, 8 * kScBins * nq),
            s_cs = L.in(cand_start, 4 * ((size_t)n_sets + 1)), s_cd = L.in(cand_desc, 8 * kScBins * ncand);
  const int s_bc = L.out(best_cand, 4 * nq), s_bd = L.out(best_dist, 8 * nq), s_bs = L.out(best_shift, 4 * nq), s_yaw = L.out(yaw, 8 * nq),
            s_da = L.out(dist_all, 8 * n_pairs), s_sa = L.out(shift_all, 4 * n_pairs);
  // the pre-selection's working arrays (written before they are read, and only for sets larger than K): ring-key distances, flags
  const int s_d2 = L.scratch(any_select ? 8 * n_pairs : 0), s_take = L.scratch(any_select ? 4 * n_pairs : 0);
  DeviceStage D(L);
  if (!D) return refuse(BSGPU_ERR_DEVICE, "scan_context_match: out of device memory");
  const auto F = [&](int s) { return D.ptr<double>(s); };
  const auto I = [&](int s) { return D.ptr<int>(s); };
  const hipError_t e = D.run(nullptr, [&] {
    launch_scan_context_match(nullptr, (int)nq, max_cands, any_select, I(s_qs), D.ptr<long long>(s_ps), F(s_qd), I(s_cs), F(s_cd), K,
                              sc_search_radius(search_ratio), dist_thres, I(s_bc), F(s_bd), I(s_bs), F(s_yaw), F(s_da), I(s_sa), F(s_d2),
                              I(s_take));
  });
  if (e != hipSuccess) { (void)hipGetLastError(); return refuse(BSGPU_ERR_DEVICE, "scan_context_match: device error"); }
  L.scatter();
  return BSGPU_OK;
} catch (...) {
  try { g_scan_context_error = "scan_context_match: out of host memory"; } catch (...) {}
  return api_exception(nullptr);
}

int bsgpu_triangulate(bsgpu_ctx* c, int32_t n_tracks, const int32_t* track_start, const int32_t* q_block, const int32_t* p_block,
                      const double* pixels, int32_t camera, int32_t truncate_pixels, double max_dist, double max_reproj, double* points,
                      int32_t* status) try {
  if (!c) return BSGPU_ERR_INVALID;
  if (n_tracks < 0 || !track_start || !points || !status) return fail(c, BSGPU_ERR_INVALID, "null argument");
  if (n_tracks == 0) return BSGPU_OK;
  const int n_obs = track_start[n_tracks];
  const StartCheck table = check_start_table(track_start, n_tracks);
  if (table == kStartNotZero || n_obs < 0 || (n_obs > 0 && (!q_block || !p_block || !pixels)))
    return fail(c, BSGPU_ERR_INVALID, "triangulate: malformed track table");
  if (camera < 0 || camera >= (int)c->cams.size()) return fail(c, BSGPU_ERR_INVALID, "camera index out of range");
  if (table == kStartDecreasing) return fail(c, BSGPU_ERR_INVALID, "triangulate: track_start must be non-decreasing");
  std::vector<int32_t> pose_off((size_t)2 * n_obs);
  for (int o = 0; o < n_obs; ++o) {
    const int qb = q_block[o], pb = p_block[o];
    if (qb < 0 || qb >= c->nb || pb < 0 || pb >= c->nb) return fail(c, BSGPU_ERR_INVALID, "triangulate: block out of range");
    if (c->size[qb] != 4 || c->size[pb] != 3) return fail(c, BSGPU_ERR_INVALID, "triangulate: view blocks must be (orientation[4], position[3])");
    pose_off[2 * (size_t)o] = c->off[qb];
    pose_off[2 * (size_t)o + 1] = c->off[pb];
  }
  int rc = finalize(c);
  if (rc != BSGPU_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const DevCamera cam = to_dev_camera(c->cams[camera]);
  const size_t nt = (size_t)n_tracks;
  StageLayout L;
  const int s_start = L.in(track_start, 4 * (nt + 1)), s_off = L.in(pose_off.data(), 8 * (size_t)n_obs), s_pix = L.in(pixels, 16 * (size_t)n_obs),
            s_pts = L.out(points, 24 * nt), s_status = L.out(status, 4 * nt);
  DeviceStage D(L);
  if (!D) return fail(c, BSGPU_ERR_DEVICE, "triangulate: device error");
  const hipError_t e = D.run(c->stream, [&] {
    launch_triangulate(c->stream, n_tracks, D.ptr<int>(s_start), D.ptr<int2>(s_off), D.ptr<double2>(s_pix), c->d_x, cam,
                       truncate_pixels != 0, max_dist, max_reproj, D.ptr<double>(s_pts), D.ptr<int>(s_status));
  });
  if (e != hipSuccess) return fail(c, BSGPU_ERR_DEVICE, "triangulate: device error");
  L.scatter();
  return BSGPU_OK;
} catch (...) { return api_exception(c); }

int bsgpu_localize_frames(bsgpu_ctx* c, int32_t n_frames, const int32_t* obs_start, const double* pixels, const double* points,
                          const int32_t* lm_block, const int32_t* camera, const double* q_init, const double* p_init,
                          int32_t loss_kind, double loss_a, double sqrt_info, int32_t truncate_pixels, int32_t min_points,
                          int32_t image_width, int32_t image_height, const bsgpu_options* options, double* q_out, double* p_out,
                          double* cov_out, double* avg_reproj, double* final_cost, int32_t* iterations, int32_t* status) try {
  if (!c) return BSGPU_ERR_INVALID;
  if (n_frames < 0 || !obs_start || !camera || !q_init || !p_init || !options || !q_out || !p_out || !status)
    return fail(c, BSGPU_ERR_INVALID, "localize_frames: null argument");
  if ((points == nullptr) == (lm_block == nullptr)) return fail(c, BSGPU_ERR_INVALID, "localize_frames: pass exactly one of points and lm_block");
  if (options->trust_region_strategy_type != BSGPU_TR_LEVENBERG_MARQUARDT)
    return fail(c, BSGPU_ERR_UNSUPPORTED, "localize_frames: its in-kernel loop is Levenberg-Marquardt only (trust_region_strategy_type must be 0)");
  if (loss_kind < BSGPU_LOSS_TRIVIAL || loss_kind > BSGPU_LOSS_HUBER) return fail(c, BSGPU_ERR_INVALID, "unknown loss kind");
  switch (check_start_table(obs_start, n_frames, INT_MAX, [&](int f) { return camera[f] >= 0 && camera[f] < (int)c->cams.size(); })) {
    case kStartNotZero: return fail(c, BSGPU_ERR_INVALID, "localize_frames: obs_start[0] must be 0");
    case kStartDecreasing: return fail(c, BSGPU_ERR_INVALID, "localize_frames: obs_start must be non-decreasing");
    case kStartBadItem: return fail(c, BSGPU_ERR_INVALID, "camera index out of range");
    default: break;
  }
  const size_t n_obs = (size_t)obs_start[n_frames], nf = (size_t)n_frames;
  if (n_obs > 0 && !pixels) return fail(c, BSGPU_ERR_INVALID, "localize_frames: null pixels");
  std::vector<int32_t> pt_off;
  if (lm_block) {
    if (!c->finalized || !c->d_x) return fail(c, BSGPU_ERR_INVALID, "localize_frames: lm_block needs the context's values on the device (finalize or solve first)");
    pt_off.resize(n_obs);
    for (size_t o = 0; o < n_obs; ++o) {
      const int b = lm_block[o];
      if (b < 0 || b >= c->nb) return fail(c, BSGPU_ERR_INVALID, "localize_frames: block out of range");
      if (c->size[b] != 3 || c->manifold[b] != BSGPU_MANIFOLD_EUCLIDEAN) return fail(c, BSGPU_ERR_INVALID, "localize_frames: lm_block must name 3-d Euclidean blocks");
      pt_off[o] = c->off[b];
    }
  }
  if (n_frames == 0) return BSGPU_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const std::vector<DevCamera> cams = dev_cameras(c);
  std::vector<double> pose(7 * nf);
  for (size_t f = 0; f < nf; ++f) {
    std::memcpy(&pose[7 * f], q_init + 4 * f, 4 * sizeof(double));
    std::memcpy(&pose[7 * f + 4], p_init + 3 * f, 3 * sizeof(double));
  }
  StageLayout L;
  const int s_start = L.in(obs_start, 4 * (nf + 1)), s_cam = L.in(camera, 4 * nf), s_off = L.in(pt_off.data(), 4 * pt_off.size()),
            s_cams = L.in(cams.data(), sizeof(DevCamera) * cams.size()), s_pix = L.in(pixels, 16 * n_obs),
            s_pts = L.in(points, points ? 24 * n_obs : 0), s_pose = L.in(pose.data(), 8 * pose.size());
  // per-frame records, split below: kLocOutStride doubles and 2 ints (bsgpu_internal.h)
  const int s_od = L.out(nullptr, 8 * kLocOutStride * nf), s_oi = L.out(nullptr, 4 * 2 * nf);
  DeviceStage D(L);
  if (!D) return fail(c, BSGPU_ERR_DEVICE, "localize_frames: out of device memory");
  const hipError_t e = D.run(c->stream, [&] {
    launch_localize(c->stream, n_frames, D.ptr<int>(s_start), D.ptr<double2>(s_pix), points ? D.ptr<double>(s_pts) : nullptr,
                    lm_block ? D.ptr<int>(s_off) : nullptr, lm_block ? c->d_x : nullptr, D.ptr<DevCamera>(s_cams), D.ptr<int>(s_cam),
                    D.ptr<double>(s_pose), loss_kind, loss_a, sqrt_info, truncate_pixels != 0 ? 1 : 0, min_points, image_width, image_height,
                    *options, D.ptr<double>(s_od), D.ptr<int>(s_oi));
  });
  if (e != hipSuccess) return fail(c, BSGPU_ERR_DEVICE, "localize_frames: device error");
  const double* od = L.out_image<double>(s_od);
  const int32_t* oi = L.out_image<int32_t>(s_oi);
  for (size_t f = 0; f < nf; ++f) {
    const double* r = od + kLocOutStride * f;
    std::memcpy(q_out + 4 * f, r, 4 * sizeof(double));
    std::memcpy(p_out + 3 * f, r + 4, 3 * sizeof(double));
    if (final_cost) final_cost[f] = r[7];
    if (avg_reproj) avg_reproj[f] = r[8];
    if (cov_out) std::memcpy(cov_out + 36 * f, r + 9, 36 * sizeof(double));
    if (iterations) iterations[f] = oi[2 * f];
    status[f] = oi[2 * f + 1];
  }
  return BSGPU_OK;
} catch (...) { return api_exception(c); }

int bsgpu_essential_ransac(bsgpu_ctx* c, int32_t n_sets, const int32_t* match_start, const double* px_prev, const double* px_cur,
                           const double* K, double prob, double threshold_px, int32_t max_iters, uint64_t seed, uint8_t* mask, double* E,
                           int32_t* n_inliers, int32_t* n_iters, int32_t* best_sample, int32_t* status) try {
  if (!c) return BSGPU_ERR_INVALID;
  if (n_sets < 0 || !match_start || !px_prev || !px_cur || !K || !mask || !status)
    return fail(c, BSGPU_ERR_INVALID, "essential_ransac: null argument");
  if (!(prob > 0.0 && prob < 1.0)) return fail(c, BSGPU_ERR_INVALID, "essential_ransac: prob must lie inside (0, 1)");
  if (!(threshold_px > 0.0) || max_iters <= 0) return fail(c, BSGPU_ERR_INVALID, "essential_ransac: threshold_px and max_iters must be positive");
  switch (check_start_table(match_start, n_sets, BSGPU_RANSAC_MAX_MATCHES, [&](int k) { return K[4 * (size_t)k] > 0.0 && K[4 * (size_t)k + 1] > 0.0; })) {
    case kStartNotZero: return fail(c, BSGPU_ERR_INVALID, "essential_ransac: match_start[0] must be 0");
    case kStartDecreasing: return fail(c, BSGPU_ERR_INVALID, "essential_ransac: match_start must be non-decreasing");
    case kStartBadItem: return fail(c, BSGPU_ERR_INVALID, "essential_ransac: focal lengths must be positive");
    case kStartTooLong: return fail(c, BSGPU_ERR_UNSUPPORTED, "essential_ransac: a set holds more than BSGPU_RANSAC_MAX_MATCHES matches");
    case kStartOk: break;
  }
  if (n_sets == 0) return BSGPU_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n_m = (size_t)match_start[n_sets], ns = (size_t)n_sets;
  StageLayout L;
  const int s_start = L.in(match_start, 4 * (ns + 1)), s_K = L.in(K, 32 * ns), s_p0 = L.in(px_prev, 16 * n_m), s_p1 = L.in(px_cur, 16 * n_m);
  // per-set ints, split below: kRansacOutInts (bsgpu_internal.h)
  const int s_E = L.out(E, 72 * ns), s_oi = L.out(nullptr, 4 * kRansacOutInts * ns), s_mask = L.out(mask, n_m);
  DeviceStage D(L);
  if (!D) return fail(c, BSGPU_ERR_DEVICE, "essential_ransac: out of device memory");
  const hipError_t e = D.run(c->stream, [&] {
    launch_essential_ransac(c->stream, n_sets, D.ptr<int>(s_start), D.ptr<double2>(s_p0), D.ptr<double2>(s_p1), D.ptr<double>(s_K), prob,
                            threshold_px, max_iters, seed, D.ptr<unsigned char>(s_mask), D.ptr<double>(s_E), D.ptr<int>(s_oi));
  });
  if (e != hipSuccess) return fail(c, BSGPU_ERR_DEVICE, "essential_ransac: device error");
  L.scatter();
  const int32_t* oi = L.out_image<int32_t>(s_oi);
  for (size_t k = 0; k < ns; ++k) {
    const int32_t* r = oi + kRansacOutInts * k;
    if (n_inliers) n_inliers[k] = r[0];
    if (n_iters) n_iters[k] = r[1];
    if (best_sample) std::memcpy(best_sample + 5 * k, r + 2, 5 * sizeof(int32_t));
    status[k] = r[7];
  }
  return BSGPU_OK;
} catch (...) { return api_exception(c); }

int bsgpu_absolute_pose_ransac(bsgpu_ctx* c, int32_t n_frames, const int32_t* obs_start, const double* pixels, const double* points,
                               const int32_t* camera, double prob, double threshold_px, int32_t max_iters, uint64_t seed,
                               int32_t truncate_pixels, uint8_t* mask, double* q_out, double* p_out, double* T_cam_world,
                               int32_t* n_inliers, int32_t* n_iters, int32_t* best_sample, int32_t* status) try {
  if (!c) return BSGPU_ERR_INVALID;
  if (n_frames < 0 || !obs_start || !pixels || !points || !camera || !mask || !q_out || !p_out || !status)
    return fail(c, BSGPU_ERR_INVALID, "absolute_pose_ransac: null argument");
  if (!(prob >= 0.0 && prob < 1.0)) return fail(c, BSGPU_ERR_INVALID, "absolute_pose_ransac: prob must lie inside [0, 1)");
  if (!(threshold_px > 0.0) || max_iters <= 0) return fail(c, BSGPU_ERR_INVALID, "absolute_pose_ransac: threshold_px and max_iters must be positive");
  switch (check_start_table(obs_start, n_frames, BSGPU_RANSAC_MAX_MATCHES, [&](int f) { return camera[f] >= 0 && camera[f] < (int)c->cams.size(); })) {
    case kStartNotZero: return fail(c, BSGPU_ERR_INVALID, "absolute_pose_ransac: obs_start[0] must be 0");
    case kStartDecreasing: return fail(c, BSGPU_ERR_INVALID, "absolute_pose_ransac: obs_start must be non-decreasing");
    case kStartBadItem: return fail(c, BSGPU_ERR_INVALID, "absolute_pose_ransac: camera index out of range");
    case kStartTooLong: return fail(c, BSGPU_ERR_UNSUPPORTED, "absolute_pose_ransac: a frame holds more than BSGPU_RANSAC_MAX_MATCHES pairs");
    case kStartOk: break;
  }
  if (n_frames == 0) return BSGPU_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const std::vector<DevCamera> cams = dev_cameras(c);
  const size_t n_obs = (size_t)obs_start[n_frames], nf = (size_t)n_frames;
  StageLayout L;
  const int s_start = L.in(obs_start, 4 * (nf + 1)), s_cam = L.in(camera, 4 * nf), s_cams = L.in(cams.data(), sizeof(DevCamera) * cams.size()),
            s_pix = L.in(pixels, 16 * n_obs), s_pts = L.in(points, 24 * n_obs);
  // per-frame records, split below: kP3pOutDoubles and kP3pOutInts (bsgpu_internal.h)
  const int s_od = L.out(nullptr, 8 * kP3pOutDoubles * nf), s_oi = L.out(nullptr, 4 * kP3pOutInts * nf), s_mask = L.out(mask, n_obs);
  DeviceStage D(L);
  if (!D) return fail(c, BSGPU_ERR_DEVICE, "absolute_pose_ransac: out of device memory");
  const hipError_t e = D.run(c->stream, [&] {
    launch_absolute_pose_ransac(c->stream, n_frames, D.ptr<int>(s_start), D.ptr<double2>(s_pix), D.ptr<double>(s_pts),
                                D.ptr<DevCamera>(s_cams), D.ptr<int>(s_cam), prob, threshold_px, max_iters, seed, truncate_pixels != 0 ? 1 : 0,
                                D.ptr<unsigned char>(s_mask), D.ptr<double>(s_od), D.ptr<int>(s_oi));
  });
  if (e != hipSuccess) return fail(c, BSGPU_ERR_DEVICE, "absolute_pose_ransac: device error");
  L.scatter();
  const double* od = L.out_image<double>(s_od);
  const int32_t* oi = L.out_image<int32_t>(s_oi);
  for (size_t f = 0; f < nf; ++f) {
    const double* r = od + kP3pOutDoubles * f;
    const int32_t* ri = oi + kP3pOutInts * f;
    if (T_cam_world) std::memcpy(T_cam_world + 12 * f, r, 12 * sizeof(double));
    std::memcpy(q_out + 4 * f, r + 12, 4 * sizeof(double));
    std::memcpy(p_out + 3 * f, r + 16, 3 * sizeof(double));
    if (n_inliers) n_inliers[f] = ri[0];
    if (n_iters) n_iters[f] = ri[1];
    if (best_sample) std::memcpy(best_sample + 3 * f, ri + 2, 3 * sizeof(int32_t));
    status[f] = ri[5];
  }
  return BSGPU_OK;
} catch (...) { return api_exception(c); }

int bsgpu_relative_pose_ransac(bsgpu_ctx* c, int32_t n_sets, const int32_t* match_start, const double* px_first, const double* px_last,
                               const int32_t* camera, double prob, double threshold_px, int32_t max_iters, uint64_t seed,
                               int32_t truncate_pixels, double validate_px, double min_inlier_ratio, uint8_t* mask, double* T_last_first,
                               double* q_out, double* p_out, double* points, uint8_t* valid_mask, double* inlier_ratio,
                               int32_t* pair_valid, int32_t* n_inliers, int32_t* n_iters, int32_t* best_sample, int32_t* status) try {
  if (!c) return BSGPU_ERR_INVALID;
  if (n_sets < 0 || !match_start || !px_first || !px_last || !camera || !mask || !q_out || !p_out || !pair_valid || !status)
    return fail(c, BSGPU_ERR_INVALID, "relative_pose_ransac: null argument");
  if (!(prob >= 0.0 && prob < 1.0)) return fail(c, BSGPU_ERR_INVALID, "relative_pose_ransac: prob must lie inside [0, 1)");
  if (!(threshold_px > 0.0) || !(validate_px > 0.0) || max_iters <= 0)
    return fail(c, BSGPU_ERR_INVALID, "relative_pose_ransac: threshold_px, validate_px and max_iters must be positive");
  if (!(min_inlier_ratio >= 0.0 && min_inlier_ratio <= 1.0)) return fail(c, BSGPU_ERR_INVALID, "relative_pose_ransac: min_inlier_ratio must lie inside [0, 1]");
  switch (check_start_table(match_start, n_sets, BSGPU_RANSAC_MAX_MATCHES, [&](int k) { return camera[k] >= 0 && camera[k] < (int)c->cams.size(); })) {
    case kStartNotZero: return fail(c, BSGPU_ERR_INVALID, "relative_pose_ransac: match_start[0] must be 0");
    case kStartDecreasing: return fail(c, BSGPU_ERR_INVALID, "relative_pose_ransac: match_start must be non-decreasing");
    case kStartBadItem: return fail(c, BSGPU_ERR_INVALID, "relative_pose_ransac: camera index out of range");
    case kStartTooLong: return fail(c, BSGPU_ERR_UNSUPPORTED, "relative_pose_ransac: a set holds more than BSGPU_RANSAC_MAX_MATCHES matches");
    case kStartOk: break;
  }
  if (n_sets == 0) return BSGPU_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const std::vector<DevCamera> cams = dev_cameras(c);
  const size_t n_m = (size_t)match_start[n_sets], ns = (size_t)n_sets;
  StageLayout L;
  const int s_start = L.in(match_start, 4 * (ns + 1)), s_cam = L.in(camera, 4 * ns), s_cams = L.in(cams.data(), sizeof(DevCamera) * cams.size()),
            s_p0 = L.in(px_first, 16 * n_m), s_p1 = L.in(px_last, 16 * n_m);
  // per-set records, split below: kRelposeOutDoubles and kRelposeOutInts (bsgpu_internal.h)
  const int s_od = L.out(nullptr, 8 * kRelposeOutDoubles * ns), s_oi = L.out(nullptr, 4 * kRelposeOutInts * ns), s_pts = L.out(points, 24 * n_m),
            s_mask = L.out(mask, n_m), s_valid = L.out(valid_mask, n_m);
  DeviceStage D(L);
  if (!D) return fail(c, BSGPU_ERR_DEVICE, "relative_pose_ransac: out of device memory");
  const hipError_t e = D.run(c->stream, [&] {
    launch_relative_pose_ransac(c->stream, n_sets, D.ptr<int>(s_start), D.ptr<double2>(s_p0), D.ptr<double2>(s_p1),
                                D.ptr<DevCamera>(s_cams), D.ptr<int>(s_cam), prob, threshold_px, max_iters, seed, truncate_pixels != 0 ? 1 : 0,
                                validate_px, min_inlier_ratio, D.ptr<unsigned char>(s_mask), D.ptr<unsigned char>(s_valid),
                                D.ptr<double>(s_pts), D.ptr<double>(s_od), D.ptr<int>(s_oi));
  });
  if (e != hipSuccess) return fail(c, BSGPU_ERR_DEVICE, "relative_pose_ransac: device error");
  L.scatter();
  const double* od = L.out_image<double>(s_od);
  const int32_t* oi = L.out_image<int32_t>(s_oi);
  for (size_t k = 0; k < ns; ++k) {
    const double* r = od + kRelposeOutDoubles * k;
    const int32_t* ri = oi + kRelposeOutInts * k;
    if (T_last_first) std::memcpy(T_last_first + 12 * k, r, 12 * sizeof(double));
    std::memcpy(q_out + 8 * k, r + 12, 8 * sizeof(double));
    std::memcpy(p_out + 6 * k, r + 20, 6 * sizeof(double));
    if (inlier_ratio) inlier_ratio[k] = r[26];
    if (n_inliers) n_inliers[k] = ri[0];
    if (n_iters) n_iters[k] = ri[1];
    if (best_sample) std::memcpy(best_sample + 7 * k, ri + 2, 7 * sizeof(int32_t));
    status[k] = ri[9];
    pair_valid[k] = ri[10];
  }
  return BSGPU_OK;
} catch (...) { return api_exception(c); }

}  // extern "C"
