// bs_models::reloc::LoopClosureAligner (beam_slam_amd/host/loop_closure_aligner.h): T_Candidate_Query_Init as T_init, the one batched
// bsgpu_register_scans_gicp call, the first converged pair in rank order and the composition of T_CandidateSubmap_QuerySubmap.  Built
// three ways by tests/test_host_loop_closure.py: against libbsgpu.so; with -DLC_STANDIN, where the stand-in below answers the C-ABI
// call pair by pair with gicp.h on one core; and with -DLC_NO_BACKEND, where nothing defines the entry point.
#include <cmath>
#include <cstdio>

#include "../../beam_slam_amd/host/loop_closure_aligner.h"

#ifdef LC_STANDIN
#include "gicp.h"
extern "C" int bsgpu_register_scans_gicp(int, int32_t n_pairs, const int32_t* ref_start, const double* ref_points, const int32_t* tgt_start,
                                         const double* tgt_points, const double* T_init, int32_t k_neighbors, double gicp_epsilon,
                                         double max_corr, int32_t max_iter, double r_eps, double t_eps, int32_t max_inner, double inner_eps,
                                         double grid_cell, double* T_refest_ref, double* T_ref_tgt, double* cost, int32_t* n_corr,
                                         int32_t* n_iters, int32_t* n_inner, int32_t* status, double*, double*) {
  const bsg::GicpParams P{k_neighbors, gicp_epsilon, max_corr, max_iter, r_eps, t_eps, max_inner, inner_eps};
  for (int p = 0; p < n_pairs; ++p)
    if (!bsg::gicp_register_serial(ref_start[p + 1] - ref_start[p], ref_points + 3 * (size_t)ref_start[p], tgt_start[p + 1] - tgt_start[p],
                                   tgt_points + 3 * (size_t)tgt_start[p], T_init ? T_init + 12 * p : nullptr, P, grid_cell,
                                   (double)BSGPU_ICP_MAX_CELLS, T_refest_ref + 12 * p, T_ref_tgt + 12 * p, cost + p, n_corr + p, n_iters + p,
                                   n_inner + p, status + p, nullptr, nullptr))
      return BSGPU_ERR_UNSUPPORTED;
  return BSGPU_OK;
}
#endif

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using namespace bs_models::reloc;

static Mat4 pose(double rx, double ry, double rz, double x, double y, double z) {
  const bs_math::Mat3 R = bs_math::so3Exp({rx, ry, rz});
  Mat4 T = Mat4::Identity();
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T(i, j) = R(i, j);
  T(0, 3) = x; T(1, 3) = y; T(2, 3) = z;
  return T;
}
static void print(const char* tag, int k, const Mat4& T) {
  std::printf("%s %d", tag, k);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) std::printf(" %.17g", T(i, j));
  std::printf("\n");
}

int main() {
#if !defined(LC_STANDIN) && !defined(LC_NO_BACKEND)
  // a strong reference: the header's is weak, and a linker that drops libraries nothing needs would leave the entry point unbound
  CHECK(bsgpu_abi_version() == 1);
#endif
  // a box seen from a lidar of the candidate submap and from one of the query submap; the query submap's world pose is 10 cm and half
  // a degree off, the clouds are noise-free views of one point set
  std::vector<double> world;
  uint64_t lcg = 4711;
  const auto uni = [&] { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992.0 - 0.5; };
  const double box[3] = {20.0, 14.0, 5.0};
  for (int i = 0; i < 1500; ++i) {
    double p[3] = {uni() * box[0], uni() * box[1], uni() * box[2]};
    const int face = i % 6;
    p[face / 2] = (face % 2 ? 0.5 : -0.5) * box[face / 2];
    world.insert(world.end(), p, p + 3);
  }
  const auto seen_from = [&](const Mat4& T_WORLD_LIDAR, size_t count) {
    const Mat4 Ti = InvertTransform(T_WORLD_LIDAR);
    std::vector<double> cloud;
    for (size_t i = 0; i < count; ++i)
      for (int a = 0; a < 3; ++a) cloud.push_back(Ti(a, 0) * world[3 * i] + Ti(a, 1) * world[3 * i + 1] + Ti(a, 2) * world[3 * i + 2] + Ti(a, 3));
    return cloud;
  };
  const Mat4 T_World_Cand = pose(0, 0, 0.3, 1.0, -0.5, 0.1), T_World_Query_true = pose(0.01, -0.02, 0.34, 1.25, -0.65, 0.15);
  const Mat4 T_World_Query_est = T_World_Query_true * pose(0.004, -0.003, 0.008, 0.08, -0.05, 0.03);
  const Mat4 T_Cand_Lidar[2] = {pose(0, 0, 0.1, 0.5, 0.2, 0.0), pose(0, 0.01, -0.05, -0.4, 0.1, 0.05)};
  const Mat4 T_Query_Lidar[2] = {pose(0, 0, -0.08, -0.3, 0.4, 0.0), pose(0.01, 0, 0.02, 0.6, -0.2, 0.02)};
  std::vector<double> cand[2], query[2];
  for (int v = 0; v < 2; ++v) {
    cand[v] = seen_from(T_World_Cand * T_Cand_Lidar[v], 1500);
    query[v] = seen_from(T_World_Query_true * T_Query_Lidar[v], 1500);
  }
  const std::vector<double> few = seen_from(T_World_Query_true * T_Query_Lidar[0], 5);    // fewer points than k: the match fails
  // rank 0 fails in the matcher, rank 1 is the answer, rank 2 would converge too but is never read
  std::vector<AlignCandidate> ranked(3);
  for (int k = 0; k < 3; ++k) {
    const int v = k == 2 ? 1 : 0;
    ranked[k].pair.candidate_submap_id = 7 + k; ranked[k].pair.candidate_scan_id = v; ranked[k].pair.query_scan_id = v;
    ranked[k].scan_candidate = &cand[v];
    ranked[k].scan_query = k == 0 ? &few : &query[v];
    ranked[k].T_SubmapCandidate_Lidar = T_Cand_Lidar[v]; ranked[k].T_SubmapQuery_Lidar = T_Query_Lidar[v];
    ranked[k].T_World_CandidateSubmap = T_World_Cand; ranked[k].T_World_QuerySubmap = T_World_Query_est;
  }
  const LoopClosureAligner aligner;
  const AlignResult res = aligner.AlignSubmapsFromScanMatches(ranked);
  CHECK(res.status.size() == 3 && aligner.AlignSubmapsFromScanMatches({}).taken == -1);
  std::printf("TAKEN %d %d\n", res.taken, res.candidate_submap_id);
  for (int k = 0; k < 3; ++k) {
    std::printf("STATUS %d %d %d %d %d %.17g\n", k, res.status[k], res.n_iters[k], res.n_inner[k], res.n_corr[k], res.cost[k]);
    if (res.status[k] == -1) continue;
    print("TINIT", k, res.T_Candidate_Query_Init[k]);
    print("TCQ", k, res.T_Candidate_Query[k]);
  }
  print("TINITWANT", 1, InvertTransform(T_Cand_Lidar[0]) * InvertTransform(T_World_Cand) * T_World_Query_est * T_Query_Lidar[0]);
  if (res.taken >= 0) {
    print("TOUT", res.taken, res.T_CandidateSubmap_QuerySubmap);
    print("TRUE", res.taken, InvertTransform(T_World_Cand) * T_World_Query_true);
  }
#ifdef LC_NO_BACKEND
  CHECK(res.taken == -1 && res.status[0] == -1 && res.status[1] == -1 && res.status[2] == -1);
#else
  CHECK(res.taken == 1 && res.candidate_submap_id == 8);
  CHECK(res.status[0] == BSGPU_GICP_TOO_FEW_CORRESPONDENCES && GicpConverged(res.status[1]) && GicpConverged(res.status[2]));
#endif
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("HOST LOOP CLOSURE DONE\n");
  return 0;
}
