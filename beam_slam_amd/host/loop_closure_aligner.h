// bs_models::reloc::LoopClosureAligner — a stand-in for RelocCandidateSearchScanContext::AlignSubmapsFromScanMatches
// (bs_models/src/lib/reloc/reloc_candidate_search_scan_context.cpp:210-262) and the try-next loop around it (:157-207) in the shipped
// matcher configuration (config/global_map/reloc_candidate_search_scan_context.json:6 -> matchers/gicp.json), around ONE
// bsgpu_register_scans_gicp call:
//   * input: the ranked match pairs of reloc_candidate_search.h (RelocResult::pairs, ascending Scan Context distance), per pair the two
//     aggregated scans — ALREADY filtered: the voxel filter of :225-230 and the matcher's own res stay with the caller, who can have
//     them from bsgpu_build_registration_maps (one map per aggregate, the scans under their T_ScanCenter_Scan) — and the four
//     transforms of :194-197;
//   * T_Candidate_Query_Init = inv(T_SubmapCandidate_Lidar) inv(T_World_CandidateSubmap) T_World_QuerySubmap T_SubmapQuery_Lidar
//     (:234-238) goes to the device as T_init: ref = the candidate's scan, target = the query's (:243-244);
//   * T_Candidate_Query = matcher_->ApplyResult(T_Candidate_Query_Init) (:246-247) is the call's T_ref_tgt;
//   * the first pair in rank order whose status is converged gives T_CandidateSubmap_QuerySubmap = T_SubmapCandidate_Lidar
//     T_Candidate_Query inv(T_SubmapQuery_Lidar) (:254-257): the answer of the reference's loop, which tries the next pair when a
//     match fails (:198-206).  All pairs are registered in the one call; the later ones are simply not read.
// Nothing is registered on the host: without the entry point in the back-end, or when the call fails, nothing is aligned.
#pragma once
#include <cstdint>
#include <vector>

#include "reloc_candidate_search.h"

// optional in a back-end: without it nothing is aligned
extern "C" int bsgpu_register_scans_gicp(int device, int32_t n_pairs, const int32_t* ref_start, const double* ref_points, const int32_t* tgt_start,
                                         const double* tgt_points, const double* T_init, int32_t k_neighbors, double gicp_epsilon,
                                         double max_corr, int32_t max_iter, double r_eps, double t_eps, int32_t max_inner, double inner_eps,
                                         double grid_cell, double* T_refest_ref, double* T_ref_tgt, double* cost, int32_t* n_corr,
                                         int32_t* n_iters, int32_t* n_inner, int32_t* status, double* ref_cov, double* tgt_cov)
    __attribute__((weak));

namespace bs_models { namespace reloc {

struct GicpMatcherParams {               // config/matchers/gicp.json; PCL's constructor (recalled); the library's own last two
  int k_neighbors = 10;
  double gicp_epsilon = 1e-3, max_corr = 5.0;
  int max_iter = 100;
  double r_eps = 1e-8, t_eps = 5e-4;
  int max_inner = 20;
  double inner_eps = 1e-10, grid_cell = 0.5;
};

struct AlignCandidate {                  // the arguments of AlignSubmapsFromScanMatches for one match pair
  MatchPair pair;
  const std::vector<double>* scan_candidate = nullptr;   // packed xyz, candidate lidar frame, aggregated and filtered
  const std::vector<double>* scan_query = nullptr;       // the same of the query
  Mat4 T_SubmapCandidate_Lidar = Mat4::Identity(), T_SubmapQuery_Lidar = Mat4::Identity();
  Mat4 T_World_CandidateSubmap = Mat4::Identity(), T_World_QuerySubmap = Mat4::Identity();
};

struct AlignResult {
  int taken = -1;                                        // index into the ranked pairs of the one taken; -1: none
  int candidate_submap_id = -1;                          // FindRelocCandidates' matched_indices entry
  Mat4 T_CandidateSubmap_QuerySubmap = Mat4::Identity();
  std::vector<int32_t> status, n_iters, n_inner, n_corr; // per pair; status -1: no back-end, or the call failed
  std::vector<double> cost;
  std::vector<Mat4> T_Candidate_Query_Init, T_Candidate_Query;
};

inline bool GicpConverged(int32_t status) { return status == BSGPU_GICP_MAX_ITERATIONS || status == BSGPU_GICP_TRANSFORM; }

class LoopClosureAligner {
 public:
  explicit LoopClosureAligner(int device = 0, const GicpMatcherParams& matcher = {}) : device_(device), m_(matcher) {}

  AlignResult AlignSubmapsFromScanMatches(const std::vector<AlignCandidate>& ranked) const {
    AlignResult out;
    const int32_t P = (int32_t)ranked.size();
    out.status.assign(P, -1); out.n_iters.assign(P, 0); out.n_inner.assign(P, 0); out.n_corr.assign(P, 0); out.cost.assign(P, 0.0);
    out.T_Candidate_Query_Init.assign(P, Mat4::Identity()); out.T_Candidate_Query.assign(P, Mat4::Identity());
    if (P == 0 || !bsgpu_register_scans_gicp) return out;
    std::vector<int32_t> rs(1, 0), ts(1, 0);
    std::vector<double> rp, tp, init;
    for (int32_t k = 0; k < P; ++k) {
      const AlignCandidate& c = ranked[k];
      rp.insert(rp.end(), c.scan_candidate->begin(), c.scan_candidate->end());
      tp.insert(tp.end(), c.scan_query->begin(), c.scan_query->end());
      rs.push_back((int32_t)(rp.size() / 3)); ts.push_back((int32_t)(tp.size() / 3));
      const Mat4 T_CandidateSubmap_QuerySubmap_Init = InvertTransform(c.T_World_CandidateSubmap) * c.T_World_QuerySubmap;
      out.T_Candidate_Query_Init[k] = InvertTransform(c.T_SubmapCandidate_Lidar) * T_CandidateSubmap_QuerySubmap_Init * c.T_SubmapQuery_Lidar;
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) init.push_back(out.T_Candidate_Query_Init[k](i, j));
    }
    rp.push_back(0.0); tp.push_back(0.0);    // (never read: non-null data() for empty clouds)
    std::vector<double> T(12 * (size_t)P), Trt(12 * (size_t)P);
    std::vector<int32_t> st(P, -1);
    if (bsgpu_register_scans_gicp(device_, P, rs.data(), rp.data(), ts.data(), tp.data(), init.data(), m_.k_neighbors, m_.gicp_epsilon, m_.max_corr,
                                  m_.max_iter, m_.r_eps, m_.t_eps, m_.max_inner, m_.inner_eps, m_.grid_cell, T.data(), Trt.data(), out.cost.data(),
                                  out.n_corr.data(), out.n_iters.data(), out.n_inner.data(), st.data(), nullptr, nullptr) != BSGPU_OK)
      return out;
    out.status = st;
    for (int32_t k = 0; k < P; ++k)
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) out.T_Candidate_Query[k](i, j) = Trt[12 * (size_t)k + 4 * i + j];
    for (int32_t k = 0; k < P; ++k) {
      if (!GicpConverged(out.status[k])) continue;       // "Scan matching failed, trying next best candidate"
      out.taken = k;
      out.candidate_submap_id = ranked[k].pair.candidate_submap_id;
      out.T_CandidateSubmap_QuerySubmap = ranked[k].T_SubmapCandidate_Lidar * out.T_Candidate_Query[k] * InvertTransform(ranked[k].T_SubmapQuery_Lidar);
      break;
    }
    return out;
  }

 private:
  int device_;
  GicpMatcherParams m_;
};

}}  // namespace bs_models::reloc
