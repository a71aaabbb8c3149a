// bs_models::reloc::RelocCandidateSearchScanContext — a stand-in for FindRelocCandidates
// (bs_models/src/lib/reloc/reloc_candidate_search_scan_context.cpp:82-208) around ONE bsgpu_scan_context_describe call, ONE
// bsgpu_scan_context_match call and ONE bsgpu_register_scans call:
//   * GetMinDistBetweenSubmaps (:313-330) and the threshold (:96-113): the candidate submaps nearer than submap_distance_threshold_m, in
//     order of that distance (the reference's std::map<double, int>; two submaps at exactly the same distance: both kept here);
//   * GetTimesToAggregate exactly as written (:292-311), its integer num_scans_to_aggregate / 2 included, and AggregateSubmapScan's
//     T_ScanCenter_ScanToAgg = inv(T_Submap_ScanCenter) T_Submap_ScanToAgg (:280) as member_T;
//   * one describe call for the keyframes of the query submap and of every gated candidate submap: every cloud goes to the device once
//     and the query's aggregates are made once, where the reference rebuilds them for every candidate submap (:138-139);
//   * one match call with a set per candidate submap (one SCManager of :120-132): detectLoopClosureID for every query keyframe;
//   * the match pairs in ascending distance (:118, :147, :159; the reference's std::map<float, MatchPair> drops a pair whose float
//     distance repeats, this list keeps it);
//   * AlignSubmapsFromScanMatches (:210-262) for the first max_tries pairs as one bsgpu_register_scans call: ref = the candidate's
//     aggregated scan, target = the query's, T_init = T_Candidate_Query_Init = inv(T_SubmapCandidate_Lidar) inv(T_World_CandidateSubmap)
//     T_World_QuerySubmap T_SubmapQuery_Lidar (:234-238); T_CandidateSubmap_QuerySubmap = T_SubmapCandidate_Lidar T_Candidate_Query
//     inv(T_SubmapQuery_Lidar) (:254-256).  The first converged pair in order is taken (:194-206).
// Not here: the voxel filter of :225-230 stays with the caller (pass filtered clouds; bsgpu_build_registration_maps, one map per
// aggregate, is the library's voxel filter: host/registration_map.h); the shipped matcher of this search is
// matchers/gicp.json, which the device does not have — ICP (bsgpu_register_scans) is what it has.  Nothing is described,
// matched or registered on the host: without the entry points in the back-end, or when a call fails, nothing is matched.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <map>
#include <vector>

#include "scan_matcher.h"

// optional in a back-end: without them nothing is matched
extern "C" int bsgpu_scan_context_describe(int device, int32_t n_scans, const int32_t* scan_start, const double* points, int32_t n_aggregates,
                                           const int32_t* member_start, const int32_t* member_scan, const double* member_T, double lidar_height,
                                           double max_radius, double* desc, double* ring_key, double* sector_key, int32_t* n_binned)
    __attribute__((weak));
extern "C" int bsgpu_scan_context_match(int device, int32_t n_sets, const int32_t* query_start, const double* query_desc,
                                        const int32_t* cand_start, const double* cand_desc, int32_t n_tree_candidates, double search_ratio,
                                        double dist_thres, int32_t* best_cand, double* best_dist, int32_t* best_shift, double* yaw,
                                        double* dist_all, int32_t* shift_all) __attribute__((weak));

namespace bs_models { namespace reloc {

using scan_registration::IcpMatcherParams;
using scan_registration::InvertTransform;
using scan_registration::Mat4;

struct ScanPose {                        // what the search reads of a bs_common::ScanPose
  Mat4 T_REFFRAME_LIDAR = Mat4::Identity();
  Mat4 T_REFFRAME_BASELINK = Mat4::Identity();
  std::vector<double> cloud;             // packed xyz, lidar frame (already filtered: see above)
};
struct Submap {                          // what it reads of a global_mapping::Submap
  Mat4 T_WORLD_SUBMAP = Mat4::Identity();
  std::map<uint64_t, ScanPose> lidar_keyframes;    // by stamp, as LidarKeyframes()
};
struct MatchPair {                       // reloc_candidate_search_scan_context.h's, with what the search found
  int candidate_submap_id = -1, candidate_scan_id = -1, query_scan_id = -1;
  double sc_dist = 0.0;
  int sc_shift = 0;
};
struct Params {                          // config/global_map/reloc_candidate_search_scan_context.json; SCManager's constants (recalled)
  double submap_distance_threshold_m = 5.0;
  double scan_context_dist_thres = 0.3;
  int num_scans_to_aggregate = 20;
  double lidar_height = 2.0, max_radius = 80.0, search_ratio = 0.1;
  int num_candidates_from_tree = 10;
  int max_tries = 4;                     // pairs sent to the matcher in the one call
  IcpMatcherParams matcher;
};
struct RelocResult {
  std::vector<int> matched_indices;                  // FindRelocCandidates' outputs: at most one entry
  std::vector<Mat4> Ts_Candidate_Query;              // T_CandidateSubmap_QuerySubmap
  std::vector<int> gated_submaps;                    // the candidate submaps inside the threshold, nearest first
  std::vector<MatchPair> pairs;                      // ascending Scan Context distance
  std::vector<int32_t> icp_status;                   // of the pairs tried (BSGPU_ICP_*)
  int taken_pair = -1;                               // index into pairs of the one taken
};

class RelocCandidateSearchScanContext {
 public:
  explicit RelocCandidateSearchScanContext(int device = 0, const Params& params = {}) : device_(device), p_(params) {}

  double GetMinDistBetweenSubmaps(const Submap& s1, const Submap& s2) const {
    double min_dist = std::numeric_limits<double>::max();
    for (const auto& k1 : s1.lidar_keyframes) {
      const Mat4 T1 = s1.T_WORLD_SUBMAP * k1.second.T_REFFRAME_BASELINK;
      for (const auto& k2 : s2.lidar_keyframes) {
        const Mat4 T2 = s2.T_WORLD_SUBMAP * k2.second.T_REFFRAME_BASELINK;
        const double dx = T2(0, 3) - T1(0, 3), dy = T2(1, 3) - T1(1, 3), dz = T2(2, 3) - T1(2, 3);
        const double dist = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (dist < min_dist) min_dist = dist;
      }
    }
    return min_dist;
  }

  // the ids (positions in the stamp order) of the keyframes aggregated around center_id, the centre itself left out
  std::vector<int> GetIdsToAggregate(size_t n_keyframes, int center_id) const {
    std::vector<int> ids;
    double curr_id = center_id - p_.num_scans_to_aggregate / 2;
    while (curr_id <= center_id + p_.num_scans_to_aggregate / 2 && curr_id < n_keyframes) {
      if (curr_id >= 0 && curr_id != center_id) ids.push_back((int)curr_id);
      curr_id++;
    }
    return ids;
  }
  std::vector<uint64_t> GetTimesToAggregate(const std::map<uint64_t, ScanPose>& keyframes, int center_id) const {
    std::vector<uint64_t> times;
    for (const int id : GetIdsToAggregate(keyframes.size(), center_id)) {
      auto iter = keyframes.begin();
      std::advance(iter, id);
      times.push_back(iter->first);
    }
    return times;
  }

  RelocResult FindRelocCandidates(const std::vector<const Submap*>& search_submaps, const Submap& query_submap,
                                  size_t ignore_last_n_submaps = 0) const {
    RelocResult out;
    if (search_submaps.size() <= ignore_last_n_submaps) return out;
    std::vector<std::pair<double, int>> gated;
    for (int i = 0; i < (int)(search_submaps.size() - ignore_last_n_submaps); ++i) {
      const double distance = GetMinDistBetweenSubmaps(query_submap, *search_submaps[i]);
      if (distance < p_.submap_distance_threshold_m) gated.emplace_back(distance, i);
    }
    std::stable_sort(gated.begin(), gated.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
    for (const auto& g : gated) out.gated_submaps.push_back(g.second);
    const int nq = (int)query_submap.lidar_keyframes.size();
    if (gated.empty() || nq == 0 || !bsgpu_scan_context_describe || !bsgpu_scan_context_match) return out;

    // ---- one describe call: submap 0 of the list below is the query, then the gated candidates -----------------------------------------
    std::vector<const Submap*> maps(1, &query_submap);
    for (const auto& g : gated) maps.push_back(search_submaps[g.second]);
    std::vector<int32_t> scan_start(1, 0), member_start(1, 0), member_scan, first_scan;
    std::vector<double> points, member_T;
    std::vector<std::vector<const ScanPose*>> poses(maps.size());
    for (size_t s = 0; s < maps.size(); ++s) {
      first_scan.push_back((int32_t)scan_start.size() - 1);
      for (const auto& kf : maps[s]->lidar_keyframes) {
        poses[s].push_back(&kf.second);
        points.insert(points.end(), kf.second.cloud.begin(), kf.second.cloud.end());
        scan_start.push_back((int32_t)(points.size() / 3));
      }
    }
    for (size_t s = 0; s < maps.size(); ++s)
      for (int c = 0; c < (int)poses[s].size(); ++c) {
        AppendMember(first_scan[s] + c, Mat4::Identity(), &member_scan, &member_T);
        const Mat4 T_ScanCenter_Submap = InvertTransform(poses[s][c]->T_REFFRAME_LIDAR);
        for (const int id : GetIdsToAggregate(poses[s].size(), c))
          AppendMember(first_scan[s] + id, T_ScanCenter_Submap * poses[s][id]->T_REFFRAME_LIDAR, &member_scan, &member_T);
        member_start.push_back((int32_t)member_scan.size());
      }
    const int32_t n_agg = (int32_t)member_start.size() - 1;
    points.push_back(0.0);                   // (never read: non-null data() for empty clouds)
    std::vector<double> desc((size_t)n_agg * kDesc);
    if (bsgpu_scan_context_describe(device_, (int32_t)scan_start.size() - 1, scan_start.data(), points.data(), n_agg, member_start.data(),
                                    member_scan.data(), member_T.data(), p_.lidar_height, p_.max_radius, desc.data(), nullptr, nullptr,
                                    nullptr) != BSGPU_OK)
      return out;

    // ---- one match call: a set per candidate submap, the query's descriptors in each ------------------------------------------------------
    const int32_t n_sets = (int32_t)gated.size();
    std::vector<int32_t> query_start(1, 0), cand_start(1, 0);
    std::vector<double> query_desc;
    for (int32_t s = 0; s < n_sets; ++s) {
      query_desc.insert(query_desc.end(), desc.begin(), desc.begin() + (size_t)nq * kDesc);
      query_start.push_back(query_start.back() + nq);
      cand_start.push_back(cand_start.back() + (int32_t)poses[s + 1].size());
    }
    const double* cand_desc = desc.data() + (size_t)nq * kDesc;       // the candidates' aggregates follow the query's, submap by submap
    std::vector<int32_t> best_cand((size_t)n_sets * nq), best_shift((size_t)n_sets * nq);
    std::vector<double> best_dist((size_t)n_sets * nq);
    if (bsgpu_scan_context_match(device_, n_sets, query_start.data(), query_desc.data(), cand_start.data(), cand_desc, p_.num_candidates_from_tree,
                                 p_.search_ratio, p_.scan_context_dist_thres, best_cand.data(), best_dist.data(), best_shift.data(), nullptr,
                                 nullptr, nullptr) != BSGPU_OK)
      return out;
    for (int32_t s = 0; s < n_sets; ++s)
      for (int q = 0; q < nq; ++q) {
        const size_t k = (size_t)s * nq + q;
        if (best_cand[k] == -1) continue;
        MatchPair m;
        m.candidate_submap_id = gated[s].second; m.candidate_scan_id = best_cand[k]; m.query_scan_id = q;
        m.sc_dist = best_dist[k]; m.sc_shift = best_shift[k];
        out.pairs.push_back(m);
      }
    std::stable_sort(out.pairs.begin(), out.pairs.end(), [](const MatchPair& a, const MatchPair& b) { return a.sc_dist < b.sc_dist; });
    if (out.pairs.empty() || !bsgpu_register_scans) return out;

    // ---- one register call: the first max_tries pairs -------------------------------------------------------------------------------------
    const int32_t P = (int32_t)std::min<size_t>(out.pairs.size(), (size_t)std::max(p_.max_tries, 1));
    std::vector<int32_t> rs(1, 0), ts(1, 0);
    std::vector<double> rp, tp, init;
    std::vector<Mat4> T_SubmapCandidate_Lidar(P), T_SubmapQuery_Lidar(P);
    for (int32_t k = 0; k < P; ++k) {
      const MatchPair& m = out.pairs[k];
      const Submap& cand = *search_submaps[m.candidate_submap_id];
      size_t s = 1;
      while (maps[s] != &cand) ++s;
      AggregateSubmapScan(poses[s], m.candidate_scan_id, &rp);
      AggregateSubmapScan(poses[0], m.query_scan_id, &tp);
      rs.push_back((int32_t)(rp.size() / 3)); ts.push_back((int32_t)(tp.size() / 3));
      T_SubmapCandidate_Lidar[k] = poses[s][m.candidate_scan_id]->T_REFFRAME_LIDAR;
      T_SubmapQuery_Lidar[k] = poses[0][m.query_scan_id]->T_REFFRAME_LIDAR;
      const Mat4 T_CandidateSubmap_QuerySubmap_Init = InvertTransform(cand.T_WORLD_SUBMAP) * query_submap.T_WORLD_SUBMAP;
      const Mat4 T_Candidate_Query_Init = InvertTransform(T_SubmapCandidate_Lidar[k]) * T_CandidateSubmap_QuerySubmap_Init * T_SubmapQuery_Lidar[k];
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) init.push_back(T_Candidate_Query_Init(i, j));
    }
    rp.push_back(0.0); tp.push_back(0.0);
    std::vector<double> T(12 * (size_t)P), Trt(12 * (size_t)P);
    out.icp_status.assign(P, -1);
    if (bsgpu_register_scans(device_, P, rs.data(), rp.data(), ts.data(), tp.data(), init.data(), p_.matcher.max_corr, p_.matcher.max_iter,
                             p_.matcher.t_eps, p_.matcher.fit_eps, p_.matcher.rotation_threshold, p_.matcher.rel_mse_eps, T.data(), Trt.data(),
                             nullptr, nullptr, nullptr, out.icp_status.data()) != BSGPU_OK) {
      out.icp_status.assign(P, -1);
      return out;
    }
    for (int32_t k = 0; k < P; ++k) {
      if (out.icp_status[k] == BSGPU_ICP_TOO_FEW_CORRESPONDENCES) continue;      // "Scan matching failed, trying next best candidate"
      Mat4 T_Candidate_Query = Mat4::Identity();                                 // matcher_->ApplyResult(T_Candidate_Query_Init)
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) T_Candidate_Query(i, j) = Trt[12 * (size_t)k + 4 * i + j];
      out.matched_indices.push_back(out.pairs[k].candidate_submap_id);
      out.Ts_Candidate_Query.push_back(T_SubmapCandidate_Lidar[k] * T_Candidate_Query * InvertTransform(T_SubmapQuery_Lidar[k]));
      out.taken_pair = k;
      break;
    }
    return out;
  }

 private:
  static constexpr size_t kDesc = (size_t)BSGPU_SC_RINGS * BSGPU_SC_SECTORS;

  static void AppendMember(int32_t scan, const Mat4& T, std::vector<int32_t>* member_scan, std::vector<double>* member_T) {
    member_scan->push_back(scan);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) member_T->push_back(T(i, j));
  }
  // AggregateSubmapScan (:264-290) as points, for the matcher: the centre's cloud, then its neighbours' in the centre's frame
  void AggregateSubmapScan(const std::vector<const ScanPose*>& keyframes, int keyframe_id, std::vector<double>* cloud) const {
    const ScanPose& centre = *keyframes[keyframe_id];
    cloud->insert(cloud->end(), centre.cloud.begin(), centre.cloud.end());
    const Mat4 T_ScanCenter_Submap = InvertTransform(centre.T_REFFRAME_LIDAR);
    for (const int id : GetIdsToAggregate(keyframes.size(), keyframe_id)) {
      const Mat4 T = T_ScanCenter_Submap * keyframes[id]->T_REFFRAME_LIDAR;
      const std::vector<double>& c = keyframes[id]->cloud;
      for (size_t i = 0; i + 2 < c.size(); i += 3)
        for (int a = 0; a < 3; ++a) cloud->push_back(T(a, 0) * c[i] + T(a, 1) * c[i + 1] + T(a, 2) * c[i + 2] + T(a, 3));
    }
  }

  int device_;
  Params p_;
};

}}  // namespace bs_models::reloc
