// bs_models::scan_registration::LoamMatcher — a stand-in for the interface of libbeam's LoamMatcher as the reference's LOAM call sites
// use it (MultiScanLoamRegistration::MatchScans, bs_models/src/lib/scan_registration/multi_scan_registration.cpp:497-531;
// ScanToMapLoamRegistration, scan_to_map_registration.cpp:158-188; RelocRefinementLoamRegistration,
// reloc_refinement_loam_registration.cpp:91-118), over bsgpu_register_scans_loam:
//   * SetRef / SetTarget take the STRONG features of a LoamPointCloud (every shipped matcher file ignores the weak ones), already in
//     the frames the caller matches them in (MatchScans moves the target into the reference's estimated frame first, :506-508);
//   * Match() registers the one pair and returns the reference's bool: converged (MAX_ITERATIONS counts, as there);
//   * GetResult() is T_REFEST_REF (:522), ApplyResult(T) = inv(T_REFEST_REF) T (:523-524), GetCovariance() the 6 x 6 of (p, theta) (:528);
//   * MatchAll() registers one target against many references — a new scan against its num_neighbors predecessors — as ONE call, the
//     target left in its own frame and each pair's T_LidarRefEst_LidarTgt handed over as T_init, so that the device moves the features.
// With device >= 0 the entry point of the back-end is called (without one in the back-end, or when the call fails, nothing matches).
// With device < 0 the same contract runs on one core through the shared header (csrc/loam.h: loam_register_serial, the kernel's
// arithmetic and order of addition), which this header includes only when LOAM_MATCHER_WITH_HEADER is defined: that path needs the
// csrc directory and the HIP headers on the include path.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/bsgpu.h"
#include "bs_common.h"
#ifdef LOAM_MATCHER_WITH_HEADER
#include "../csrc/loam.h"
#endif

// optional in a back-end: without it nothing is matched on a device
extern "C" int bsgpu_register_scans_loam(int device, int32_t n_pairs, const int32_t* ref_edge_start, const double* ref_edges,
                                         const int32_t* ref_surf_start, const double* ref_surfs, const int32_t* tgt_edge_start,
                                         const double* tgt_edges, const int32_t* tgt_surf_start, const double* tgt_surfs, const double* T_init,
                                         double max_corr, int32_t min_measurements, int32_t max_outer, double conv_translation_m,
                                         double conv_rotation_deg, const bsgpu_options* inner, int32_t loss_kind, double loss_a, double grid_cell,
                                         double* T_refest_ref, double* T_ref_tgt, double* cov, double* cost, int32_t* n_edge, int32_t* n_surf,
                                         int32_t* n_iters, int32_t* n_inner, int32_t* status) __attribute__((weak));

namespace bs_models { namespace scan_registration {

using LoamMat4 = bs_math::Mat<4, 4>;
using LoamCov6 = bs_math::Mat<6, 6>;

struct LoamPointCloud {                  // what the matcher reads of a LoamPointCloud: edges.strong, surfaces.strong, packed xyz
  std::vector<double> edges, surfaces;
};

struct LoamMatcherParams {               // config/matchers/loam_vlp16.json, config/optimization/ceres_config.json; grid_cell: the library's own
  double max_correspondence_distance = 0.5;
  int min_number_measurements = 30;
  bool iterate_correspondences = true;
  int max_correspondence_iterations = 10;
  double convergence_criteria_translation_m = 1e-3, convergence_criteria_rotation_deg = 0.1;
  int max_num_iterations = 50;
  double function_tolerance = 1e-8, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  int loss_kind = BSGPU_LOSS_HUBER;
  double loss_scaling = 1.0;
  double grid_cell = 0.5;
};

struct LoamMatch {
  bool converged = false;
  int32_t status = -1, n_edge = 0, n_surf = 0, n_iters = 0, n_inner = 0;      // status -1: no back-end, or the call failed
  double cost = 0.0;
  LoamMat4 T_RefEst_Ref = LoamMat4::Identity(), T_Ref_Tgt = LoamMat4::Identity();
  LoamCov6 covariance;
};

inline bool LoamConverged(int32_t status) { return status == BSGPU_LOAM_MAX_ITERATIONS || status == BSGPU_LOAM_TRANSFORM; }

class LoamMatcher {
 public:
  explicit LoamMatcher(int device = 0, const LoamMatcherParams& params = {}) : device_(device), m_(params) {}

  void SetRef(const LoamPointCloud* ref) { ref_ = ref; }
  void SetTarget(const LoamPointCloud* target) { tgt_ = target; }
  bool Match() {
    last_ = ref_ && tgt_ ? MatchAll({ref_}, *tgt_, {LoamMat4::Identity()})[0] : LoamMatch();
    return last_.converged;
  }
  const LoamMat4& GetResult() const { return last_.T_RefEst_Ref; }
  const LoamCov6& GetCovariance() const { return last_.covariance; }
  const LoamMatch& last() const { return last_; }
  LoamMat4 ApplyResult(const LoamMat4& T_RefEst_Tgt) const {
    const LoamMat4& T = last_.T_RefEst_Ref;
    LoamMat4 inv = LoamMat4::Identity();
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) inv(i, j) = T(j, i);
      inv(i, 3) = -(T(0, i) * T(0, 3) + T(1, i) * T(1, 3) + T(2, i) * T(2, 3));
    }
    return inv * T_RefEst_Tgt;
  }

  // One target against refs.size() references in one call; T_init[k] (T_LidarRefEst_LidarTgt of pair k) moves the target's features
  // into reference k's estimated frame first.  Result k: T_RefEst_Ref, and T_Ref_Tgt = inv(T_RefEst_Ref) T_init[k] = T_LIDARREF_LIDARTGT.
  std::vector<LoamMatch> MatchAll(const std::vector<const LoamPointCloud*>& refs, const LoamPointCloud& tgt, const std::vector<LoamMat4>& T_init) const {
    const int32_t P = (int32_t)refs.size();
    std::vector<LoamMatch> out((size_t)P);
    if (P == 0 || T_init.size() != refs.size()) return out;
    std::vector<int32_t> res(1, 0), rss(1, 0), tes(1, 0), tss(1, 0);
    std::vector<double> re, rs, te, ts, init;
    for (int32_t k = 0; k < P; ++k) {
      re.insert(re.end(), refs[k]->edges.begin(), refs[k]->edges.end());
      rs.insert(rs.end(), refs[k]->surfaces.begin(), refs[k]->surfaces.end());
      te.insert(te.end(), tgt.edges.begin(), tgt.edges.end());
      ts.insert(ts.end(), tgt.surfaces.begin(), tgt.surfaces.end());
      res.push_back((int32_t)(re.size() / 3)); rss.push_back((int32_t)(rs.size() / 3));
      tes.push_back((int32_t)(te.size() / 3)); tss.push_back((int32_t)(ts.size() / 3));
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) init.push_back(T_init[k](i, j));
    }
    re.push_back(0.0); rs.push_back(0.0); te.push_back(0.0); ts.push_back(0.0);    // (never read: non-null data() for empty clouds)
    bsgpu_options o = InnerOptions();
    const int32_t max_outer = m_.iterate_correspondences ? m_.max_correspondence_iterations : 1;
    std::vector<double> T(12 * (size_t)P), Trt(12 * (size_t)P), cov(36 * (size_t)P), cost((size_t)P);
    std::vector<int32_t> ne(P), ns(P), ni(P), nn(P), st(P, -1);
    if (device_ >= 0) {
      if (!bsgpu_register_scans_loam ||
          bsgpu_register_scans_loam(device_, P, res.data(), re.data(), rss.data(), rs.data(), tes.data(), te.data(), tss.data(), ts.data(), init.data(),
                                    m_.max_correspondence_distance, m_.min_number_measurements, max_outer, m_.convergence_criteria_translation_m,
                                    m_.convergence_criteria_rotation_deg, &o, m_.loss_kind, m_.loss_scaling, m_.grid_cell, T.data(), Trt.data(),
                                    cov.data(), cost.data(), ne.data(), ns.data(), ni.data(), nn.data(), st.data()) != BSGPU_OK)
        return out;
    } else {
#ifdef LOAM_MATCHER_WITH_HEADER
      bsg::LoamParams Q;
      Q.mc2 = m_.max_correspondence_distance * m_.max_correspondence_distance; Q.min_measurements = m_.min_number_measurements; Q.max_outer = max_outer;
      Q.conv_translation = m_.convergence_criteria_translation_m; Q.cos_rotation = bsg::loam_cos_bound(m_.convergence_criteria_rotation_deg);
      Q.loss_kind = m_.loss_kind; Q.loss_a = m_.loss_scaling; Q.inner = o;
      for (int32_t k = 0; k < P; ++k) {
        bsg::LoamResult r;
        if (!bsg::loam_register_serial(res[k + 1] - res[k], re.data() + 3 * (size_t)res[k], rss[k + 1] - rss[k], rs.data() + 3 * (size_t)rss[k],
                                       tes[k + 1] - tes[k], te.data() + 3 * (size_t)tes[k], tss[k + 1] - tss[k], ts.data() + 3 * (size_t)tss[k],
                                       init.data() + 12 * (size_t)k, Q, m_.grid_cell, (double)BSGPU_ICP_MAX_CELLS, &T[12 * (size_t)k], &Trt[12 * (size_t)k], &r))
          return out;
        for (int i = 0; i < 36; ++i) cov[36 * (size_t)k + i] = r.cov[i];
        cost[k] = r.cost; ne[k] = r.n_edge; ns[k] = r.n_surf; ni[k] = r.n_iters; nn[k] = r.n_inner; st[k] = r.status;
      }
#else
      return out;
#endif
    }
    for (int32_t k = 0; k < P; ++k) {
      LoamMatch& m = out[(size_t)k];
      m.status = st[k]; m.converged = LoamConverged(st[k]);
      m.n_edge = ne[k]; m.n_surf = ns[k]; m.n_iters = ni[k]; m.n_inner = nn[k]; m.cost = cost[k];
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) { m.T_RefEst_Ref(i, j) = T[12 * (size_t)k + 4 * i + j]; m.T_Ref_Tgt(i, j) = Trt[12 * (size_t)k + 4 * i + j]; }
      for (int i = 0; i < 36; ++i) m.covariance.a[i] = cov[36 * (size_t)k + i];
    }
    return out;
  }

 private:
  // Ceres' defaults (bsgpu_options_default) under what ceres_config.json sets
  bsgpu_options InnerOptions() const {
    bsgpu_options o = {};
    o.jacobi_scaling = 1; o.max_num_consecutive_invalid_steps = 5; o.max_solver_time_in_seconds = 1e9;
    o.initial_trust_region_radius = 1e4; o.max_trust_region_radius = 1e16; o.min_trust_region_radius = 1e-32;
    o.min_relative_decrease = 1e-3; o.min_lm_diagonal = 1e-6; o.max_lm_diagonal = 1e32;
    o.trust_region_strategy_type = BSGPU_TR_LEVENBERG_MARQUARDT;
    o.max_num_iterations = m_.max_num_iterations; o.function_tolerance = m_.function_tolerance;
    o.gradient_tolerance = m_.gradient_tolerance; o.parameter_tolerance = m_.parameter_tolerance;
    return o;
  }

  int device_;
  LoamMatcherParams m_;
  const LoamPointCloud *ref_ = nullptr, *tgt_ = nullptr;
  LoamMatch last_;
};

}}  // namespace bs_models::scan_registration
