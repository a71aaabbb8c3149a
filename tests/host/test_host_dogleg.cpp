// GpuGraph::optimize / optimizeFor hand ceres_compat::SolverOptions::trust_region_strategy_type and dogleg_type to the back-end, and a
// SUBSPACE_DOGLEG the back-end refuses is thrown through check().  Built by tests/test_host_dogleg.py against the CPU oracle
// (tests/host/oracle_backend.h) with bsgpu_solve pointed at a recording wrapper: the oracle's own solve ignores the strategy.
#include "oracle_backend.h"
#undef bsgpu_solve
#define bsgpu_solve recording_solve
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../beam_slam_amd/host/fixed_lag_smoother.h"

extern "C" int bso_solve(bsgpu_ctx* ctx, const bsgpu_options* o, bsgpu_summary* s);
static std::vector<int32_t> g_seen;
extern "C" int recording_solve(bsgpu_ctx* ctx, const bsgpu_options* o, bsgpu_summary* s) {
  g_seen.push_back(o->trust_region_strategy_type);
  if (o->trust_region_strategy_type == BSGPU_TR_SUBSPACE_DOGLEG) return BSGPU_ERR_UNSUPPORTED;   // (what libbsgpu answers)
  return bso_solve(ctx, o, s);
}

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("  CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

int main() {
  bs_common::ImuState IS1(fuse_core::Time(1.0), {0.952, 0.038, -0.189, 0.239}, {1.5, -3.0, 1.0}, {1.5, -3.0, 1.0}, {4e-5, 5e-5, 6e-5}, {1e-5, 2e-5, 3e-5});
  bs_optimizers::GpuGraph graph;
  graph.addVariable(IS1.Orientation().clone());
  graph.addVariable(IS1.Position().clone());
  graph.addConstraint(std::make_shared<fuse_constraints::AbsolutePose3DStampedConstraint>("test", IS1.Position(), IS1.Orientation(),
                                                                                          bs_constraints::Vector7d{0, 0, 0, 1, 0, 0, 0},
                                                                                          bs_math::Mat<6, 6>::Identity()));
  ceres_compat::SolverOptions o;
  CHECK(o.trust_region_strategy_type == ceres_compat::LEVENBERG_MARQUARDT && o.dogleg_type == ceres_compat::TRADITIONAL_DOGLEG);
  CHECK(graph.optimize(o).IsSolutionUsable());
  o.trust_region_strategy_type = ceres_compat::DOGLEG;
  CHECK(graph.optimize(o).IsSolutionUsable());
  CHECK(graph.optimizeFor(1.0, o).IsSolutionUsable());
  o.dogleg_type = ceres_compat::SUBSPACE_DOGLEG;
  bool threw = false;
  try { graph.optimize(o); } catch (const std::runtime_error&) { threw = true; }
  CHECK(threw);
  o.trust_region_strategy_type = ceres_compat::LEVENBERG_MARQUARDT;   // (dogleg_type means nothing to LM)
  CHECK(graph.optimize(o).IsSolutionUsable());
  const std::vector<int32_t> want = {BSGPU_TR_LEVENBERG_MARQUARDT, BSGPU_TR_DOGLEG, BSGPU_TR_DOGLEG, BSGPU_TR_SUBSPACE_DOGLEG, BSGPU_TR_LEVENBERG_MARQUARDT};
  CHECK(g_seen == want);
  for (int32_t v : g_seen) std::printf("%d ", v);
  std::printf("\n%s\n", g_fail ? "HOST DOGLEG TESTS FAILED" : "ALL HOST DOGLEG TESTS PASSED");
  return g_fail ? 1 : 0;
}
