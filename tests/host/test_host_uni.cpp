// bs_constraints::Unicycle3DStateKinematicConstraint in a GpuGraph: a chain of unicycle states (p, q, v, w, a) with a prior on the first
// state and a noisy pose measurement of every later one, the unicycle part built like bs_models::Unicycle3D builds it.  Built by tests/test_host_unicycle.py:
//   "pack"  (any back-end): prints each constraint's packed BSGPU_F_UNICYCLE row (block indices in the order the variables were added,
//           consts) and the constraint's inputs, for the test to check against the Python layout;
//   "solve" (libbsgpu.so): optimises the graph and prints every variable's value and the final cost.
#include <cstdio>
#include <cmath>
#include <cstring>
#include <map>
#include <random>

#include "../../beam_slam_amd/host/fixed_lag_smoother.h"

using namespace bs_math;

int main(int argc, char** argv) {
  const bool solve = argc > 1 && std::strcmp(argv[1], "solve") == 0;
  std::mt19937 rng(3);
  std::normal_distribution<double> N(0.0, 1.0);
  const int n = 12;
  bs_optimizers::GpuGraph graph;
  std::vector<fuse_core::Variable::SharedPtr> vars;   // in the order added: q, p, v, w, a per state
  std::map<fuse_core::UUID, int32_t> index;
  std::vector<fuse_variables::Position3DStamped::SharedPtr> ps;
  std::vector<fuse_variables::Orientation3DStamped::SharedPtr> qs;
  std::vector<fuse_variables::VelocityLinear3DStamped::SharedPtr> vs;
  std::vector<fuse_variables::VelocityAngular3DStamped::SharedPtr> ws;
  std::vector<fuse_variables::AccelerationLinear3DStamped::SharedPtr> as;
  for (int k = 0; k < n; ++k) {
    const fuse_core::Time t(10.0 + 0.1 * k + 0.013 * (k % 3));
    auto q = fuse_variables::Orientation3DStamped::make_shared(t);
    auto p = fuse_variables::Position3DStamped::make_shared(t);
    auto v = fuse_variables::VelocityLinear3DStamped::make_shared(t);
    auto w = fuse_variables::VelocityAngular3DStamped::make_shared(t);
    auto a = fuse_variables::AccelerationLinear3DStamped::make_shared(t);
    const double yaw = 0.3 * k + 0.02 * N(rng), pitch = 0.05 * N(rng), roll = 0.05 * N(rng);
    const double cy = std::cos(yaw / 2), sy = std::sin(yaw / 2), cp = std::cos(pitch / 2), sp = std::sin(pitch / 2), cr = std::cos(roll / 2), sr = std::sin(roll / 2);
    q->data()[0] = cr * cp * cy + sr * sp * sy; q->data()[1] = sr * cp * cy - cr * sp * sy;
    q->data()[2] = cr * sp * cy + sr * cp * sy; q->data()[3] = cr * cp * sy - sr * sp * cy;
    for (int i = 0; i < 3; ++i) {
      p->data()[i] = (i == 0 ? 0.2 * k : i == 1 ? 0.03 * k * k : 0.01 * k) + 0.02 * N(rng);
      v->data()[i] = (i == 0 ? 2.0 : 0.0) + 0.05 * N(rng);
      w->data()[i] = (i == 2 ? 3.0 : 0.0) + 0.05 * N(rng);
      a->data()[i] = 0.1 * N(rng);
    }
    for (fuse_core::Variable::SharedPtr x : {fuse_core::Variable::SharedPtr(q), fuse_core::Variable::SharedPtr(p), fuse_core::Variable::SharedPtr(v),
                                             fuse_core::Variable::SharedPtr(w), fuse_core::Variable::SharedPtr(a)}) {
      index[x->uuid()] = (int32_t)vars.size();
      vars.push_back(x);
      graph.addVariable(x);
    }
    qs.push_back(q); ps.push_back(p); vs.push_back(v); ws.push_back(w); as.push_back(a);
  }
  Mat<15, 15> cov = Mat<15, 15>::Identity();
  for (int i = 0; i < 15; ++i) for (int j = 0; j < 15; ++j) cov(i, j) = (i == j ? 1e-3 * (1 + i % 5) : 2e-5 * std::cos(1.0 + i * j));
  Mat<6, 6> cov6 = Mat<6, 6>::Identity(); for (int i = 0; i < 6; ++i) cov6(i, i) = 1e-4;
  Mat<3, 3> cov3 = Mat<3, 3>::Identity(); for (int i = 0; i < 3; ++i) cov3(i, i) = 1e-2;
  const double* q0 = qs[0]->data(); const double* p0 = ps[0]->data();
  graph.addConstraint(std::make_shared<fuse_constraints::AbsolutePose3DStampedConstraint>(
      "prior", *ps[0], *qs[0], bs_constraints::Vector7d{p0[0], p0[1], p0[2], q0[0], q0[1], q0[2], q0[3]}, cov6));
  for (const fuse_core::Variable* x : {(const fuse_core::Variable*)vs[0].get(), (const fuse_core::Variable*)ws[0].get(), (const fuse_core::Variable*)as[0].get()})
    graph.addConstraint(std::make_shared<fuse_constraints::AbsoluteVec3Constraint>("fuse_constraints::AbsoluteVec3Constraint", "prior", *x,
                                                                                    Vec3{x->data()[0], x->data()[1], x->data()[2]}, cov3));
  // a noisy pose measurement of every later state (a GPS-like source): the graph is over-determined
  Mat<6, 6> covm = Mat<6, 6>::Identity(); for (int i = 0; i < 6; ++i) covm(i, i) = 1e-2;
  for (int k = 1; k < n; ++k) {
    const double* q = qs[k]->data(); const double* p = ps[k]->data();
    bs_constraints::Vector7d m{p[0] + 0.05 * N(rng), p[1] + 0.05 * N(rng), p[2] + 0.05 * N(rng), q[0] + 0.01 * N(rng), q[1] + 0.01 * N(rng), q[2], q[3]};
    const double nq = std::sqrt(m[3] * m[3] + m[4] * m[4] + m[5] * m[5] + m[6] * m[6]);
    for (int i = 3; i < 7; ++i) m[i] /= nq;
    graph.addConstraint(std::make_shared<fuse_constraints::AbsolutePose3DStampedConstraint>("gps", *ps[k], *qs[k], m, covm));
    std::printf("MEAS %d", k); for (int i = 0; i < 7; ++i) std::printf(" %.17g", m[i]); std::printf("\n");
  }
  fuse_core::BlockOf block_of([&](const fuse_core::UUID& u) { return index.at(u); });
  for (int k = 0; k + 1 < n; ++k) {
    auto c = std::make_shared<bs_constraints::Unicycle3DStateKinematicConstraint>("bs_models::Unicycle3D", *ps[k], *qs[k], *vs[k], *ws[k], *as[k],
                                                                                  *ps[k + 1], *qs[k + 1], *vs[k + 1], *ws[k + 1], *as[k + 1], cov);
    graph.addConstraint(c);
    if (!solve) {
      fuse_core::FactorTables t;
      c->pack(block_of, t);
      std::printf("IDX %d", k);
      for (int32_t b : t.idx[BSGPU_F_UNICYCLE]) std::printf(" %d", b);
      std::printf("\nCONST %d", k);
      for (double v : t.consts[BSGPU_F_UNICYCLE]) std::printf(" %.17g", v);
      std::printf("\nSTAMPS %d %lld %lld\nLOSS %d %d %zu\n", k, (long long)ps[k]->stamp().ns, (long long)ps[k + 1]->stamp().ns, k,
                  t.loss_kind[BSGPU_F_UNICYCLE].empty() ? -1 : t.loss_kind[BSGPU_F_UNICYCLE][0], t.idx[BSGPU_F_UNICYCLE].size());
    }
  }
  for (int i = 0; i < 15; ++i) { std::printf("COV %d", i); for (int j = 0; j < 15; ++j) std::printf(" %.17g", cov(i, j)); std::printf("\n"); }
  if (solve) {
    for (size_t i = 0; i < vars.size(); ++i) { std::printf("X0 %zu", i); for (size_t j = 0; j < vars[i]->size(); ++j) std::printf(" %.17g", vars[i]->data()[j]); std::printf("\n"); }
    auto summary = graph.optimize();
    if (!summary.IsSolutionUsable()) { std::printf("solve not usable\n"); return 1; }
    for (size_t i = 0; i < vars.size(); ++i) {
      const fuse_core::Variable& v = graph.getVariable(vars[i]->uuid());
      std::printf("X %zu", i); for (size_t j = 0; j < v.size(); ++j) std::printf(" %.17g", v.data()[j]); std::printf("\n");
    }
    std::printf("final cost %.17g\n", summary.final_cost);
  }
  std::printf("HOST UNICYCLE DONE\n");
  return 0;
}
