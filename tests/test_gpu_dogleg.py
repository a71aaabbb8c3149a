"""trust_region_strategy_type = DOGLEG (Ceres TRADITIONAL_DOGLEG) on the MI355X against the numpy restatement tests/dogleg_ref.py, driven by
the CPU oracle's residuals and Jacobians: the same accept / reject / invalid sequence, per-iteration cost and radius within 1e-9, the model
cost change within 1e-8, final values within 1e-7; the factorisation count; what DOGLEG leaves untouched (LM after DOGLEG, default
options); every refusal; a batch that mixes both strategies."""
import os

import numpy as np
import pytest

import dogleg_ref
import helpers
from beam_slam_amd import capi, synthetic
from beam_slam_amd.problem import Problem
from beam_slam_amd.synthetic import quat_from_aa, quat_mul

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
    return Problem.from_arrays(np.load(os.path.join(GOLDEN, name + ".npz")))


def _marg_window(oracle_cls):
    """mixed_problem with its first state marginalised into ONE dense prior (the oracle's marginalisation at the start values)."""
    pr = helpers.mixed_problem(seed=3, n_state=5, n_lm=16, consistent=True)
    o = oracle_cls(threads=1)
    pr.load(o)
    marg = [int(b) for b in pr.meta["states"][0]]
    kept, A, b, xbar = o.marginalize(marg, pr.size)
    out = pr.marginalized(marg, kept, A, b, xbar, values=pr.values)
    v = out.values.copy()
    rng = np.random.default_rng(3)
    for b_ in pr.meta["states"][2:, 1]:
        v[out.offset[b_]:out.offset[b_] + 3] += rng.normal(0, 0.05, 3)
    out.values = v
    return out


def _perturbed(oracle_cls):
    """every state rotated and moved away from a consistent window's optimum, solved from a large initial radius: a run of rejected steps
    that reuse their Gauss-Newton step"""
    pr = helpers.mixed_problem(seed=1, n_state=5, n_lm=30, consistent=True)
    rng = np.random.default_rng(1)
    v = pr.values.copy()
    for b in range(pr.n_blocks):
        if pr.is_const[b]:
            continue
        o, n = pr.offset[b], pr.size[b]
        if pr.manifold[b] == capi.MANIFOLD_QUAT_RIGHT:
            v[o:o + 4] = quat_mul(v[o:o + 4], quat_from_aa(rng.normal(0, 0.3, 3)))
        else:
            v[o:o + n] += rng.normal(0, 0.3, n)
    pr.values = v
    return pr


CASES = {
    "all_types_seed0": lambda oc: _golden("all_types_seed0"),
    "all_types_seed7_const": lambda oc: _golden("all_types_seed7_const"),
    "lio_window_12kf": lambda oc: _golden("lio_window_12kf"),
    "mixed_problem": lambda oc: helpers.mixed_problem(seed=0, n_state=5, n_lm=30, consistent=True),
    "pose_graph_40": lambda oc: _golden("pose_graph_40"),
    "dense_prior": _marg_window,
    "perturbed_large_radius": _perturbed,   # (radius 1e8)
}


def _dogleg(solver, radius=None):
    o = solver.options_default()
    o.trust_region_strategy_type = capi.TR_DOGLEG
    if radius is not None:
        o.initial_trust_region_radius = radius
    return o


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# (the device's and the oracle's residuals and Jacobians agree to ~1e-9 — tests/test_gpu_parity.py — and a start far from the optimum
# amplifies that along its rejected steps: the perturbed run is held to 1e-8)
TOL = {"perturbed_large_radius": 1e-8}


@pytest.mark.parametrize("name", list(CASES))
def test_dogleg_matches_restatement(gpu_solver_cls, oracle_cls, name):
    pr = CASES[name](oracle_cls)
    radius = 1e8 if name == "perturbed_large_radius" else None
    g = gpu_solver_cls(0)
    pr.load(g)
    s = g.solve(_dogleg(g, radius))
    its = g.iterations()
    o = oracle_cls(threads=1)
    ref = dogleg_ref.solve(pr, o, _dogleg(o, radius), fixed_cost=s.fixed_cost)
    rr = ref["records"]
    assert [(i.step_is_valid, i.step_is_successful) for i in its] == [(r["valid"], r["successful"]) for r in rr], s.message
    tol = TOL.get(name, 1e-9)
    for i, r in zip(its, rr):
        assert _rel(i.cost, r["cost"]) <= tol, (i.iteration, i.cost, r["cost"])
        assert _rel(i.trust_region_radius, r["radius"]) <= tol, (i.iteration, i.trust_region_radius, r["radius"])
        if i.step_is_valid and i.iteration > 0:
            assert _rel(i.model_cost_change, r["mcc"]) <= 10 * tol, (i.iteration, i.model_cost_change, r["mcc"])
    x = g.get_blocks()
    assert np.abs(x - ref["x"]).max() <= 1e-7 * max(1.0, np.abs(ref["x"]).max())
    assert s.num_linear_solves == ref["steps"]
    # linear systems: every step computed, minus the ones that reused their Gauss-Newton step, plus mu retries
    assert g.num_factorizations() == ref["factorizations"] >= ref["steps"] - ref["reused"] - ref["invalid"]
    if name == "perturbed_large_radius":
        assert ref["reused"] > 0 and g.num_factorizations() < s.num_linear_solves


def _same_run(a, its_a, xa, b, its_b, xb):
    """two solves of one window by the same strategy: the same path (the assembly adds with atomics, so the last bits may differ)"""
    assert a.num_iterations == b.num_iterations and a.termination_type == b.termination_type
    assert [i.step_is_successful for i in its_a] == [i.step_is_successful for i in its_b]
    for i, j in zip(its_a, its_b):
        assert _rel(i.cost, j.cost) <= 1e-12 and _rel(i.trust_region_radius, j.trust_region_radius) <= 1e-12
    assert _rel(a.final_cost, b.final_cost) <= 1e-12
    assert np.abs(xa - xb).max() <= 1e-10 * max(1.0, np.abs(xb).max())


def test_lm_after_dogleg_is_fresh_lm(gpu_solver_cls):
    pr = _golden("all_types_seed0")
    fresh = gpu_solver_cls(0)
    pr.load(fresh)
    s0 = fresh.solve(fresh.options_default())
    g = gpu_solver_cls(0)
    pr.load(g)
    g.solve(_dogleg(g))
    g.reset_values()
    s1 = g.solve(g.options_default())
    _same_run(s1, g.iterations(), g.get_blocks(), s0, fresh.iterations(), fresh.get_blocks())
    assert g.num_factorizations() == fresh.num_factorizations() == s0.num_linear_solves


def test_default_options_are_levenberg_marquardt(gpu_solver_cls):
    g = gpu_solver_cls(0)
    o = g.options_default()
    assert o.trust_region_strategy_type == capi.TR_LEVENBERG_MARQUARDT
    assert g.options_vio().trust_region_strategy_type == capi.TR_LEVENBERG_MARQUARDT
    pr = _golden("lio_window_12kf")
    pr.load(g)
    a = g.solve(o)
    its_a, xa = g.iterations(), g.get_blocks()
    o.trust_region_strategy_type = capi.TR_LEVENBERG_MARQUARDT
    g.reset_values()
    b = g.solve(o)
    _same_run(a, its_a, xa, b, g.iterations(), g.get_blocks())
    # ... and DOGLEG is not what the default runs
    g.reset_values()
    d = g.solve(_dogleg(g))
    assert [i.trust_region_radius for i in g.iterations()] != [i.trust_region_radius for i in its_a] or d.num_iterations != a.num_iterations


def test_refusals(gpu_solver_cls):
    pr = _golden("all_types_seed0")
    g = gpu_solver_cls(0)
    pr.load(g)
    for lin in (capi.LINEAR_PCG, capi.LINEAR_SCHUR_PCG):
        o = _dogleg(g)
        o.linear_solver_type = lin
        with pytest.raises(capi.SolverError) as e:
            g.solve(o)
        assert e.value.code == capi.ERR_INVALID and "DOGLEG" in str(e.value)
    o = _dogleg(g)
    o.trust_region_strategy_type = capi.TR_SUBSPACE_DOGLEG
    with pytest.raises(capi.SolverError) as e:
        g.solve(o)
    assert e.value.code == capi.ERR_UNSUPPORTED and "SUBSPACE" in str(e.value)
    o.trust_region_strategy_type = 7
    with pytest.raises(capi.SolverError) as e:
        g.solve(o)
    assert e.value.code == capi.ERR_INVALID
    # inverse-depth factors
    pi = _golden("idp_window_8kf_60lm")
    gi = gpu_solver_cls(0)
    pi.load(gi)
    with pytest.raises(capi.SolverError) as e:
        gi.solve(_dogleg(gi))
    assert e.value.code == capi.ERR_UNSUPPORTED and "inverse-depth" in str(e.value)
    # bsgpu_localize_frames keeps its in-kernel LM
    o = _dogleg(g)
    with pytest.raises(capi.SolverError) as e:
        g.localize_frames([0, 0], np.zeros((0, 2)), [[1, 0, 0, 0]], [[0, 0, 0]], 0, points=np.zeros((0, 3)), options=o)
    assert e.value.code == capi.ERR_UNSUPPORTED
    # DOGLEG where AUTO resolves to the block-sparse PCG (a pose-side system above the exact path's limit)
    big = synthetic.pose_graph(n_pose=2200, n_loop=3000, seed=4207)
    gb = gpu_solver_cls(0)
    big.load(gb)
    o = _dogleg(gb)
    assert o.linear_solver_type == capi.LINEAR_AUTO
    with pytest.raises(capi.SolverError) as e:
        gb.solve(o)
    assert e.value.code == capi.ERR_UNSUPPORTED and "PCG" in str(e.value)
    # the context still solves (LM) after every refusal, and a refused solve reports no factorisation
    s = g.solve(g.options_default())
    assert s.is_solution_usable == 1 and g.num_factorizations() == s.num_linear_solves > 0
    o = _dogleg(g)
    o.linear_solver_type = capi.LINEAR_PCG
    with pytest.raises(capi.SolverError):
        g.solve(o)
    assert g.num_factorizations() == 0


def test_lm_dogleg_lm_under_captured_graphs(gpu_solver_cls, monkeypatch):
    """BSGPU_GRAPH=1: LM steps replayed from hipGraphs that hold the context's x and candidate buffers frozen.  A DOGLEG solve in between
    (five accepted steps) must leave them where the captured LM steps find them: the LM solves after it match a fresh context's."""
    pr = _golden("all_types_seed0")
    plain = gpu_solver_cls(0)
    pr.load(plain)
    sd = plain.solve(_dogleg(plain))
    its_d, xd = plain.iterations(), plain.get_blocks()
    assert sum(i.step_is_successful for i in its_d[1:]) % 2 == 1
    monkeypatch.setenv("BSGPU_GRAPH", "1")
    fresh = gpu_solver_cls(0)
    pr.load(fresh)
    s0 = fresh.solve(fresh.options_default())
    its0, x0 = fresh.iterations(), fresh.get_blocks()
    g = gpu_solver_cls(0)
    pr.load(g)
    g.solve(g.options_default())
    s1 = g.solve(_dogleg(g))                 # (from the LM optimum)
    assert s1.is_solution_usable == 1
    g.reset_values()
    s2 = g.solve(_dogleg(g))
    _same_run(s2, g.iterations(), g.get_blocks(), sd, its_d, xd)
    g.reset_values()
    s3 = g.solve(g.options_default())
    _same_run(s3, g.iterations(), g.get_blocks(), s0, its0, x0)
    g.solve(_dogleg(g))
    g.set_values(pr.values)
    s4 = g.solve(g.options_default())
    _same_run(s4, g.iterations(), g.get_blocks(), s0, its0, x0)


def test_batch_mixing_strategies_returns_lone_solves(gpu_solver_cls):
    names = ["all_types_seed0", "lio_window_12kf", "pose_graph_40", "all_types_seed7_const"]
    strategies = [capi.TR_DOGLEG, capi.TR_LEVENBERG_MARQUARDT, capi.TR_DOGLEG, capi.TR_LEVENBERG_MARQUARDT]
    lone = []
    for n, t in zip(names, strategies):
        g = gpu_solver_cls(0)
        _golden(n).load(g)
        o = g.options_default()
        o.trust_region_strategy_type = t
        s = g.solve(o)
        lone.append((s.final_cost, g.get_blocks(), [(i.cost, i.trust_region_radius) for i in g.iterations()], g.num_factorizations()))
    gs, opts = [], []
    for n, t in zip(names, strategies):
        g = gpu_solver_cls(0)
        _golden(n).load(g)
        o = g.options_default()
        o.trust_region_strategy_type = t
        gs.append(g)
        opts.append(o)
    ss = capi.Solver.solve_batch(gs, opts)
    for (fc, x, its, nf), g, s in zip(lone, gs, ss):
        assert g.num_factorizations() == nf == s.num_linear_solves
        assert _rel(s.final_cost, fc) <= 1e-12
        assert np.abs(g.get_blocks() - x).max() <= 1e-10 * max(1.0, np.abs(x).max())
        got = [(i.cost, i.trust_region_radius) for i in g.iterations()]
        assert len(got) == len(its)
        for (c1, r1), (c0, r0) in zip(got, its):
            assert _rel(c1, c0) <= 1e-12 and _rel(r1, r0) <= 1e-12
