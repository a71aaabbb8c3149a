"""The yardstick of tests/test_gpu_linear_solve.py, checked before any device is involved (tests/linear_ref.py): the reference solver
stays at rounding level on every family and shape whatever the condition number, the graphs' normal equations are exact in double, the
hook's shapes reach the planner features they are there for (asked of dense_plan.h itself, tests/plan/plan_features.cpp), and the recipe
for the LM step's system is the one the CPU oracle solves."""
import os
import subprocess

import numpy as np
import pytest

import linear_ref as lr
from beam_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_longdouble = pytest.mark.skipif(not lr.longdouble_ok(), reason="numpy.longdouble is no wider than double here (eps %.3g, 2e-19 needed): "
                                      "the backward error cannot be measured" % float(np.finfo(np.longdouble).eps))

HOOK_CASES = [("dominant", (n, bw, far)) for (n, bw, _, far), _ in lr.HOOK_SHAPES] + \
             [("laplacian", (n, bw, k, far)) for (n, bw, _, far), _ in lr.HOOK_SHAPES for k in lr.LAPLACIAN_K]
HOOK_CASES = sorted(set(HOOK_CASES), key=HOOK_CASES.index)      # (450 is there with max_chains 4 and 1: one system)
GRAPH_CASES = [(name, k, lg, jac) for name in lr.GRAPHS for k in lr.GRAPH_K for lg in lr.GRAPH_LOG2_RADIUS for jac in (0, 1)]


def _id(v):
    return "-".join(str(int(x) if isinstance(x, bool) else x) for x in v) if isinstance(v, tuple) else str(v)


@needs_longdouble
@pytest.mark.parametrize("family,shape", HOOK_CASES, ids=_id)
def test_reference_stays_at_rounding_level(family, shape):
    """numpy's Cholesky is backward stable on every matrix family and shape: cond 3 to 8e10, eta at most 4.1e-16 measured"""
    assert lr.eta_ref(family, shape) <= 1e-15


@needs_longdouble
@pytest.mark.parametrize("name,k,log2_radius,jacobi", GRAPH_CASES)
def test_reference_stays_at_rounding_level_on_the_graphs(name, k, log2_radius, jacobi):
    assert lr.eta_ref("graph", lr.graph_shape(name, k, log2_radius, jacobi)) <= 1e-15


def test_condition_numbers_are_what_the_families_are_for():
    assert np.linalg.cond(lr.dominant(449, 60, 0)[0]) < 10.0
    for k, lo in zip(lr.LAPLACIAN_K, (1e4, 1e7, 1e10)):
        assert lo < np.linalg.cond(lr.laplacian(449, 60, 0, k)[0]) < 100.0 * lo


@pytest.mark.parametrize("name", list(lr.GRAPHS))
@pytest.mark.parametrize("k", lr.GRAPH_K)
def test_graph_normal_equations_are_exact_in_double(name, k):
    """every entry of H and g is a whole multiple of 2^-40 below 2^12, and so is every partial sum (normal_equations asserts it): the
    system the test writes down is the one a device assembles, in whatever order it adds"""
    N, band, loop, hub = lr.GRAPHS[name]
    for seed in lr.SEEDS:
        _, J, r = lr.vec3_graph(N, band, k, seed, loop, hub)
        H, g = lr.normal_equations(J, r)
        assert (H == H.T).all() and H.shape == (3 * N, 3 * N)
        # ... and it is the sum in extended precision too
        Jl = J.astype(np.longdouble)
        assert (Jl.T @ r.astype(np.longdouble) == g).all()
        if seed == 0 and N <= 64:
            assert (Jl.T @ Jl == H).all()


@pytest.fixture(scope="module")
def plan_features(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_features")
    out = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                          os.path.join(ROOT, "tests", "plan", "plan_features.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]

    def run(A, max_chains):
        adj = lr.tile_adjacency(A)
        rows = ["".join("1" if v else "0" for v in row) for row in adj]
        res = subprocess.run([exe, str(A.shape[0]), str(max_chains), str(len(rows))] + rows, capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stderr[-2000:]
        return {k: int(v) for k, v in (kv.split("=") for kv in res.stdout.split())}
    return run


@pytest.mark.parametrize("shape,expect", lr.HOOK_SHAPES, ids=_id)
def test_hook_shapes_reach_the_planner_features(plan_features, shape, expect):
    """The plan bsgpu_dense_solve builds for each shape (from the non-zero tiles of the very matrices the GPU test sends): independent
    chains with separators, appendix-tile tasks, K-chunks of a chain's last updates, the level-synchronised back-substitution.  The
    qualitative facts only — a planner that keeps the coverage may change every count."""
    n, bw, max_chains, far = shape
    chains, ext, split, level_sync = expect
    feats = []
    for A in (lr.dominant(n, bw, 0, far)[0],) + tuple(lr.laplacian(n, bw, 0, k, far)[0] for k in lr.LAPLACIAN_K):
        adj = lr.tile_adjacency(A)
        T = adj.shape[0]
        wt = (bw + 63) // 64
        band = np.abs(np.arange(T)[:, None] - np.arange(T)[None, :]) <= wt
        if far:
            band[0, T - 1] = band[T - 1, 0] = True
        assert (adj == band).all()                       # a banded tile structure of half-width wt, plus the far coupling
        feats.append(plan_features(A, max_chains))
    assert all(f == feats[0] for f in feats)             # one structure, one plan
    f = feats[0]
    assert f["n_chains"] == chains
    assert f["panels"] >= 1 and f["chain"] >= 1
    if ext is not None:
        assert (f["ext"] > 0) == ext
    if split is not None:
        assert (f["split"] > 0) == split
    assert bool(f["bs_level_sync"]) == level_sync


def test_the_shapes_cover_every_feature():
    exp = [e for _, e in lr.HOOK_SHAPES]
    assert {e[0] for e in exp} == {1, 2, 4}
    assert any(e[1] for e in exp) and any(e[2] for e in exp) and any(e[3] for e in exp) and any(e[3] is False for e in exp)
    assert {s[0] % 64 for s, _ in lr.HOOK_SHAPES} >= {0, 1, 63}     # no padding, one real column, one padded column


@needs_longdouble
@pytest.mark.parametrize("name,k,log2_radius,jacobi", GRAPH_CASES)
def test_oracle_lm_step_solves_the_damped_normal_equations(oracle_cls, name, k, log2_radius, jacobi):
    """The recipe the GPU test holds the device to — (H + diag(d) / radius) delta = -g — is what the CPU oracle's first LM step solves:
    its Jacobian and residuals are the test's own, bit for bit, and its step has eta within the margin of numpy's (measured
    5.5e-17 .. 6.5e-17 against 3.9e-17 .. 4.9e-17)."""
    shape = lr.graph_shape(name, k, log2_radius, jacobi)
    pr, J, r = lr.vec3_graph(*shape[:3], 0, *shape[3:5])
    o = oracle_cls()
    summary, delta = lr.lm_step(o, pr, log2_radius, jacobi)
    r_o, J_o = lr.evaluate_at_start(oracle_cls(), pr)
    assert (J_o == J).all() and (r_o == r).all()
    its = o.iterations()
    assert len(its) == 2 and its[1].step_is_successful == 1
    assert summary.linear_solver_used == capi.LINEAR_SCHUR_CHOLESKY
    M, rhs = lr.damped_system(J, r, 2.0 ** log2_radius, jacobi)
    e, ref = lr.eta(M, rhs, delta), lr.eta_ref("graph", shape)
    assert e <= lr.higham_cap(len(rhs))
    assert e <= lr.MARGIN * ref, (e, ref)
