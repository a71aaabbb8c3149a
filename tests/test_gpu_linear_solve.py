"""The reduced system's tiled Cholesky as a LINEAR SOLVER, at the accuracy a Cholesky solver owes (tests/linear_ref.py; the yardstick
itself is checked on the CPU by tests/test_linear_ref.py).

Part one, the hook (gpu.dense_solve -> DensePlan::build, chol_fused_kernel, the back-substitutions): banded SPD systems whose tile
structure makes the planner cut chains, separators, appendix tiles and K-chunks (asserted from the planner in test_linear_ref.py),
cond 3 to 8e10.  Part two, the production path (DimOrder + build_ordered, partial tiles inside the plan, the LM diagonal as tasks of
the factorisation, the single-launch back-substitution): ONE LM step of a linear graph from 0, whose exact system the test writes down
itself — (H + diag(d) / radius) delta = -g, H and g exact in double — under the default path, under the BSGPU_* switches that select
another one, and through solve_batch.

Criterion everywhere: the normwise backward error eta of the device's solution is at most MARGIN = 8 times that of numpy's Cholesky on
seeds 0..4 of the same family and shape (eta_ref), and never above Higham's a-priori bound n * gamma_{3n+1} (higham_cap), above which a
solve is wrong, not inaccurate.  Every test prints its figures before it asserts.

Measured on an MI355X (2026-10-20), device eta / eta_ref / their ratio, per family over its shapes (the multi-chain cases add with
FP64 atomics in no fixed order, so the last digit moves from run to run; three runs):
    dominant                       1.2e-16 .. 2.4e-16 / 6.4e-17 .. 1.0e-16 / 1.2 .. 2.8
    laplacian k = 10               2.8e-16 .. 7.6e-16 / 1.6e-16 .. 3.2e-16 / 1.4 .. 3.0
    laplacian k = 20               2.4e-16 .. 9.8e-16 / 1.9e-16 .. 2.9e-16 / 1.2 .. 3.9   (worst: n = 450 with the far coupling)
    laplacian k = 30               3.0e-16 .. 6.0e-16 / 1.7e-16 .. 4.2e-16 / 1.3 .. 2.2
    graphs, radius 2^20            1.6e-17 .. 9.4e-17 / 1.6e-17 .. 6.1e-17 / 0.8 .. 3.1
    graphs, radius 2^40            1.3e-17 .. 8.4e-17 / 9.9e-18 .. 7.3e-17 / 0.3 .. 2.9
    graphs under the 16 settings   3.3e-17 .. 9.1e-17 / 3.1e-17 .. 4.1e-17 / 0.9 .. 3.0
    solve_batch                    6.4e-17 .. 8.4e-17 / 3.1e-17 .. 3.7e-17 / 1.7 .. 2.7; against the lone solve 0, 0 and 5.7e-17
No case needs more than the margin: the explicit tile inverses of the back-substitution cost nothing measurable up to cond 8e10 (hook)
and 5e12 (graphs, k = 20 at radius 2^40), so no case is held to the cap alone.  The exact cases are exact.  Plans: the 450- and
522-dimensional plain graphs run as 6 and 8 chains (3 schedule steps, 10 and 11 tiles)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import linear_ref as lr
from beam_slam_amd import capi, gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not lr.longdouble_ok(), reason="numpy.longdouble is no wider than double here (2e-19 needed): "
                                                  "the backward error cannot be measured")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(v):
    return "-".join(str(int(x) if isinstance(x, bool) else x) for x in v) if isinstance(v, tuple) else str(v)


def _check(tag, e, ref, n):
    print("linear-solve %s: eta %.3e  eta_ref %.3e  ratio %.2f  cap %.3e" % (tag, e, ref, e / ref, lr.higham_cap(n)))
    assert np.isfinite(e) and e <= lr.higham_cap(n), (tag, e)
    assert e <= lr.MARGIN * ref, (tag, e, ref)


_died = []      # what faulted the device or ended with a signal or at its limit: this module starts nothing more on the device after it


@pytest.fixture(autouse=True)
def _nothing_after_a_device_fault():
    if _died:
        pytest.skip("%s ended with a device error, a signal or at its time limit: nothing more is started on the device" % _died[0])


def _device(what, fn, *args, **kwargs):
    """fn(*args) on the device; a HIP failure (ERR_DEVICE) is remembered, and every later test of the module is skipped"""
    try:
        return fn(*args, **kwargs)
    except capi.SolverError as e:
        if e.code == capi.ERR_DEVICE:
            _died.append(what)
        raise


def _dense_solve(*args, **kwargs):
    return _device("gpu.dense_solve", gpu.dense_solve, *args, **kwargs)


def _lm_step(*args):
    return _device("an LM step", lr.lm_step, *args)


def _evaluate_at_start(*args):
    return _device("an evaluation", lr.evaluate_at_start, *args)


# ---- part one: the hook -------------------------------------------------------------------------------------------------------------------------------
HOOK_FAMILIES = [("dominant", None)] + [("laplacian", k) for k in lr.LAPLACIAN_K]


@pytest.mark.parametrize("family,k", HOOK_FAMILIES, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", [s for s, _ in lr.HOOK_SHAPES], ids=_id)
def test_hook_backward_error(shape, family, k):
    n, bw, max_chains, far = shape
    fshape = (n, bw, far) if family == "dominant" else (n, bw, k, far)
    A, b = lr.system(family, fshape, 0)
    x, _ = _dense_solve(A, b, max_chains=max_chains)
    _check("hook %s %s" % (family, _id(shape + (k,))), lr.eta(A, b, x), lr.eta_ref(family, fshape), n)


def _diag_cases():
    rng = np.random.default_rng(11)
    out = [("identity-%d" % n, np.ones(n)) for n in (63, 65, 200)]
    out += [("diag-%d" % n, 4.0 ** rng.integers(-3, 4, n)) for n in (65, 200)]
    out.append(("blocks-200", np.repeat(4.0 ** rng.integers(-3, 4, 4), 64)[:200]))
    return out


@pytest.mark.parametrize("name,diag", _diag_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_hook_exact_cases_come_back_bit_for_bit(name, diag):
    """nothing rounds: square roots of powers of 4, quotients by powers of 2, products with 0 and 1"""
    n = len(diag)
    A = np.diag(diag)
    b = np.random.default_rng(12).integers(-64, 65, n) / 8.0
    x, _ = _dense_solve(A, b)
    print("linear-solve exact %s: max |x - b / diag| = %.3e" % (name, np.abs(x - b / diag).max()))
    assert (x == b / diag).all()
    x, _ = _dense_solve(A, np.zeros(n))
    assert (x == 0.0).all()


@pytest.mark.parametrize("shape", [(65, 30, 4, False), (449, 60, 4, False)], ids=_id)
def test_hook_zero_right_hand_side(shape):
    n, bw, max_chains, far = shape
    for A in (lr.dominant(n, bw, 0, far)[0], lr.laplacian(n, bw, 0, 20, far)[0]):
        x, _ = _dense_solve(A, np.zeros(n), max_chains=max_chains)
        assert (x == 0.0).all()


@pytest.mark.parametrize("shape", [(65, 30, 4, False), (200, 40, 4, False)], ids=_id)
def test_hook_reports_a_matrix_that_is_not_positive_definite(shape):
    """the Laplacian without its diagonal mass (singular) and one diagonal entry negated: ERR_NUMERIC, and the call after it is sound"""
    n, bw, max_chains, far = shape
    A, b = lr.laplacian(n, bw, 0, 20, far)
    bad = A.copy()
    bad[np.arange(n), np.arange(n)] -= 2.0 ** -20
    bad[n // 2, n // 2] = -bad[n // 2, n // 2]
    with pytest.raises(capi.SolverError) as err:
        _dense_solve(bad, b, max_chains=max_chains)
    assert err.value.code == capi.ERR_NUMERIC
    x, _ = _dense_solve(A, b, max_chains=max_chains)
    _check("hook after a failed call %s" % _id(shape), lr.eta(A, b, x), lr.eta_ref("laplacian", (n, bw, 20, far)), n)


# ---- part two: one LM step of a linear graph ----------------------------------------------------------------------------------------------------------
GRAPH_CASES = [(name, k, lg, jac) for name in lr.GRAPHS for k in lr.GRAPH_K for lg in lr.GRAPH_LOG2_RADIUS for jac in (0, 1)]


def _graph(name, k):
    N, band, loop, hub = lr.GRAPHS[name]
    return lr.vec3_graph(N, band, k, 0, loop, hub)


@pytest.mark.parametrize("k", lr.GRAPH_K)
@pytest.mark.parametrize("name", list(lr.GRAPHS))
def test_device_linearisation_is_the_tests_own(gpu_solver_cls, name, k):
    """what makes the written-down system THE system: the device's residuals and Jacobian at the start, bit for bit"""
    pr, J, r = _graph(name, k)
    r_d, J_d = _evaluate_at_start(gpu_solver_cls(0), pr)
    assert (J_d == J).all() and (r_d == r).all()


@pytest.mark.parametrize("name,k,log2_radius,jacobi", GRAPH_CASES)
def test_lm_step_backward_error(gpu_solver_cls, name, k, log2_radius, jacobi):
    pr, J, r = _graph(name, k)
    g = gpu_solver_cls(0)
    summary, delta = _lm_step(g, pr, log2_radius, jacobi)
    its = g.iterations()
    assert len(its) == 2 and its[1].step_is_successful == 1
    assert summary.linear_solver_used == capi.LINEAR_SCHUR_CHOLESKY
    M, rhs = lr.damped_system(J, r, 2.0 ** log2_radius, jacobi)
    _check("graph %s k=%d radius=2^%d jacobi=%d" % (name, k, log2_radius, jacobi), lr.eta(M, rhs, delta),
           lr.eta_ref("graph", lr.graph_shape(name, k, log2_radius, jacobi)), len(rhs))


@pytest.mark.parametrize("name", ["450", "522"])
def test_plain_graphs_are_planned_as_several_chains(gpu_solver_cls, name):
    """the 450- and 522-dimensional chains of band 4 are cut by the per-dimension nested dissection: what the cases above run is the
    multi-chain plan with separators, not one chain in natural order"""
    pr, _, _ = _graph(name, 20)
    g = gpu_solver_cls(0)
    pr.load(g)
    n_chains, n_steps, n_tiles = g.plan_info()
    print("linear-solve plan %s: n_chains %d n_steps %d n_tiles %d" % (name, n_chains, n_steps, n_tiles))
    assert n_chains >= 2


# ---- the alternative paths: one process per setting, one after another --------------------------------------------------------------------------------
ENV_GRAPHS = ["66", "450", "522-loop"]
ENV_K, ENV_LOG2_RADIUS, ENV_JACOBI = 20, 40, 1
SCRIPT = r"""
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import linear_ref as lr
from beam_slam_amd.gpu import GpuSolver
names, k, lg, jac, twice = sys.argv[1].split(","), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
out = {}
for name in names:
    N, band, loop, hub = lr.GRAPHS[name]
    pr, J, r = lr.vec3_graph(N, band, k, 0, loop, hub)
    g = GpuSolver(0)
    s, delta = lr.lm_step(g, pr, lg, jac)
    M, rhs = lr.damped_system(J, r, 2.0 ** lg, jac)
    rec = {"eta": lr.eta(M, rhs, delta), "ok": [int(i.step_is_successful) for i in g.iterations()], "solver": int(s.linear_solver_used),
           "plan": list(g.plan_info())}
    if twice:
        g2 = GpuSolver(0)
        rec["same_bytes"] = int(lr.lm_step(g2, pr, lg, jac)[1].tobytes() == delta.tobytes())
    out[name] = rec
print(json.dumps(out))
""" % (ROOT, os.path.join(ROOT, "tests"))

SETTINGS = [
    {"BSGPU_CHOL_FUSED": "0"},
    {"BSGPU_BACKSOLVE_LEGACY": "1"},
    {"BSGPU_BACKSOLVE_FUSED": "0"},
    {"BSGPU_BACKSOLVE_NO_W": "1"},
    {"BSGPU_BACKSOLVE_GLOBAL_Y": "1"},
    {"BSGPU_CHAINS": "1"},
    {"BSGPU_POSE_DIAG_LAUNCH": "1"},
    {"BSGPU_CHOL_EXT": "0"},
    {"BSGPU_CHOL_NOTURN": "0"},
    {"BSGPU_DIM_ORDER": "0"},
    {"BSGPU_DIM_ORDER": "0", "BSGPU_CHAINS": "4"},
    {"BSGPU_DIM_ORDER_DEPTH": "0"},
    {"BSGPU_DIM_ORDER_DEPTH": "2"},
    {"BSGPU_DIM_ABSORB": "0"},
    {"BSGPU_SHARED": "0"},
    {"BSGPU_GRAPH": "1"},
]
DIED = (-6, -11, 134, 139, 124, 137)


def _run_setting(setting, twice=False):
    env = dict(os.environ)
    env.update(setting)
    try:
        out = subprocess.run([sys.executable, "-c", SCRIPT, ",".join(ENV_GRAPHS), str(ENV_K), str(ENV_LOG2_RADIUS), str(ENV_JACOBI), str(int(twice))],
                             capture_output=True, text=True, timeout=120, env=env)
    except subprocess.TimeoutExpired:
        _died.append(str(setting))
        raise
    if out.returncode in DIED or out.returncode < 0:
        _died.append(str(setting))
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join("%s=%s" % kv for kv in s.items()))
def test_lm_step_backward_error_under_alternative_paths(setting):
    """Under BSGPU_CHOL_NOTURN=0 (the factorisation's updates in turn order) the factor is documented as bit-reproducible: two solves in
    that process give the same bytes.  (What that takes on a multi-chain plan — the K-chunks of a tile in list order, one summation order
    per update whatever the timing — is in DESIGN.md.)"""
    noturn = setting == {"BSGPU_CHOL_NOTURN": "0"}
    res = _run_setting(setting, twice=noturn)
    tag = ",".join("%s=%s" % kv for kv in setting.items())
    for name in ENV_GRAPHS:
        rec = res[name]
        print("linear-solve plan %s %s: %s" % (tag, name, rec["plan"]))
        assert rec["ok"] == [1, 1] and rec["solver"] == capi.LINEAR_SCHUR_CHOLESKY
        _check("graph %s under %s" % (name, tag), rec["eta"], lr.eta_ref("graph", lr.graph_shape(name, ENV_K, ENV_LOG2_RADIUS, ENV_JACOBI)),
               3 * lr.GRAPHS[name][0])
        if noturn:
            assert rec["same_bytes"] == 1
    if setting == {"BSGPU_CHAINS": "1"}:        # (the setting reached the process: one chain in natural order)
        assert all(res[name]["plan"][0] == 1 for name in ENV_GRAPHS)


# ---- solve_batch ----------------------------------------------------------------------------------------------------------------------------------------
def test_solve_batch_steps_meet_the_same_criterion(gpu_solver_cls):
    """Three windows in one bsgpu_solve_batch call: each step meets the criterion and is its lone solve's step in the backward measure
    (|M (delta_batch - delta_lone)| on eta's scale) — not bit for bit, the default update mode adds with FP64 atomics in no fixed order."""
    names, k, lg, jac = ["63", "66", "450"], 20, 40, 1
    graphs = [_graph(name, k) for name in names]
    solvers = [gpu_solver_cls(0) for _ in names]
    for (pr, _, _), g in zip(graphs, solvers):
        pr.load(g)
    summaries = _device("solve_batch", gpu_solver_cls.solve_batch, solvers, lr.step_options(solvers[0], lg, jac))
    for name, (pr, J, r), g, s in zip(names, graphs, solvers, summaries):
        delta = g.get_blocks()
        its = g.iterations()
        assert len(its) == 2 and its[1].step_is_successful == 1 and s.linear_solver_used == capi.LINEAR_SCHUR_CHOLESKY
        M, rhs = lr.damped_system(J, r, 2.0 ** lg, jac)
        ref = lr.eta_ref("graph", lr.graph_shape(name, k, lg, jac))
        _check("graph %s in a batch" % name, lr.eta(M, rhs, delta), ref, len(rhs))
        _, lone = _lm_step(gpu_solver_cls(0), pr, lg, jac)
        diff = lr.eta_between(M, rhs, delta, lone)
        print("linear-solve graph %s batch against lone: %.3e (ratio %.2f)" % (name, diff, diff / ref))
        assert diff <= lr.MARGIN * ref
