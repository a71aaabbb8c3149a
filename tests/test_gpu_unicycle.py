"""BSGPU_F_UNICYCLE on the MI355X: evaluation against the dual-number restatement (tests/unicycle_ref.py), solves against a dense
numpy manifold Gauss-Newton run to convergence (the oracle evaluates every other factor: it has no unicycle type), the batched
solve against lone solves, marginalisation against the numpy Schur complement and covariance requests against (J^T J)^-1."""
import numpy as np
import pytest

from beam_slam_amd import capi, synthetic
import unicycle_ref as U

pytestmark = pytest.mark.gpu


def _tight(g, linear=None):
    o = g.options_default()
    o.max_num_iterations = 200
    o.function_tolerance = 1e-16
    o.gradient_tolerance = 1e-16
    o.parameter_tolerance = 1e-16
    if linear is not None:
        o.linear_solver_type = linear
        o.pcg_tolerance = 1e-12
        o.pcg_max_iterations = 5000
    return o


def test_evaluate_matches_restatement(gpu_solver_cls, oracle_cls):
    for dense in (False, True):
        pr = synthetic.unicycle_window(n_states=40, seed=7 + dense, dense_cov=dense)
        g = gpu_solver_cls(0)
        pr.load(g)
        cost, r, _, J = g.evaluate(jacobian=True)
        toff = [g.tangent_offset(b) for b in range(pr.n_blocks)]
        ru, Ju = U.unicycle_rows(pr, pr.values, toff, J.shape[1])
        m = ru.size
        assert np.abs(r[-m:] - ru).max() <= 1e-12 * np.abs(ru).max()
        assert np.abs(J[-m:] - Ju).max() <= 1e-10 * np.abs(Ju).max()
        Jr, rr, _ = U.reference_system(pr, oracle_cls)
        c_ref = 0.5 * float(rr @ rr)
        assert abs(cost - c_ref) <= 1e-12 * c_ref, (cost, c_ref)


def _solve_against_gn(g, pr, oracle_cls, opt):
    pr.load(g)
    s = g.solve(opt)
    assert s.is_solution_usable == 1
    x_ref, c_ref = U.gauss_newton(pr, oracle_cls)
    assert abs(s.final_cost - c_ref) <= 1e-9 * c_ref, (s.final_cost, c_ref)
    assert np.abs(g.get_blocks() - x_ref).max() <= 1e-7 * max(1.0, np.abs(x_ref).max())
    return s


def test_pose_only_window_reaches_gauss_newton_optimum(gpu_solver_cls, oracle_cls):
    pr = synthetic.unicycle_window(n_states=200, seed=3)
    g = gpu_solver_cls(0)
    _solve_against_gn(g, pr, oracle_cls, _tight(g))


def test_pose_only_window_under_pcg(gpu_solver_cls, oracle_cls):
    pr = synthetic.unicycle_window(n_states=200, seed=4, dense_cov=True)
    g = gpu_solver_cls(0)
    _solve_against_gn(g, pr, oracle_cls, _tight(g, capi.LINEAR_PCG))


def test_visual_window_with_unicycle_factors(gpu_solver_cls, oracle_cls):
    pr = synthetic.unicycle_window(n_states=20, n_lm=500, seed=5, dense_cov=True)
    assert pr.n_factors(capi.F_REPROJ) > 0
    g = gpu_solver_cls(0)
    _solve_against_gn(g, pr, oracle_cls, _tight(g))


def test_batch_matches_lone_solves(gpu_solver_cls):
    cases = [synthetic.unicycle_window(n_states=30 + 5 * i, seed=100 + i, dense_cov=i % 2 == 1) for i in range(8)]
    cases.insert(3, synthetic.lio_window(n_kf=20, n_rel=300, seed=20250801))
    lone = []
    for pr in cases:
        g = gpu_solver_cls(0)
        pr.load(g)
        lone.append((g.solve(g.options_default()), g.get_blocks(), g.iterations()))
    gs = []
    for pr in cases:
        g = gpu_solver_cls(0)
        pr.load(g)
        gs.append(g)
    sums = gpu_solver_cls.solve_batch(gs, gs[0].options_default())
    for (s0, x0, it0), g, s1 in zip(lone, gs, sums):
        assert s1.num_iterations == s0.num_iterations and s1.termination_type == s0.termination_type
        assert s1.num_successful_steps == s0.num_successful_steps
        it1 = g.iterations()
        assert len(it0) == len(it1)
        for a, b in zip(it0, it1):
            assert a.step_is_successful == b.step_is_successful
            assert abs(a.cost - b.cost) <= 1e-9 * abs(a.cost)
        assert abs(s1.final_cost - s0.final_cost) <= 1e-9 * abs(s0.final_cost)
        assert np.abs(g.get_blocks() - x0).max() < 1e-8


def _cols(pr, toff, blocks):
    return np.concatenate([np.arange(toff[b], toff[b] + 3) for b in blocks])


def test_marginalize_oldest_state(gpu_solver_cls, oracle_cls):
    pr = synthetic.unicycle_window(n_states=8, seed=9, dense_cov=True)
    kf = pr.meta["kf_blocks"]
    g = gpu_solver_cls(0)
    pr.load(g)
    g.solve(g.options_default())
    x = g.get_blocks()
    marg = [int(b) for b in kf[0]]
    kept, A, b, xbar = g.marginalize(marg, pr.size)
    assert sorted(int(k) for k in kept) == sorted(int(v) for v in kf[1])
    # numpy: the rows of every factor touching state 0 (its priors and the first unicycle factor), restated at the same point
    J, r, toff = U.reference_system(pr, oracle_cls, x)
    mcols, kcols = _cols(pr, toff, marg), _cols(pr, toff, [int(k) for k in kept])
    rows = np.where(np.abs(J[:, mcols]).max(axis=1) > 0)[0]
    J, r = J[rows], r[rows]
    H, gr = J.T @ J, J.T @ r
    Hmm, Hkm, Hkk = H[np.ix_(mcols, mcols)], H[np.ix_(kcols, mcols)], H[np.ix_(kcols, kcols)]
    S = Hkk - Hkm @ np.linalg.solve(Hmm, Hkm.T)
    gs = gr[kcols] - Hkm @ np.linalg.solve(Hmm, gr[mcols])
    assert np.abs(A.T @ A - S).max() <= 1e-9 * np.abs(S).max()
    assert np.abs(A.T @ b - gs).max() <= 1e-9 * max(1.0, np.abs(gs).max())


def test_covariance_requests(gpu_solver_cls, oracle_cls):
    pr = synthetic.unicycle_window(n_states=12, seed=13, dense_cov=True)
    kf = pr.meta["kf_blocks"]   # q, p, v, w, a per state
    g = gpu_solver_cls(0)
    pr.load(g)
    g.solve(g.options_default())
    x = g.get_blocks()
    pairs = [(kf[5, 3], kf[5, 3]), (kf[7, 4], kf[2, 1]), (kf[4, 0], kf[9, 2]), (kf[11, 3], kf[11, 3])]
    got = g.covariance_requests(pairs)
    J, _, toff = U.reference_system(pr, oracle_cls, x)
    C = np.linalg.inv(J.T @ J)
    for (a, b_), m in zip(pairs, got):
        ref = C[np.ix_(np.arange(toff[a], toff[a] + 3), np.arange(toff[b_], toff[b_] + 3))]
        assert np.abs(m - ref).max() <= 1e-8 * np.abs(C).max(), (a, b_, m, ref)
