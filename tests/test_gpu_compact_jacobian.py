"""The compact pose part of the reprojection Jacobian (Visual::ja, csrc/bsgpu_internal.h): a window that keeps no C rows stores
[theta row 0 | theta row 1] per factor and its readers take the translation columns from the landmark part (d r / d t = -d r / d P).
Against the full layout (BSGPU_COMPACT_J=0) on the same windows: the Jacobian read-back bit for bit, full solves (LM, DOGLEG, batched)
and a covariance request within the bounds tests/test_gpu_band.py::test_no_c_rows uses between two assemblies of one system
(costs rtol 1e-11, final cost 1e-10 relative, values 1e-7).  The arithmetic is the same in both layouts (negation is exact); what differs
from run to run is the order of the FP64 atomic adds, as between two runs of one layout: each test prints the gap it measured."""
import numpy as np
import pytest

from beam_slam_amd import capi, synthetic

pytestmark = pytest.mark.gpu


def _n_reproj(pr):
    return sum(int(t[0].shape[0]) for t in pr.factors[capi.F_REPROJ])


def _hold_and_fix(pr):
    """a constant landmark in nine and a held pose: factors of constant landmarks store B = 0, the window keeps the full layout"""
    for b in pr.meta["lm_blocks"][::9]:
        pr.is_const[int(b)] = 1
    for b in pr.meta["kf_blocks"][5][:2]:
        pr.is_const[int(b)] = 1
    return pr


def _both(monkeypatch, fn):
    """fn() on fresh contexts with the full layout forced, then with the library's own choice"""
    monkeypatch.setenv("BSGPU_COMPACT_J", "0")
    full = fn()
    monkeypatch.setenv("BSGPU_COMPACT_J", "1")
    return full, fn()


def _solve(pr, gpu_solver_cls, iters=7, dogleg=False):
    g = gpu_solver_cls(0)
    pr.load(g)
    o = g.options_vio()
    o.max_num_iterations = iters
    o.max_solver_time_in_seconds = 0.0
    if dogleg:
        o.trust_region_strategy_type = capi.TR_DOGLEG
    s = g.solve(o)
    return s, [(i.cost, i.step_is_successful, i.trust_region_radius) for i in g.iterations()], g.get_blocks(), g.reproj_jacobian_bytes()


def _same_solve(tag, a, b):
    (s0, it0, x0, _), (s1, it1, x1, _) = a, b
    assert len(it0) == len(it1) and [i[1] for i in it0] == [i[1] for i in it1]          # the same accept / reject sequence
    c0, c1 = np.array([i[0] for i in it0]), np.array([i[0] for i in it1])
    gap_c = float(np.max(np.abs(c0 - c1) / np.abs(c0)))
    gap_f = abs(s0.final_cost - s1.final_cost) / abs(s0.final_cost)
    gap_x = float(np.abs(x0 - x1).max())
    print(f"{tag}: iterations {len(it0)} cost gap {gap_c:.3e} final cost gap {gap_f:.3e} values gap {gap_x:.3e}")
    assert np.allclose(c0, c1, rtol=1e-11, atol=0.0)
    assert gap_f <= 1e-10
    assert gap_x < 1e-7


@pytest.mark.parametrize("kind", ["compact", "full"])
def test_jacobian_readback_is_bit_identical(gpu_solver_cls, monkeypatch, kind):
    """bsgpu_evaluate returns the full 2 x 9 rows under either layout; a window with a constant landmark and a held pose reports the full
    layout (the library's byte count of the evaluation, 200 B per factor against 152) whatever the switch says."""
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    pr = synthetic.vio_window(n_kf=12, n_lm=300, seed=71, track_min=2, track_max=9)
    if kind == "full":
        pr = _hold_and_fix(pr)

    def run():
        g = gpu_solver_cls(0)
        pr.load(g)
        cost, r, grad, J = g.evaluate(jacobian=True)
        return cost, r, grad, J, g.reproj_jacobian_bytes()

    (c0, r0, g0, J0, b0), (c1, r1, g1, J1, b1) = _both(monkeypatch, run)
    n = _n_reproj(pr)
    assert b0 - b1 == (48 * n if kind == "compact" else 0), (b0, b1, n)
    assert np.array_equal(J0, J1) and np.array_equal(r0, r1) and c0 == c1
    assert np.array_equal(g0, g1)   # (the host sums the gradient of the read-back rows in one order)
    assert np.count_nonzero(J0) > 0


def test_band_window_solves_the_same(gpu_solver_cls, monkeypatch):
    """the window of test_gpu_band.py::test_no_c_rows (band form forced, robust losses, a held pose, pose-only riders)"""
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    pr = synthetic.vio_window(n_kf=22, n_lm=1200, seed=59, track_min=2, track_max=12)
    for b in pr.meta["kf_blocks"][7][:2]:
        pr.is_const[int(b)] = 1
    full, compact = _both(monkeypatch, lambda: _solve(pr, gpu_solver_cls))
    assert full[3] - compact[3] == 48 * _n_reproj(pr)
    _same_solve("band window", full, compact)


def test_dogleg_solves_the_same(gpu_solver_cls, monkeypatch):
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    pr = synthetic.vio_window(n_kf=16, n_lm=700, seed=60, track_min=2, track_max=10)
    full, compact = _both(monkeypatch, lambda: _solve(pr, gpu_solver_cls, iters=6, dogleg=True))
    assert full[3] - compact[3] == 48 * _n_reproj(pr)
    _same_solve("dogleg", full, compact)


def test_batched_windows_solve_the_same(gpu_solver_cls, monkeypatch):
    """bsgpu_solve_batch over a window that takes the compact layout and one that must not (constant landmarks): each launch reads its window's table entry"""
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    cases = [synthetic.vio_window(n_kf=16, n_lm=700, seed=61, track_min=2, track_max=10),
             _hold_and_fix(synthetic.vio_window(n_kf=16, n_lm=700, seed=62, track_min=2, track_max=10))]

    def run():
        gs = []
        for pr in cases:
            g = gpu_solver_cls(0)
            pr.load(g)
            gs.append(g)
        opt = gs[0].options_vio()
        opt.max_num_iterations = 5
        opt.max_solver_time_in_seconds = 0.0
        sums = gpu_solver_cls.solve_batch(gs, opt)
        return [(s, [(i.cost, i.step_is_successful, i.trust_region_radius) for i in g.iterations()], g.get_blocks(), g.reproj_jacobian_bytes())
                for s, g in zip(sums, gs)]

    full, compact = _both(monkeypatch, run)
    assert full[0][3] - compact[0][3] == 48 * _n_reproj(cases[0]) and full[1][3] == compact[1][3]
    for w in range(2):
        _same_solve(f"batched window {w}", full[w], compact[w])


def test_covariance_request_is_the_same(gpu_solver_cls, monkeypatch):
    """landmark and pose blocks of a compact window at its start values; the bound is the one tests/test_gpu_covariance_requests.py holds
    against the oracle (1e-8 of the pair's diagonal scale)"""
    monkeypatch.setenv("BSGPU_PAIRS_BAND", "1")
    pr = synthetic.vio_window(n_kf=12, n_lm=300, seed=71, track_min=2, track_max=9)
    kf, lm = pr.meta["kf_blocks"], [int(b) for b in pr.meta["lm_blocks"]]
    pairs = [(lm[3], lm[3]), (lm[3], lm[40]), (lm[10], int(kf[5, 1])), (int(kf[2, 0]), lm[10]), (int(kf[4, 1]), int(kf[4, 1])), (int(kf[6, 1]), int(kf[1, 0]))]
    diag = sorted({b for p in pairs for b in p})

    def run():
        g = gpu_solver_cls(0)
        pr.load(g)
        return g.covariance_requests(pairs), dict(zip(diag, g.covariance_requests([(b, b) for b in diag]))), g.reproj_jacobian_bytes()

    (cov0, d0, b0), (cov1, _, b1) = _both(monkeypatch, run)
    assert b0 - b1 == 48 * _n_reproj(pr)
    worst = 0.0
    for (a, b), m0, m1 in zip(pairs, cov0, cov1):
        scale = max(np.abs(m0).max(), np.sqrt(np.abs(d0[a]).max() * np.abs(d0[b]).max()))
        worst = max(worst, float(np.abs(m0 - m1).max() / scale))
        assert np.abs(m0 - m1).max() <= 1e-8 * scale, (a, b)
    print(f"covariance: largest gap {worst:.3e} of the pair's scale")
