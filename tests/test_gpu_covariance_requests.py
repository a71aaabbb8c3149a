"""bsgpu_covariance_requests (Graph::getCovariance(requests, matrices) for any variable) against the oracle's dense (J^T J)^-1.
Tolerance as test_gpu_parity.py::test_covariance_blocks_match_oracle: 1e-8 relative to the diagonal scale of the pair."""
import numpy as np
import pytest

from beam_slam_amd import capi, synthetic
from helpers import mixed_problem

pytestmark = pytest.mark.gpu


def _pair(pr, oracle_cls, gpu_solver_cls):
    g = gpu_solver_cls(0)
    o = oracle_cls()
    pr.load(g)
    pr.load(o)
    return g, o


def _tsize(pr, b):
    return 3 if pr.manifold[b] == capi.MANIFOLD_QUAT_RIGHT else int(pr.size[b])


def _check_against_oracle(pr, g, o, pairs):
    got = g.covariance_requests(pairs)
    assert len(got) == len(pairs)
    for (a, b), cg in zip(pairs, got):
        ta, tb = _tsize(pr, a), _tsize(pr, b)
        assert cg.shape == (ta, tb)
        co = o.covariance(int(a), int(b), ta, tb)
        caa = o.covariance(int(a), int(a), ta, ta)
        cbb = o.covariance(int(b), int(b), tb, tb)
        scale = max(np.abs(co).max(), np.sqrt(np.abs(caa).max() * np.abs(cbb).max()))
        assert np.abs(cg - co).max() <= 1e-8 * scale, (a, b, np.abs(cg - co).max(), scale)
    return got


def _observed_by(pr, ftype, block):
    """Landmarks of the reprojection factors of type ftype whose orientation or position slot is `block`."""
    out = set()
    for idx, _, _, _ in pr.factors.get(ftype, []):
        for row in idx:
            if row[0] == block or row[1] == block:
                out.add(int(row[2]))
    return sorted(out)


def test_landmarks_and_poses_mixed_problem(oracle_cls, gpu_solver_cls):
    pr = mixed_problem(4, n_state=4, n_lm=20, with_losses=True, consistent=True)
    g, o = _pair(pr, oracle_cls, gpu_solver_cls)
    g.solve(); o.set_values(g.get_blocks())
    st, lm = pr.meta["states"], [int(b) for b in pr.meta["landmarks"]]
    pairs = [(lm[0], lm[0]), (lm[0], lm[1]), (lm[2], int(st[1, 0])), (int(st[0, 0]), int(st[0, 0])), (int(st[1, 1]), int(st[3, 0])),
             (int(st[2, 1]), lm[3]), (lm[7], lm[7]), (lm[1], lm[0])]
    got = _check_against_oracle(pr, g, o, pairs)
    assert np.allclose(got[1], got[-1].T, rtol=0, atol=1e-12 * np.abs(got[0]).max())
    # a later solve is not disturbed by the query
    c0 = g.solve().final_cost
    assert abs(c0 - o.solve().final_cost) <= 1e-6 * c0


def test_landmarks_and_poses_vio_window(oracle_cls, gpu_solver_cls):
    pr = synthetic.vio_window(n_kf=8, n_lm=60, seed=5)
    g, o = _pair(pr, oracle_cls, gpu_solver_cls)
    g.solve(); o.set_values(g.get_blocks())
    kf, lm = pr.meta["kf_blocks"], [int(b) for b in pr.meta["lm_blocks"]]
    pairs = [(lm[3], lm[3]), (lm[3], lm[40]), (lm[10], int(kf[5, 1])), (int(kf[2, 0]), lm[10]), (int(kf[4, 1]), int(kf[4, 1])),
             (int(kf[6, 2]), int(kf[1, 0])), (lm[59], lm[59])]
    _check_against_oracle(pr, g, o, pairs)


def test_more_than_one_rhs_tile(oracle_cls, gpu_solver_cls):
    """32 landmarks (96 rows) and three poses: two factorisation passes, cross pairs whose rows lie in different passes."""
    pr = synthetic.vio_window(n_kf=8, n_lm=60, seed=6)
    g, o = _pair(pr, oracle_cls, gpu_solver_cls)
    g.solve(); o.set_values(g.get_blocks())
    kf, lm = pr.meta["kf_blocks"], [int(b) for b in pr.meta["lm_blocks"]]
    pairs = [(lm[i], lm[i]) for i in range(32)]
    pairs += [(lm[0], lm[31]), (lm[20], lm[21]), (int(kf[1, 1]), lm[0]), (lm[31], int(kf[1, 1])), (int(kf[7, 0]), int(kf[0, 1])),
              (lm[2], int(kf[7, 0])), (int(kf[1, 1]), int(kf[1, 1]))]
    _check_against_oracle(pr, g, o, pairs)


def test_landmark_on_the_pose_only_route_and_constant_observer(oracle_cls, gpu_solver_cls):
    """A landmark with a position prior is not eliminated (unit rows); a landmark observed by a held-constant state."""
    pr = mixed_problem(9, n_state=4, n_lm=16, with_losses=True, hold_first=True, consistent=True)
    lms = [int(b) for b in pr.meta["landmarks"]]
    A = synthetic.sqrt_information_upper(0.01 * np.eye(3))
    pr.add_factors(capi.F_ABS_VEC3, [[lms[0]]], [np.concatenate([pr.block(lms[0]) + 0.02, A.ravel()])])
    st = pr.meta["states"]
    seen_by_const = [b for b in _observed_by(pr, capi.F_REPROJ, int(st[0, 0])) if b != lms[0]]
    assert seen_by_const
    lc = seen_by_const[0]
    g, o = _pair(pr, oracle_cls, gpu_solver_cls)
    g.solve(); o.set_values(g.get_blocks())
    pairs = [(lms[0], lms[0]), (lms[0], lc), (lc, lc), (lc, int(st[2, 1])), (lms[0], int(st[1, 0])), (lms[5], lms[0])]
    _check_against_oracle(pr, g, o, pairs)


@pytest.mark.parametrize("elim", [True, False])
def test_inverse_depth_scalars(oracle_cls, gpu_solver_cls, monkeypatch, elim):
    if not elim:
        monkeypatch.setenv("BSGPU_IDP_ELIM", "0")
    pr = synthetic.idp_window(n_kf=8, n_lm=60)
    g, o = _pair(pr, oracle_cls, gpu_solver_cls)
    g.solve(); o.set_values(g.get_blocks())
    kf, rho = pr.meta["kf_blocks"], [int(b) for b in pr.meta["rho_blocks"]]
    pairs = [(rho[0], rho[0]), (rho[0], rho[1]), (rho[2], int(kf[3, 1])), (int(kf[4, 0]), int(kf[4, 0])), (int(kf[6, 0]), rho[5]),
             (rho[59], rho[59]), (rho[30], rho[59])]
    _check_against_oracle(pr, g, o, pairs)


def test_pose_requests_agree_with_per_pair_covariance(gpu_solver_cls):
    pr = mixed_problem(4, n_state=4, n_lm=20, consistent=True)
    g = gpu_solver_cls(0)
    pr.load(g)
    g.solve()
    st = pr.meta["states"]
    pairs = [(st[0, 0], st[0, 0]), (st[0, 0], st[0, 1]), (st[1, 1], st[3, 0]), (st[2, 2], st[2, 4]), (st[3, 3], st[0, 1]), (st[3, 1], st[3, 1])]
    pairs = [(int(a), int(b)) for a, b in pairs]
    got = g.covariance_requests(pairs)
    for (a, b), cg in zip(pairs, got):
        c1 = g.covariance(a, b)
        scale = np.sqrt(np.abs(g.covariance(a, a)).max() * np.abs(g.covariance(b, b)).max())
        assert np.abs(cg - c1).max() <= 1e-12 * scale


def test_reference_kat_as_one_call(gpu_solver_cls):
    """bs_constraints/tests/absolute_imu_state_3d_stamped_constraint_test.cpp:167-297: the 15 x 15 covariance from one 15-pair call."""
    from test_oracle_reference_kats import _kat1_problem, kat1_cov
    pr, b = _kat1_problem()
    g = gpu_solver_cls(0)
    pr.load(g)
    assert g.solve().is_solution_usable == 1
    pairs = [(int(b[i]), int(b[j])) for i in range(5) for j in range(i, 5)]
    assert len(pairs) == 15
    got = g.covariance_requests(pairs)
    cov = np.zeros((15, 15))
    for (i, j), m in zip([(i, j) for i in range(5) for j in range(i, 5)], got):
        cov[3 * i:3 * i + 3, 3 * j:3 * j + 3] = m
        cov[3 * j:3 * j + 3, 3 * i:3 * i + 3] = m.T
    assert np.abs(cov - kat1_cov()).max() < 1e-5


def test_sizes_only_and_empty(gpu_solver_cls):
    import ctypes as C
    pr = synthetic.vio_window(n_kf=5, n_lm=40, seed=3, track_min=3, track_max=5)
    g = gpu_solver_cls(0)
    pr.load(g)
    assert g.covariance_requests([]) == []
    kf, lm = pr.meta["kf_blocks"], pr.meta["lm_blocks"]
    fn = g._f("covariance_requests")
    fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    pairs = np.array([[lm[0], lm[0]], [kf[1, 0], lm[2]]], np.int32)
    off = np.full(3, -1, np.int64)
    assert fn(g._ctx, 2, pairs.ctypes.data_as(C.POINTER(C.c_int32)), off.ctypes.data_as(C.POINTER(C.c_int64)), None) == capi.OK
    assert list(off) == [0, 9, 18]
    assert fn(g._ctx, 2, None, None, None) == capi.ERR_INVALID
    assert fn(g._ctx, -1, None, None, None) == capi.ERR_INVALID


def test_errors(oracle_cls, gpu_solver_cls):
    # a constant block
    pr = mixed_problem(9, n_state=4, n_lm=16, hold_first=True, consistent=True)
    g, o = _pair(pr, oracle_cls, gpu_solver_cls)
    st = pr.meta["states"]
    with pytest.raises(capi.SolverError) as e:
        g.covariance_requests([(int(st[1, 0]), int(st[0, 0]))])
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.SolverError) as e:
        g.covariance_requests([(int(st[1, 0]), pr.n_blocks)])
    assert e.value.code == capi.ERR_INVALID
    # ... and the context solves as the oracle does after a query
    g.covariance_requests([(int(st[1, 0]), int(pr.meta["landmarks"][0]))])
    sg, so = g.solve(), o.solve()
    assert abs(sg.final_cost - so.final_cost) <= 1e-6 * so.final_cost
    # a gauge-free pose graph: singular J^T J
    pg = synthetic.pose_graph(n_pose=12, n_loop=10, seed=4)
    pg.factors.pop(capi.F_ABSPOSE)
    g2 = gpu_solver_cls(0)
    pg.load(g2)
    with pytest.raises(capi.SolverError) as e2:
        g2.covariance_requests([(0, 0), (0, 1)])
    assert e2.value.code == capi.ERR_NUMERIC
    # a reduced system above the dense limit (the block-sparse PCG path has no factor)
    big = synthetic.pose_graph(n_pose=2200, n_loop=3000, seed=3)
    g3 = gpu_solver_cls(0)
    big.load(g3)
    with pytest.raises(capi.SolverError) as e3:
        g3.covariance_requests([(0, 0)])
    assert e3.value.code == capi.ERR_UNSUPPORTED
