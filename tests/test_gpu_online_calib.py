"""Online calibration: windows whose BSGPU_F_REPROJ_ONLINE_CALIB factors name one extrinsic pair (q_BASELINK_CAM, p_BASELINK_CAM) that
is NOT constant — both blocks free, or one of them — solved on the device with the landmarks still eliminated (csrc/k_calib.hip), against
the CPU oracle on the same IR.

Tolerances are the ones tests/test_gpu_parity.py uses for the same comparisons (test_landmark_blocks_shared_with_other_factors:
residuals / Jacobian / gradient 1e-9 * max(1, |.|max), cost 1e-12 relative, per-iteration cost 1e-8 relative, final cost 1e-6 relative;
test_c1_window: values 1e-6; test_lm_rejected_steps_path: 1e-4 through the first rejected step and the two after it), and the one
tests/test_gpu_covariance_requests.py uses for pose-side pairs (1e-8 of the pair's diagonal scale)."""
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


def _window(n_kf=8, n_lm=60, seed=7, cov=1e-2, **kw):
    return synthetic.vio_window(n_kf=n_kf, n_lm=n_lm, seed=seed, online_calib=True, free_extrinsics=True, calib_prior_cov=cov, **kw)


def _free_the_pair(pr):
    """clears the is_const flags of the extrinsic pair the type-1 factors of a tests/helpers.py graph name"""
    idx = pr.factors[capi.F_REPROJ_ONLINE_CALIB][0][0]
    qe, pe = int(idx[0, 3]), int(idx[0, 4])
    pr.is_const[qe] = 0
    pr.is_const[pe] = 0
    return qe, pe


def _check_evaluate_and_solve(pr, oracle_cls, gpu_solver_cls, value_tol=1e-6, options=None):
    g, o = _pair(pr, oracle_cls, gpu_solver_cls)
    assert [g.tangent_offset(b) for b in range(pr.n_blocks)] == [o.tangent_offset(b) for b in range(pr.n_blocks)]
    assert g.num_parameters_tangent() == o.num_parameters_tangent()
    cg, rg, gg, Jg = g.evaluate(jacobian=True)
    co, ro, go, Jo = o.evaluate(jacobian=True)
    assert np.abs(rg - ro).max() <= 1e-9 * max(1.0, np.abs(ro).max())
    assert np.abs(Jg - Jo).max() <= 1e-9 * max(1.0, np.abs(Jo).max())
    assert abs(cg - co) <= 1e-12 * abs(co)
    assert np.abs(gg - go).max() <= 1e-9 * max(1.0, np.abs(go).max())
    sg, so = g.solve(options), o.solve(options)
    ig, io = g.iterations(), o.iterations()
    assert [i.step_is_successful for i in ig] == [i.step_is_successful for i in io]
    for a, b in zip(ig, io):
        assert abs(a.cost - b.cost) <= 1e-8 * abs(b.cost)
    assert abs(sg.final_cost - so.final_cost) <= 1e-6 * so.final_cost
    assert np.abs(g.get_blocks() - o.get_blocks()).max() < value_tol
    return g, o


# ---- 1. the windows of the issue ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_kf,n_lm,cov", [(20, 500, 1e-5), (20, 500, 1e-2), (8, 60, 1e-2)])
def test_window_matches_oracle(oracle_cls, gpu_solver_cls, n_kf, n_lm, cov):
    pr = _window(n_kf, n_lm, 7, cov)
    qe, pe = pr.meta["ext_blocks"]
    x0 = pr.values.copy()
    g, o = _check_evaluate_and_solve(pr, oracle_cls, gpu_solver_cls)
    assert g.tangent_offset(qe) >= 0 and g.tangent_offset(pe) >= 0
    xg = g.get_blocks()
    assert not np.array_equal(pr.block(pe, xg), pr.block(pe, x0))   # the pair is estimated
    if cov == 1e-2 and n_kf == 20:
        assert np.linalg.norm(pr.block(pe, xg) - pr.block(pe, x0)) > 0.05   # ... and really moves: more than 5 cm
    # the screening quantity at the CURRENT extrinsic values
    idx, consts = pr.factors[capi.F_REPROJ_ONLINE_CALIB][0][:2]
    err = g.reprojection_errors(idx.shape[0])
    R_cb = synthetic.quat_to_rot(pr.block(qe, xg)).T
    t_cb = -R_cb @ pr.block(pe, xg)
    for f in (0, idx.shape[0] // 2, idx.shape[0] - 1):
        R = synthetic.quat_to_rot(pr.block(int(idx[f, 0]), xg))
        Pc = R_cb @ (R.T @ (pr.block(int(idx[f, 2]), xg) - pr.block(int(idx[f, 1]), xg))) + t_cb
        uv = np.array([synthetic.FX * Pc[0] / Pc[2] + synthetic.CX, synthetic.FY * Pc[1] / Pc[2] + synthetic.CY])
        assert abs(err[f] - np.linalg.norm(consts[f, :2] - uv)) <= 1e-9 * max(1.0, err[f])
    # a second solve from the device-resident initial values gives the same answer (the two differ by the order of the border's atomic
    # sums, 1e-16 relative per sum: 1e-9 leaves the amplification the issue measured for this window, 2e-10 per 1e-12, a wide margin)
    first = g.iterations()
    g.reset_values()
    s2 = g.solve()
    assert len(g.iterations()) == len(first)
    assert abs(s2.final_cost - first[-1].cost) <= 1e-9 * first[-1].cost


@pytest.mark.parametrize("seed", [1, 9])
def test_rejected_steps_path(oracle_cls, gpu_solver_cls, seed):
    """Random measurements, the pair freed: rejected steps.  Compared as test_gpu_parity.py::test_lm_rejected_steps_path compares."""
    pr = mixed_problem(seed, n_state=4, n_lm=16)
    _free_the_pair(pr)
    g, o = _pair(pr, oracle_cls, gpu_solver_cls)
    opt = g.options_default()
    opt.max_num_iterations = 9
    g.solve(opt), o.solve(opt)
    ig, io = g.iterations(), o.iterations()
    first_rej = next(i for i, a in enumerate(io) if not a.step_is_successful)
    upto = min(len(ig), len(io), first_rej + 3)
    assert upto > first_rej
    for a, b in zip(ig[:upto], io[:upto]):
        assert a.step_is_successful == b.step_is_successful
        assert abs(a.cost - b.cost) <= 1e-4 * abs(b.cost)
        assert abs(a.trust_region_radius - b.trust_region_radius) <= 1e-4 * b.trust_region_radius
        assert abs(a.model_cost_change - b.model_cost_change) <= 1e-4 * abs(b.model_cost_change) + 1e-12


# ---- 2. the shapes around it -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "p"])
def test_one_block_of_the_pair_free(oracle_cls, gpu_solver_cls, which):
    pr = _window()
    qe, pe = pr.meta["ext_blocks"]
    held = pe if which == "q" else qe
    pr.is_const[held] = 1
    x0 = pr.values.copy()
    g, _ = _check_evaluate_and_solve(pr, oracle_cls, gpu_solver_cls)
    assert g.tangent_offset(held) == -1 and g.tangent_offset(qe if which == "q" else pe) >= 0
    assert np.array_equal(pr.block(held, g.get_blocks()), pr.block(held, x0))


def test_held_first_key_frame(oracle_cls, gpu_solver_cls):
    pr = _window()
    kf = pr.meta["kf_blocks"]
    pr.is_const[int(kf[0, 0])] = 1
    pr.is_const[int(kf[0, 1])] = 1
    _check_evaluate_and_solve(pr, oracle_cls, gpu_solver_cls)


def test_constant_landmarks_among_the_observed(oracle_cls, gpu_solver_cls):
    pr = _window()
    for b in pr.meta["lm_blocks"][::5]:
        pr.is_const[int(b)] = 1
    _check_evaluate_and_solve(pr, oracle_cls, gpu_solver_cls)


def test_type0_and_type1_factors_on_the_same_landmarks(oracle_cls, gpu_solver_cls):
    """tests/helpers.py: a quarter of the observations are type-1 factors, on landmarks the type-0 factors see too."""
    pr = mixed_problem(9, n_state=4, n_lm=16, with_losses=True, consistent=True)
    qe, pe = _free_the_pair(pr)
    A = synthetic.sqrt_information_upper(1e-2 * np.eye(6))
    pr.add_factors(capi.F_ABSPOSE, [[pe, qe]], [np.concatenate([pr.block(pe), pr.block(qe), A.ravel()])])
    _check_evaluate_and_solve(pr, oracle_cls, gpu_solver_cls, value_tol=1e-7)


# ---- 3. the calibration's own uncertainty ------------------------------------------------------------------------------------------
def test_covariance_of_the_pair(oracle_cls, gpu_solver_cls):
    pr = _window(20, 500, 7, 1e-2)
    g, o = _pair(pr, oracle_cls, gpu_solver_cls)
    assert o.num_parameters_tangent() <= 4000
    g.solve(); o.set_values(g.get_blocks())
    qe, pe = pr.meta["ext_blocks"]
    kf = pr.meta["kf_blocks"]
    pairs = [(pe, pe), (qe, qe), (pe, qe), (int(kf[10, 1]), pe), (int(kf[3, 0]), int(kf[3, 1]))]
    got = g.covariance_requests(pairs)
    for (a, b), cg in zip(pairs, got):
        co = o.covariance(int(a), int(b), 3, 3)
        caa, cbb = o.covariance(int(a), int(a), 3, 3), o.covariance(int(b), int(b), 3, 3)
        scale = max(np.abs(co).max(), np.sqrt(np.abs(caa).max() * np.abs(cbb).max()))
        assert np.abs(cg - co).max() <= 1e-8 * scale, (a, b, np.abs(cg - co).max(), scale)
    # the single-pair and joint entry points see the same system
    c1 = g.covariance(pe, qe)
    assert np.abs(c1 - got[2]).max() <= 1e-8 * np.sqrt(np.abs(got[0]).max() * np.abs(got[1]).max())
    cj = g.covariance_joint([qe, pe], [3, 3])
    assert np.abs(cj[3:, 3:] - got[0]).max() <= 1e-8 * np.abs(got[0]).max()
    assert np.abs(cj[:3, :3] - got[1]).max() <= 1e-8 * np.abs(got[1]).max()


# ---- 4. among other windows --------------------------------------------------------------------------------------------------------
def test_solve_batch_equals_lone_solves(gpu_solver_cls):
    prs = [_window(8, 60, 7), _window(10, 120, 8), synthetic.vio_window(n_kf=8, n_lm=60, seed=5)]
    lone = []
    for pr in prs:
        g = gpu_solver_cls(0)
        pr.load(g)
        s = g.solve()
        lone.append((s, g.get_blocks()))
    batch = []
    for pr in prs:
        g = gpu_solver_cls(0)
        pr.load(g)
        batch.append(g)
    sums = gpu_solver_cls.solve_batch(batch)
    for (s0, x0), s1, g in zip(lone, sums, batch):
        assert s1.num_iterations == s0.num_iterations
        assert abs(s1.final_cost - s0.final_cost) <= 1e-8 * s0.final_cost
        assert np.abs(g.get_blocks() - x0).max() < 1e-6


# ---- 5. what is refused, and why ---------------------------------------------------------------------------------------------------
def _refused(call, fragment):
    with pytest.raises(capi.SolverError) as e:
        call()
    assert e.value.code == capi.ERR_UNSUPPORTED, str(e.value)
    assert fragment in str(e.value), str(e.value)


def test_refusals(gpu_solver_cls):
    # two free pairs
    pr = _window()
    qe, pe = pr.meta["ext_blocks"]
    q2, p2 = pr.add_quat(pr.block(qe)), pr.add_block(pr.block(pe))
    idx = pr.factors[capi.F_REPROJ_ONLINE_CALIB][0][0]
    idx[::2, 3] = q2
    idx[::2, 4] = p2
    g = gpu_solver_cls(0)
    pr.load(g)
    _refused(g.finalize, "more than one free extrinsic pair")
    # a landmark that is not eliminated
    pr = _window()
    b = int(pr.meta["lm_blocks"][3])
    A = synthetic.sqrt_information_upper(0.01 * np.eye(3))
    pr.add_factors(capi.F_ABS_VEC3, [[b]], [np.concatenate([pr.block(b) + 0.02, A.ravel()])])
    g = gpu_solver_cls(0)
    pr.load(g)
    _refused(g.finalize, "landmark block is not eliminated")
    # a factor of the free pair whose pose and landmark blocks are all constant
    pr = _window()
    row = pr.factors[capi.F_REPROJ_ONLINE_CALIB][0][0][0]
    for b in row[:3]:
        pr.is_const[int(b)] = 1
    g = gpu_solver_cls(0)
    pr.load(g)
    _refused(g.finalize, "pose and landmark blocks are all constant")
    # strategies and linear solvers
    pr = _window()
    g = gpu_solver_cls(0)
    pr.load(g)
    opt = g.options_default()
    opt.trust_region_strategy_type = capi.TR_DOGLEG
    _refused(lambda: g.solve(opt), "free extrinsic pair")
    for lin in (capi.LINEAR_PCG, capi.LINEAR_SCHUR_PCG):
        opt = g.options_default()
        opt.linear_solver_type = lin
        _refused(lambda: g.solve(opt), "free extrinsic pair")
    # marginalisation, landmark covariances
    kf = pr.meta["kf_blocks"]
    _refused(lambda: g.marginalize([int(b) for b in kf[0]], pr.size), "free extrinsic pair")
    lm = int(pr.meta["lm_blocks"][0])
    _refused(lambda: g.covariance_requests([(lm, lm)]), "free extrinsic pair")
    _refused(lambda: g.covariance_requests([(pr.meta["ext_blocks"][1], lm)]), "free extrinsic pair")
    # ... and the window still solves
    assert g.solve().is_solution_usable == 1


# ---- 6. what does not change -------------------------------------------------------------------------------------------------------
def test_constant_pair_is_the_type0_window_on_the_equivalent_camera(gpu_solver_cls):
    """Both blocks constant (what the reference's holdConstant() gives): the derived camera is folded at finalize(), as before."""
    pr1 = synthetic.vio_window(n_kf=20, n_lm=500, seed=7, online_calib=True, free_extrinsics=False)
    qe, pe = pr1.meta["ext_blocks"]
    pr0 = synthetic.vio_window(n_kf=20, n_lm=500, seed=7)
    R_cb = synthetic.quat_to_rot(pr1.block(qe)).T
    t_cb = -R_cb @ pr1.block(pe)
    pr0.cameras[0].R_cam_baselink[:] = list(R_cb.ravel())
    pr0.cameras[0].t_cam_baselink[:] = list(t_cb)
    g1, g0 = gpu_solver_cls(0), gpu_solver_cls(0)
    pr1.load(g1)
    pr0.load(g0)
    assert g1.plan_info() == g0.plan_info()
    assert g1.tangent_offset(qe) == -1 and g1.tangent_offset(pe) == -1
    s1, s0 = g1.solve(), g0.solve()
    assert s1.num_iterations == s0.num_iterations
    for a, b in zip(g1.iterations(), g0.iterations()):
        assert abs(a.cost - b.cost) <= 1e-8 * abs(b.cost)
