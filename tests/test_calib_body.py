"""The extrinsic columns of the online-calibration reprojection factor on the CPU: the shared host/device body
(beam_slam_amd/csrc/calib_body.h, compiled with g++) against the oracle's dense Jacobian — the functor on Jets — for the two extrinsic
blocks, Cauchy / Huber / trivial loss, both blocks free or either one constant.  Bound: 1e-9 * max(1, |J|max), the bound
tests/test_gpu_parity.py puts on every Jacobian."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from beam_slam_amd import capi, synthetic
from beam_slam_amd.problem import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def calib_eval(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("calib_body")), "calib_body.so")
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                          os.path.join(ROOT, "tests", "plan", "calib_body_capi.cpp"), "-o", so], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    lib = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.calib_eval.argtypes = [dp] * 7 + [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, dp]

    def ev(q_wb, t_wb, P, q_bc, p_bc, K, uvw, loss_kind, loss_a, theta_free, p_free):
        a = [np.ascontiguousarray(v, float) for v in (q_wb, t_wb, P, q_bc, p_bc, K, uvw)]
        E = np.zeros(12)
        lib.calib_eval(*[v.ctypes.data_as(dp) for v in a], int(loss_kind), float(loss_a), int(theta_free), int(p_free), E.ctypes.data_as(dp))
        return E.reshape(2, 6)
    return ev


def _problem(seed, const_q, const_p):
    """A few poses and landmarks seen through one extrinsic pair; a third of the factors each with Cauchy, Huber and no loss."""
    rng = np.random.default_rng(seed)
    pr = Problem()
    R_cb, t_cb = synthetic._t_cam_baselink()
    cam = pr.add_camera(synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY, R_cb, t_cb)
    n_pose, n_lm = 4, 12
    q_t = [synthetic.quat_from_aa(rng.normal(0, 0.2, 3)) for _ in range(n_pose)]
    p_t = [rng.normal(0, 0.5, 3) for _ in range(n_pose)]
    poses = [(pr.add_quat(synthetic._perturb_quat(q_t[i], rng, 0.01)), pr.add_block(p_t[i] + rng.normal(0, 0.03, 3))) for i in range(n_pose)]
    T_bc = synthetic.T_IMU_CAM
    qe = pr.add_quat(synthetic._perturb_quat(synthetic.rot_to_quat(T_bc[:3, :3]), rng, 0.02), const=const_q)
    pe = pr.add_block(T_bc[:3, 3] + rng.normal(0, 0.03, 3), const=const_p)
    rows = {capi.LOSS_TRIVIAL: ([], []), capi.LOSS_CAUCHY: ([], []), capi.LOSS_HUBER: ([], [])}
    kinds = list(rows)
    n = 0
    for j in range(n_lm):
        k = int(rng.integers(0, n_pose))
        Pc = np.array([rng.uniform(-1, 1), rng.uniform(-0.7, 0.7), rng.uniform(4, 9)])
        Pw = synthetic.quat_to_rot(q_t[k]) @ (R_cb.T @ (Pc - t_cb)) + p_t[k]
        b = pr.add_block(Pw + rng.normal(0, 0.05, 3))
        for kk in range(n_pose):
            Pck = R_cb @ (synthetic.quat_to_rot(q_t[kk]).T @ (Pw - p_t[kk])) + t_cb
            if Pck[2] < 1.0:
                continue
            uv = np.array([synthetic.FX * Pck[0] / Pck[2] + synthetic.CX, synthetic.FY * Pck[1] / Pck[2] + synthetic.CY])
            idx, cs = rows[kinds[n % 3]]
            idx.append([poses[kk][0], poses[kk][1], b, qe, pe, cam])
            cs.append([*(uv + rng.normal(0, 3.0, 2)), rng.uniform(0.5, 2.0)])   # (errors on both sides of the Huber / Cauchy scale)
            n += 1
    for kind, (idx, cs) in rows.items():
        pr.add_factors(capi.F_REPROJ_ONLINE_CALIB, idx, cs, kind, 2.0)
    return pr, qe, pe


@pytest.mark.parametrize("const_q,const_p", [(False, False), (True, False), (False, True)])
def test_extrinsic_columns_match_the_oracle(calib_eval, oracle_cls, const_q, const_p):
    n_checked = 0
    for seed in (3, 4, 5):
        pr, qe, pe = _problem(seed, const_q, const_p)
        o = oracle_cls()
        pr.load(o)
        _, _, _, J = o.evaluate(jacobian=True)
        tq, tp = o.tangent_offset(qe), o.tangent_offset(pe)
        assert (tq < 0) == const_q and (tp < 0) == const_p
        scale = max(1.0, np.abs(J).max())
        x = pr.values
        K = [synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY]
        row = 0
        for idx, consts, lk, la in pr.factors[capi.F_REPROJ_ONLINE_CALIB]:
            for f in range(idx.shape[0]):
                E = calib_eval(pr.block(int(idx[f, 0]), x), pr.block(int(idx[f, 1]), x), pr.block(int(idx[f, 2]), x), pr.block(qe, x),
                               pr.block(pe, x), K, consts[f], lk[f], la[f], not const_q, not const_p)
                if not const_q:
                    assert np.abs(E[:, :3] - J[row:row + 2, tq:tq + 3]).max() <= 1e-9 * scale
                else:
                    assert np.all(E[:, :3] == 0.0)
                if not const_p:
                    assert np.abs(E[:, 3:] - J[row:row + 2, tp:tp + 3]).max() <= 1e-9 * scale
                else:
                    assert np.all(E[:, 3:] == 0.0)
                row += 2
                n_checked += 1
    assert n_checked >= 100
