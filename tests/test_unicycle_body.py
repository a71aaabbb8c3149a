"""BSGPU_F_UNICYCLE on the CPU: the type's table sizes through the C-ABI, and the shared host/device body
(beam_slam_amd/csrc/unicycle_body.h, compiled with g++) against an independent dual-number restatement of the reference functor
(tests/unicycle_ref.py) and against central differences on the manifold."""
import ctypes
import math

import numpy as np
import pytest

from beam_slam_amd import capi, gpu, problem
import unicycle_ref as U


def test_type_sizes_through_the_c_abi():
    lib = ctypes.CDLL(gpu.LIB_PATH)
    assert capi.F_UNICYCLE == 12 and capi.F_NUM_TYPES == 13
    assert (lib.bsgpu_nidx(capi.F_UNICYCLE), lib.bsgpu_nconst(capi.F_UNICYCLE), lib.bsgpu_nres(capi.F_UNICYCLE)) == (10, 226, 15)
    assert (problem.NIDX[capi.F_UNICYCLE], problem.NCONST[capi.F_UNICYCLE], problem.NRES[capi.F_UNICYCLE]) == (10, 226, 15)
    assert lib.bsgpu_nidx(capi.F_NUM_TYPES) == -1
    for t in range(capi.F_NUM_TYPES):
        assert (lib.bsgpu_nidx(t), lib.bsgpu_nconst(t), lib.bsgpu_nres(t)) == (problem.NIDX[t], problem.NCONST[t], problem.NRES[t])


def _quat(rng, norm_jitter=0.05):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q) * rng.uniform(1 - norm_jitter, 1 + norm_jitter)


def _state(rng, q):
    return np.concatenate([rng.normal(0, 2, 3), q, rng.normal(0, 1, 3), rng.normal(0, 0.5, 3), rng.normal(0, 0.5, 3)])


def _pitch_quat(theta, yaw=0.3, scale=1.0):
    """q = Rz(yaw) Ry(theta): s = 2(wy - zx) = scale^2 sin(theta)"""
    qy = np.array([math.cos(theta / 2), 0, math.sin(theta / 2), 0])
    qz = np.array([math.cos(yaw / 2), 0, 0, math.sin(yaw / 2)])
    w1, x1, y1, z1 = qz
    w2, x2, y2, z2 = qy
    q = np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                  w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
    return scale * q


def _yaw_quat(yaw, rng):
    return _pitch_quat(rng.normal(0, 0.1), yaw) * rng.uniform(0.97, 1.03)


def _cases():
    rng = np.random.default_rng(11)
    out = []
    for _ in range(40):                     # random states, |q| != 1
        out.append(("random", np.concatenate([_state(rng, _quat(rng)), _state(rng, _quat(rng))]), rng.uniform(0.01, 0.5)))
    for th in (math.pi / 2 - 1e-3, -math.pi / 2 + 1e-3, math.pi / 2 - 1e-4, -math.pi / 2 + 1e-4):   # pitch near +-pi/2
        out.append(("near_pole", np.concatenate([_state(rng, _pitch_quat(th)), _state(rng, _quat(rng))]), 0.1))
        out.append(("near_pole2", np.concatenate([_state(rng, _quat(rng)), _state(rng, _pitch_quat(th))]), 0.1))
    for th, sc in ((math.pi / 2, 1.01), (-math.pi / 2, 1.02), (math.pi / 2 - 1e-3, 1.01)):           # |s| >= 1: the clamp
        out.append(("clamped", np.concatenate([_state(rng, _pitch_quat(th, scale=sc)), _state(rng, _pitch_quat(-th, scale=sc))]), 0.1))
    for y1, y2 in ((math.pi - 0.02, -math.pi + 0.03), (-math.pi + 0.01, math.pi - 0.04), (math.pi - 0.001, math.pi - 0.05)):
        x = np.concatenate([_state(rng, _yaw_quat(y1, rng)), _state(rng, _yaw_quat(y2, rng))])
        x[10:13] = [0.0, 0.0, 0.6]         # yaw rate: the prediction crosses +-pi too
        out.append(("yaw_wrap", x, 0.1))
    return out


def test_body_matches_dual_restatement(tmp_path):
    ev = U.body_lib(tmp_path)
    wraps = 0
    for kind, x, dt in _cases():
        e, J = ev(x, dt)
        e_ref, J_ref = U.error_and_jacobian(x, dt)
        assert np.abs(e - e_ref).max() <= 1e-13 * np.abs(e_ref).max(), (kind, e, e_ref)
        assert np.abs(J - J_ref).max() <= 1e-11 * np.abs(J_ref).max(), (kind, np.abs(J - J_ref).max())
        if kind == "clamped":
            assert np.all(J[4, 18:21] == 0.0)   # (pitch(q2) is +-pi/2 with a zero derivative)
        if kind == "yaw_wrap":
            r1 = math.atan2(2 * (x[3] * x[6] + x[4] * x[5]), 1 - 2 * (x[5] ** 2 + x[6] ** 2))
            wraps += abs(r1 + 0.6 * dt) > math.pi
            assert abs(e[5]) < 0.2, e[5]
    assert wraps >= 1


def test_body_matches_central_differences(tmp_path):
    ev = U.body_lib(tmp_path)
    for kind, x, dt in _cases():
        s1, s2 = 2 * (x[3] * x[5] - x[6] * x[4]), 2 * (x[19] * x[21] - x[22] * x[20])
        if max(abs(s1), abs(s2)) > 1 - 1e-5:
            continue   # (at the clamp or within a step of it the function is flat or steeper than any difference resolves)
        _, J = ev(x, dt)
        Jf = U.fd_jacobian(x, dt)
        assert np.abs(J - Jf).max() <= 1e-6 * np.abs(J).max(), (kind, np.abs(J - Jf).max(), np.abs(J).max())
