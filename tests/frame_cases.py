"""Seeded frame-localisation cases (bsgpu_localize_frames, beam_slam_amd/csrc/frame_lm.h) and their oracle answer: the same frame as a
one-pose BSGPU_F_REPROJ problem (free orientation and position blocks, constant landmark blocks) solved by the CPU oracle.

Shared by tests/test_frame_lm.py (the core on the CPU) and tests/test_gpu_localize_frames.py (the kernel)."""
import numpy as np

from beam_slam_amd import capi
from beam_slam_amd.problem import Problem

K = (458.654, 457.296, 367.215, 248.375)
WIDTH, HEIGHT = 752, 480
# baselink x forward / z up -> camera z forward / y down, tilted a little, offset from the baselink (a non-identity T_cam_baselink)
_R0 = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rot_to_quat(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.copysign(np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    q = np.array([w, x, y, z])
    return q / np.linalg.norm(q)


R_CB = _rot([0.3, 1.0, -0.2], 0.04) @ _R0
T_CB = np.array([0.05, -0.02, 0.1])


def camera():
    c = capi.Camera()
    c.fx, c.fy, c.cx, c.cy = K
    c.R_cam_baselink[:] = list(R_CB.ravel())
    c.t_cam_baselink[:] = list(T_CB)
    return c


def project(q, p, P):
    """pi(K, T_cam_baselink T_world_baselink^-1 P) for points P (n x 3): (uv (n x 2), depth (n))."""
    Pb = (np.asarray(P) - p) @ quat_to_rot(q)
    Pc = Pb @ R_CB.T + T_CB
    fx, fy, cx, cy = K
    return np.stack([fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy], 1), Pc[:, 2]


def make_frame(seed, n_obs, rot_deg, trans_m, noise_px=0.5, outlier_frac=0.0):
    rng = np.random.default_rng(seed)
    q_true = rot_to_quat(_rot(rng.normal(size=3), rng.uniform(0, np.pi)))
    p_true = rng.normal(size=3) * 5.0
    fx, fy, cx, cy = K
    u, v = rng.uniform(0, WIDTH, n_obs), rng.uniform(0, HEIGHT, n_obs)
    z = rng.uniform(2.0, 20.0, n_obs)
    Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Pb = (Pc - T_CB) @ R_CB
    P = Pb @ quat_to_rot(q_true).T + p_true
    uv, _ = project(q_true, p_true, P)
    pix = uv + rng.normal(scale=noise_px, size=uv.shape)
    n_out = int(round(outlier_frac * n_obs))
    if n_out:
        k = rng.choice(n_obs, n_out, replace=False)
        pix[k] = np.stack([rng.uniform(0, WIDTH, n_out), rng.uniform(0, HEIGHT, n_out)], 1)
    q_init = rot_to_quat(quat_to_rot(q_true) @ _rot(rng.normal(size=3), np.deg2rad(rot_deg)))
    d = rng.normal(size=3)
    p_init = p_true + trans_m * d / np.linalg.norm(d)
    return dict(pixels=pix, points=P, q_init=q_init, p_init=p_init, q_true=q_true, p_true=p_true)


def oracle_localize(oracle_cls, fr, loss_kind, loss_a, w, opts, truncate=False):
    """The frame as a one-pose BSGPU_F_REPROJ problem through the oracle: pose, cost, iterations, trace (0 invalid, 1 rejected,
    2 accepted per recorded iteration) and the covariance of [p, q tangent] (6 x 6)."""
    pr = Problem()
    pr.add_camera(*K, R_CB, T_CB)
    qb = pr.add_quat(fr["q_init"])
    pb = pr.add_block(fr["p_init"])
    lms = pr.add_blocks(fr["points"], const=True)
    pix = np.trunc(fr["pixels"]) if truncate else fr["pixels"]
    n = len(lms)
    idx = np.stack([np.full(n, qb), np.full(n, pb), lms, np.zeros(n, np.int32)], 1)
    pr.add_factors(capi.F_REPROJ, idx, np.concatenate([pix, np.full((n, 1), w)], 1), loss_kind, loss_a)
    o = oracle_cls(threads=1)
    pr.load(o)
    s = o.solve(opts)
    x = o.get_blocks()
    its = o.iterations()
    trace = [0 if not it.step_is_valid else (2 if it.step_is_successful else 1) for it in its[1:]]
    cov = np.full((6, 6), np.nan)
    try:
        cov[:3, :3] = o.covariance(pb, pb)
        cov[:3, 3:] = o.covariance(pb, qb)
        cov[3:, :3] = o.covariance(qb, pb)
        cov[3:, 3:] = o.covariance(qb, qb)
    except capi.SolverError:
        pass
    return dict(q=x[pr.offset[qb]:pr.offset[qb] + 4], p=x[pr.offset[pb]:pr.offset[pb] + 3], cost=s.final_cost,
                iterations=s.num_iterations, trace=trace, cov=cov, usable=s.is_solution_usable)


def options(oracle_cls, kind="default"):
    o = oracle_cls(threads=1)
    opts = o.options_vio() if kind == "vio" else o.options_default()
    o.close()
    if kind == "vio":
        opts.max_solver_time_in_seconds = 0.0
    return opts


#: (seed, n_obs, rotation deg, translation m, loss kind, loss a, options kind, outlier fraction)
CASES = [
    (1, 20, 1.0, 0.05, capi.LOSS_TRIVIAL, 1.0, "default", 0.0),
    (2, 60, 3.0, 0.1, capi.LOSS_HUBER, 2.0, "default", 0.0),
    (3, 200, 5.0, 0.3, capi.LOSS_CAUCHY, 1.0, "default", 0.0),
    (4, 500, 2.0, 0.2, capi.LOSS_HUBER, 1.0, "vio", 0.0),
    (5, 2000, 4.0, 0.15, capi.LOSS_TRIVIAL, 1.0, "vio", 0.0),
    (6, 1000, 5.0, 0.3, capi.LOSS_CAUCHY, 2.0, "default", 0.0),
    (7, 33, 2.5, 0.25, capi.LOSS_CAUCHY, 0.5, "vio", 0.0),
    (8, 300, 4.0, 0.2, capi.LOSS_CAUCHY, 1.0, "default", 0.2),
]


def compare(got, ref, tag):
    """The CPU test's and the GPU test's tolerances against the oracle."""
    assert got["iterations"] == ref["iterations"], (tag, got["iterations"], ref["iterations"])
    if "trace" in got:
        assert list(got["trace"]) == list(ref["trace"]), (tag, got["trace"], ref["trace"])
    assert abs(got["cost"] - ref["cost"]) <= 1e-10 * abs(ref["cost"]), (tag, got["cost"], ref["cost"])
    qg, qo = np.asarray(got["q"]), np.asarray(ref["q"])
    assert min(np.abs(qg - qo).max(), np.abs(qg + qo).max()) <= 1e-9, (tag, qg, qo)
    assert np.abs(np.asarray(got["p"]) - ref["p"]).max() <= 1e-9, (tag, got["p"], ref["p"])
    scale = np.abs(np.diag(ref["cov"])).max()
    assert np.abs(np.asarray(got["cov"]) - ref["cov"]).max() <= 1e-8 * scale, (tag, np.abs(got["cov"] - ref["cov"]).max(), scale)
