"""Independent NumPy restatement of bsgpu_absolute_pose_ransac (include/bsgpu.h) and of beam_slam_amd/csrc/p3p.h, in the manner of
essential_ref.py: nothing here is transcribed from the header, and the minimal solver takes another route than the header's.

* p3p(): the three law-of-cosines equations s_i^2 + s_j^2 - 2 s_i s_j c_ij = d_ij^2 with s1^2 eliminated: two conics in
  (u, v) = (s2 / s1, s3 / s1), their resultant in u — a quartic in v — from numpy.polynomial arithmetic, its roots from
  numpy.polynomial's companion matrix (real when LAPACK returns a zero imaginary part), u from the linear remainder of the two
  conics, the pose of each depth triple by Kabsch / SVD.  Solutions with all depths positive, in ascending depth of the first point.
* reproj_sq(), sample_indices() (splitmix64 in Python integers), update_niters() and ransac_serial(): the contract's serial loop.
* the seeded case generators shared by tests/test_p3p.py, tests/test_gpu_absolute_pose_ransac.py and
  scripts/time_absolute_pose_ransac.py."""
import math

import numpy as np
from numpy.polynomial import Polynomial as Poly

K_DEFAULT = (458.654, 457.296, 367.215, 248.375)   # configuration C2's pinhole intrinsics (beam_slam_amd/synthetic.py)
WIDTH, HEIGHT = 752, 480
M64 = (1 << 64) - 1
STATUS_OK, STATUS_TOO_FEW, STATUS_NO_MODEL = 0, 1, 2


# ---- minimal solver ------------------------------------------------------------------------------------------------------------
def bearings(px, K):
    fx, fy, cx, cy = K
    px = np.asarray(px, float).reshape(-1, 2)
    b = np.column_stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(len(px))])
    return b / np.linalg.norm(b, axis=1)[:, None]


def kabsch(P, Q):
    """R, t of Q = R P + t in the least-squares sense (rows are points)."""
    pc, qc = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - qc).T @ (P - pc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, qc - R @ pc


def p3p(px, P, K, with_roots=False):
    """All poses (R, t) of T_CAMERA_WORLD with positive depths for three pixel / world-point pairs, in ascending camera-frame z of
    the first point.  with_roots: also the real and complex roots of the quartic."""
    P = np.asarray(P, float).reshape(3, 3)
    y = bearings(px, K)
    c12, c13, c23 = y[0] @ y[1], y[0] @ y[2], y[1] @ y[2]
    a12, a13, a23 = np.sum((P[0] - P[1]) ** 2), np.sum((P[0] - P[2]) ** 2), np.sum((P[1] - P[2]) ** 2)
    v = Poly([0.0, 1.0])
    A1, B1, C1 = Poly([a23 - a12]), -2.0 * a23 * c12 + 2.0 * a12 * c23 * v, a23 - a12 * v * v
    A2, B2, C2 = Poly([-a13]), 2.0 * a13 * c23 * v, a23 * (1.0 + v * v - 2.0 * c13 * v) - a13 * v * v
    res = (A1 * C2 - A2 * C1) ** 2 - (A1 * B2 - A2 * B1) * (B1 * C2 - B2 * C1)
    roots = res.roots() if res.degree() >= 1 and np.all(np.isfinite(res.coef)) else np.array([])
    sols = []
    for r in roots:
        if np.imag(r) != 0.0 or not np.real(r) > 0.0:
            continue
        vv = float(np.real(r))
        den = (A2 * B1 - A1 * B2)(vv)
        if den == 0.0:
            continue
        u = float((A1 * C2 - A2 * C1)(vv) / den)
        q = 1.0 + u * u - 2.0 * u * c12
        if not (u > 0.0 and q > 0.0):
            continue
        s1 = math.sqrt(a12 / q)
        s = np.array([s1, u * s1, vv * s1])
        R, t = kabsch(P, y * s[:, None])
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
            sols.append((R, t))
    sols.sort(key=lambda Rt: (Rt[0] @ P[0] + Rt[1])[2])
    return (sols, roots) if with_roots else sols


def near_double(roots, rel=1e-3):
    """Two roots of the quartic (complex ones included: a pair about to meet on the real axis) within a relative `rel`."""
    r = np.asarray(roots, complex)
    for i in range(len(r)):
        for j in range(i + 1, len(r)):
            if abs(r[i] - r[j]) <= rel * max(abs(r[i]), abs(r[j])):
                return True
    return False


def constraint_residual(R, t, px, P, K):
    """Largest | |R P_i + t| y_i - (R P_i + t) | over the three pairs, relative to the depth: 0 for an exact solution."""
    Pc = np.asarray(P, float).reshape(3, 3) @ R.T + t
    y = bearings(px, K)
    d = np.linalg.norm(Pc, axis=1)
    return float(np.max(np.linalg.norm(y * d[:, None] - Pc, axis=1) / d))


def pose_dist(Rt, R_true, t_true):
    return max(np.abs(Rt[0] - R_true).max(), np.abs(Rt[1] - t_true).max())


# ---- error, sampler, loop ------------------------------------------------------------------------------------------------------
def reproj_sq(R, t, K, px, P):
    """|z - pi(K, R P + t)|^2 per pair; inf for a point not in front of the camera."""
    fx, fy, cx, cy = K
    Pc = np.asarray(P, float).reshape(-1, 3) @ R.T + t
    px = np.asarray(px, float).reshape(-1, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = (fx * Pc[:, 0] / Pc[:, 2] + cx - px[:, 0]) ** 2 + (fy * Pc[:, 1] / Pc[:, 2] + cy - px[:, 1]) ** 2
    return np.where(Pc[:, 2] > 0.0, e, np.inf)


def sample_indices(seed, frame_index, sample_index, n):
    state = (seed ^ ((frame_index * 0x9E3779B97F4A7C15) & M64) ^ ((sample_index * 0xBF58476D1CE4E5B9) & M64)) & M64
    out = []
    while len(out) < 3:
        state = (state + 0x9E3779B97F4A7C15) & M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        i = z % n
        if i not in out:
            out.append(int(i))
    return out


def update_niters(p, ep, niters):
    num = math.log(1.0 - p)
    t = 1.0 - (1.0 - ep) ** 3
    den = math.log(t) if t > 0.0 else -math.inf
    if den >= 0.0 or -num >= niters * (-den):
        return niters
    return int(round(num / den))


def ransac_serial(px, P, K, prob=0.0, threshold_px=5.0, max_iters=100, seed=0, frame_index=0, truncate=False):
    """The contract's serial loop for one frame -> dict(mask uint8 (n), R, t (T_CAMERA_WORLD; NaN without a model), n_inliers,
    n_iters, best_sample (3), status, err (squared pixel error of the best model per pair), thr2)."""
    px = np.asarray(px, float).reshape(-1, 2)
    if truncate:
        px = np.trunc(px)
    P = np.asarray(P, float).reshape(-1, 3)
    n = len(px)
    out = dict(mask=np.zeros(n, np.uint8), R=np.full((3, 3), np.nan), t=np.full(3, np.nan), n_inliers=0, n_iters=0,
               best_sample=-np.ones(3, np.int32), status=STATUS_TOO_FEW, err=None, thr2=threshold_px * threshold_px)
    if n < 4:
        return out
    thr2 = threshold_px * threshold_px
    niters, best, s = max_iters, 0, 0
    out["status"] = STATUS_NO_MODEL
    while s < niters:
        idx = sample_indices(seed, frame_index, s, n)
        for R, t in p3p(px[idx], P[idx], K):
            err = reproj_sq(R, t, K, px, P)
            inl = err < thr2
            good = int(inl.sum())
            if good > max(best, 3):
                best = good
                out.update(mask=inl.astype(np.uint8), R=R, t=t, n_inliers=good, best_sample=np.array(idx, np.int32), status=STATUS_OK,
                           err=err)
                if 0.0 < prob < 1.0:
                    niters = update_niters(prob, (n - good) / n, niters)
        s += 1
    out["n_iters"] = s
    return out


# ---- poses ---------------------------------------------------------------------------------------------------------------------
def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, float) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def baselink_pose(R_cw, t_cw, R_cb, t_cb):
    """T_WORLD_BASELINK = T_CAMERA_WORLD^-1 T_cam_baselink -> (R_wb, p)."""
    return R_cw.T @ R_cb, R_cw.T @ (np.asarray(t_cb) - t_cw)


def baselink_dist(q, p, R_wb, p_wb):
    return max(np.abs(quat_to_rot(q) - R_wb).max(), np.abs(np.asarray(p) - p_wb).max())


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def make_pose(rng):
    """T_CAMERA_WORLD: any rotation, the world origin a few metres off."""
    w = rng.normal(size=3)
    w *= rng.uniform(0.0, math.pi) / np.linalg.norm(w)
    return rodrigues(w), rng.normal(size=3) * 3.0


def make_pairs(rng, n, R, t, K=K_DEFAULT):
    """n noise-free pixel / world-point pairs: pixels uniform over the image, depth U[3, 15]."""
    fx, fy, cx, cy = K
    u, v, d = rng.uniform(0, WIDTH, n), rng.uniform(0, HEIGHT, n), rng.uniform(3.0, 15.0, n)
    Pc = np.column_stack([(u - cx) / fx * d, (v - cy) / fy * d, d])
    return np.column_stack([u, v]), (Pc - t) @ R


def make_frame(seed, n, n_out, K=K_DEFAULT, truncate=False, behind_frac=0.25):
    """A seeded frame -> dict(pixels, points, labels (1 inlier), R, t (true T_CAMERA_WORLD), K, behind (bool per pair)).  An outlier
    keeps its world point and gets a pixel drawn uniformly at least 10 px from the true projection; about behind_frac of the
    outliers instead get a world point behind the camera (and keep a pixel inside the image)."""
    rng = np.random.default_rng(seed)
    R, t = make_pose(rng)
    pix, pts = make_pairs(rng, n, R, t, K)
    labels = np.ones(n, np.uint8)
    behind = np.zeros(n, bool)
    for j, i in enumerate(rng.permutation(n)[:n_out]):
        labels[i] = 0
        if j < behind_frac * n_out:
            Pc = pts[i] @ R.T + t
            Pc[2] = -rng.uniform(0.5, 15.0)
            pts[i] = (Pc - t) @ R
            behind[i] = True
            continue
        while True:
            c = np.array([rng.uniform(0, WIDTH), rng.uniform(0, HEIGHT)])
            if np.linalg.norm(c - pix[i]) >= 10.0:
                pix[i] = c
                break
    if truncate:
        pix = np.trunc(pix)
    return dict(pixels=pix, points=pts, labels=labels, R=R, t=t, K=K, behind=behind)


def make_random_frame(seed, n, K=K_DEFAULT):
    rng = np.random.default_rng(seed)
    return dict(pixels=rng.uniform(0, [WIDTH, HEIGHT], size=(n, 2)), points=rng.normal(size=(n, 3)) * 5.0 + [0, 0, 8.0], K=K)


def minimal_case(seed, K=K_DEFAULT):
    """A noise-free three-pair problem -> (pixels (3, 2), points (3, 3), R_true, t_true)."""
    rng = np.random.default_rng(seed)
    R, t = make_pose(rng)
    pix, pts = make_pairs(rng, 3, R, t, K)
    return pix, pts, R, t
