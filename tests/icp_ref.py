"""NumPy restatement of the ICP that include/bsgpu.h pins for bsgpu_register_scans: brute-force nearest neighbour over all targets (no
grid), numpy.linalg.svd, plain sums.  Deliberately not the code of beam_slam_amd/csrc/icp.h.  Also the scenes of the tests and the
margins of their decisions (the gap between the best and the second-best squared distance; the distance of any squared distance from
the threshold), which must be far above rounding for two implementations to be comparable at all.
"""
import functools

import numpy as np

MAX_ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, TOO_FEW = 1, 2, 3, 4, 5
DEFAULTS = dict(max_corr=1.0, max_iter=50, t_eps=1e-8, fit_eps=1e-2, rotation_threshold=0.99999, rel_mse_eps=1e-5)   # config/matchers/icp.json
EYE = np.hstack([np.eye(3), np.zeros((3, 1))])


def rotvec(r):
    r = np.asarray(r, float)
    th = np.linalg.norm(r)
    if th == 0.0:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def transform(T, P):
    T = np.asarray(T, float).reshape(3, 4)
    return np.asarray(P, float).reshape(-1, 3) @ T[:, :3].T + T[:, 3]


def nearest(s, Q, block=256):
    """Per row of s: (index of the nearest row of Q — the lowest among equals —, its squared distance, the second-smallest squared
    distance); (-1, inf, inf) without targets."""
    n = len(s)
    idx, d2, second = np.full(n, -1), np.full(n, np.inf), np.full(n, np.inf)
    if len(Q) == 0:
        return idx, d2, second
    for a in range(0, n, block):
        D = ((s[a:a + block, None, :] - Q[None, :, :]) ** 2).sum(axis=2)
        j = D.argmin(axis=1)                      # the first of equal minima
        idx[a:a + block], d2[a:a + block] = j, D[np.arange(len(j)), j]
        if Q.shape[0] > 1:
            D[np.arange(len(j)), j] = np.inf
            second[a:a + block] = D.min(axis=1)
    return idx, d2, second


def run(S, Q, T_init=None, max_corr=1.0, max_iter=50, t_eps=1e-8, fit_eps=1e-2, rotation_threshold=0.99999, rel_mse_eps=1e-5):
    """One pair.  Returns dict(T (3x4), T_ref_tgt, mse, n_corr, n_iters, status, gap, margin): gap = the smallest difference between a
    source point's best and second-best squared distance, margin = the smallest |d^2 - max_corr^2|, over all iterations."""
    S, Q = np.asarray(S, float).reshape(-1, 3), np.asarray(Q, float).reshape(-1, 3)
    Ti = EYE if T_init is None else np.asarray(T_init, float).reshape(3, 4)
    Q = transform(Ti, Q)
    R, t = np.eye(3), np.zeros(3)
    mse_prev, mse, n_corr, status, n_iters = np.inf, 0.0, 0, 0, 0
    gap = margin = np.inf
    h2 = max_corr * max_corr
    k = 0
    while status == 0:
        k += 1
        s = S @ R.T + t
        j, d2, second = nearest(s, Q)
        if len(d2) and len(Q) > 1:
            gap, margin = min(gap, float((second - d2).min())), min(margin, float(np.abs(d2 - h2).min()))
        keep = d2 <= h2
        n_corr = int(keep.sum())
        mse = float(d2[keep].sum() / n_corr) if n_corr else 0.0
        if n_corr < 3:
            status, n_iters = TOO_FEW, k - 1
            break
        a, b = s[keep], Q[j[keep]]
        ca, cb = a.sum(axis=0) / n_corr, b.sum(axis=0) / n_corr
        H = (a - ca).T @ (b - cb)
        U, _, Vt = np.linalg.svd(H)
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
        dR = Vt.T @ D @ U.T
        dt = cb - dR @ ca
        R, t = dR @ R, dR @ t + dt
        n_iters = k
        with np.errstate(invalid="ignore"):
            if k >= max_iter:
                status = MAX_ITERATIONS
            elif 0.5 * (np.trace(dR) - 1.0) >= rotation_threshold and dt @ dt <= t_eps:
                status = TRANSFORM
            elif abs(mse - mse_prev) < fit_eps:
                status = ABS_MSE
            elif abs(mse - mse_prev) / mse_prev < rel_mse_eps:
                status = REL_MSE
        mse_prev = mse
    T = np.hstack([R, t[:, None]])
    T_ref_tgt = np.hstack([R.T @ Ti[:, :3], (R.T @ (Ti[:, 3] - t))[:, None]])
    return dict(T=T, T_ref_tgt=T_ref_tgt, mse=mse, n_corr=n_corr, n_iters=n_iters, status=status, gap=gap, margin=margin)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
BOX = np.array([20.0, 14.0, 5.0])
MOTION_R, MOTION_T = rotvec([0.01, -0.02, 0.04]), np.array([0.25, -0.15, 0.05])


def box_points(n, rng):
    """n points on the faces of the 20 x 14 x 5 m box (centred at the origin, seen from inside), uniform by area."""
    areas = np.array([BOX[1] * BOX[2], BOX[1] * BOX[2], BOX[0] * BOX[2], BOX[0] * BOX[2], BOX[0] * BOX[1], BOX[0] * BOX[1]])
    face = rng.choice(6, size=n, p=areas / areas.sum())
    P = (rng.random((n, 3)) - 0.5) * BOX
    axis, side = face // 2, np.where(face % 2 == 0, -0.5, 0.5)
    P[np.arange(n), axis] = side * BOX[axis]
    return P


@functools.lru_cache(maxsize=None)
def scene(n, seed=7):
    """(reference cloud S, target cloud Q), n points each: two independent 80 % subsamples of one set of points on the box, the target
    moved by rotation vector (0.01, -0.02, 0.04) and translation (0.25, -0.15, 0.05), both with 1 cm noise."""
    rng = np.random.default_rng(seed + n)
    full = box_points(int(round(n / 0.8)), rng)
    S = full[np.sort(rng.choice(len(full), n, replace=False))] + 0.01 * rng.standard_normal((n, 3))
    Q = full[np.sort(rng.choice(len(full), n, replace=False))] @ MOTION_R.T + MOTION_T + 0.01 * rng.standard_normal((n, 3))
    S.setflags(write=False); Q.setflags(write=False)
    return S, Q


CASES = {"n600_fit": (600, dict(fit_eps=1e-2)), "n600_nofit": (600, dict(fit_eps=0.0)), "n4000_fit": (4000, dict(fit_eps=1e-2)),
         "n4000_nofit": (4000, dict(fit_eps=0.0))}


@functools.lru_cache(maxsize=None)
def case(name):
    """(S, Q, keyword arguments, the restatement's result, its result with the source points in reversed order) — computed once per
    process and shared by every test that needs it."""
    n, kw = CASES[name]
    S, Q = scene(n)
    kw = dict(DEFAULTS, **kw)
    return S, Q, kw, run(S, Q, **kw), run(S[::-1], Q, **kw)


def bounds(res, rev):
    """The allowed differences from `res`: 8 x the restatement's own difference under another summation order (the source points
    reversed), per quantity — rotation block, translation, mse —, and not below one unit of FP64 precision of the quantity's largest
    magnitude."""
    out = {}
    for name, a, b in (("R", res["T"][:, :3], rev["T"][:, :3]), ("t", res["T"][:, 3], rev["T"][:, 3]), ("mse", res["mse"], rev["mse"])):
        a, b = np.asarray(a, float), np.asarray(b, float)
        out[name] = (max(8.0 * np.abs(a - b).max(), 2.0 ** -52 * np.abs(a).max()), float(np.abs(a - b).max()))
    return out


def check(got_T, got_mse, res, rev, who):
    """Asserts the bounds; returns {quantity: difference / bound} (printed by the callers, recorded in their docstrings)."""
    bd = bounds(res, rev)
    got_T = np.asarray(got_T, float).reshape(3, 4)
    diff = {"R": np.abs(got_T[:, :3] - res["T"][:, :3]).max(), "t": np.abs(got_T[:, 3] - res["T"][:, 3]).max(), "mse": abs(got_mse - res["mse"])}
    ratio = {k: float(diff[k] / bd[k][0]) for k in diff}
    print(f"{who}: difference / bound {ratio}; the restatement's own difference {({k: v[1] for k, v in bd.items()})}")
    for k in diff:
        assert diff[k] <= bd[k][0], (who, k, diff[k], bd[k])
    return ratio
