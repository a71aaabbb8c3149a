"""Independent NumPy restatement of bsgpu_essential_ransac (include/bsgpu.h) and of beam_slam_amd/csrc/five_point.h, in the manner
of dogleg_ref.py: nothing here is transcribed from the header.

* five_point(): the null space from numpy.linalg.svd, the ten cubic constraints (det E = 0, 2 E E^T E - tr(E E^T) E = 0) from
  generic polynomial arithmetic on {exponent triple: coefficient} dictionaries, the solutions from numpy.linalg.eig of the 10 x 10
  action matrix of multiplication by x on the quotient-ring basis (x^2, xy, xz, y^2, yz, z^2, x, y, z, 1).  An eigenvalue is real
  when LAPACK returns it with a zero imaginary part.  Solutions are returned with |E|_F = 1, the largest-magnitude entry positive,
  in ascending order of E[0, 0] (the contract's order inside a sample).
* sampson_sq(), sample_indices() (splitmix64 in Python integers masked to 64 bits), update_niters() and ransac_serial(): the
  contract's serial loop.
* the seeded case generator shared by tests/test_five_point.py, tests/test_gpu_essential_ransac.py and
  scripts/time_essential_ransac.py."""
import math

import numpy as np

K_DEFAULT = (400.0, 400.0, 320.0, 240.0)
WIDTH, HEIGHT = 640, 480
M64 = (1 << 64) - 1
STATUS_OK, STATUS_TOO_FEW, STATUS_NO_MODEL = 0, 1, 2


# ---- polynomials in (x, y, z) as dictionaries ----------------------------------------------------------------------------------
def p_add(a, b, s=1.0):
    out = dict(a)
    for m, c in b.items():
        out[m] = out.get(m, 0.0) + s * c
    return out


def p_mul(a, b):
    out = {}
    for ma, ca in a.items():
        for mb, cb in b.items():
            m = (ma[0] + mb[0], ma[1] + mb[1], ma[2] + mb[2])
            out[m] = out.get(m, 0.0) + ca * cb
    return out


CUBICS = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def normalize_E(E):
    E = np.asarray(E, float).reshape(3, 3)
    E = E / np.linalg.norm(E)
    k = np.argmax(np.abs(E))
    return E if E.flat[k] > 0 else -E


def epipolar_matrix(x1, x2):
    """Rows of x2^T E x1 = 0 in the row-major entries of E; x1, x2: (n, 2) normalised coordinates."""
    h1 = np.column_stack([x1, np.ones(len(x1))])
    h2 = np.column_stack([x2, np.ones(len(x2))])
    return np.einsum("ni,nj->nij", h2, h1).reshape(len(x1), 9)


def five_point(x1, x2):
    """All real essential matrices of five normalised matches -> list of 3x3 arrays (possibly empty)."""
    A = epipolar_matrix(np.asarray(x1, float), np.asarray(x2, float))
    _, _, vt = np.linalg.svd(A)
    Eb = vt[5:9].reshape(4, 3, 3)
    lin = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
    E = [[{lin[b]: Eb[b, i, j] for b in range(4)} for j in range(3)] for i in range(3)]
    det = {}
    for (a, b, c), s in (((0, 1, 2), 1), ((1, 2, 0), 1), ((2, 0, 1), 1), ((0, 2, 1), -1), ((1, 0, 2), -1), ((2, 1, 0), -1)):
        det = p_add(det, p_mul(p_mul(E[0][a], E[1][b]), E[2][c]), s)
    EEt = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for k in range(3):
            q = {}
            for l in range(3):
                q = p_add(q, p_mul(E[i][l], E[k][l]))
            EEt[i][k] = q
    tr = p_add(p_add(EEt[0][0], EEt[1][1]), EEt[2][2])
    cons = [det]
    for i in range(3):
        for j in range(3):
            c = {}
            for k in range(3):
                c = p_add(c, p_mul(EEt[i][k], E[k][j]), 2.0)
            cons.append(p_add(c, p_mul(tr, E[i][j]), -1.0))
    C = np.array([[c.get(m, 0.0) for m in CUBICS + BASIS] for c in cons])
    try:
        M = np.linalg.solve(C[:, :10], C[:, 10:])     # cubic_i = -M[i] . basis
    except np.linalg.LinAlgError:
        return []
    if not np.all(np.isfinite(M)):
        return []
    act = np.zeros((10, 10))                          # act v = x v for v = basis monomials at a solution
    for r, m in enumerate(BASIS):
        xm = (m[0] + 1, m[1], m[2])
        if xm in BASIS:
            act[r, BASIS.index(xm)] = 1.0
        else:
            act[r] = -M[CUBICS.index(xm)]
    w, v = np.linalg.eig(act)
    sols = []
    for k in range(10):
        if w[k].imag != 0.0:
            continue
        vec = v[:, k].real
        if vec[9] == 0.0:
            continue
        x, y, z = vec[6] / vec[9], vec[7] / vec[9], vec[8] / vec[9]
        Ek = x * Eb[0] + y * Eb[1] + z * Eb[2] + Eb[3]
        if np.all(np.isfinite(Ek)) and np.linalg.norm(Ek) > 0:
            sols.append(normalize_E(Ek))
    sols.sort(key=lambda e: e[0, 0])
    return sols


# ---- error, sampler, loop -----------------------------------------------------------------------------------------------------
def normalize_pixels(px, K):
    fx, fy, cx, cy = K
    px = np.asarray(px, float).reshape(-1, 2)
    return np.column_stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy])


def sampson_sq(E, x1, x2):
    """(x2^T E x1)^2 / ((E x1)_0^2 + (E x1)_1^2 + (E^T x2)_0^2 + (E^T x2)_1^2), x1 previous, x2 current, per match."""
    h1 = np.column_stack([x1, np.ones(len(x1))])
    h2 = np.column_stack([x2, np.ones(len(x2))])
    Ex1 = h1 @ E.T
    Etx2 = h2 @ E
    num = np.sum(h2 * Ex1, axis=1) ** 2
    return num / (Ex1[:, 0] ** 2 + Ex1[:, 1] ** 2 + Etx2[:, 0] ** 2 + Etx2[:, 1] ** 2)


def sample_indices(seed, set_index, sample_index, n):
    state = (seed ^ ((set_index * 0x9E3779B97F4A7C15) & M64) ^ ((sample_index * 0xBF58476D1CE4E5B9) & M64)) & M64
    out = []
    while len(out) < 5:
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
    t = 1.0 - (1.0 - ep) ** 5
    den = math.log(t) if t > 0.0 else -math.inf
    if den >= 0.0 or -num >= niters * (-den):
        return niters
    return int(round(num / den))


def ransac_serial(px_prev, px_cur, K, prob=0.99, threshold_px=1.0, max_iters=1000, seed=0, set_index=0):
    """The contract's serial loop for one set -> dict(mask uint8 (n), E (3x3), n_inliers, n_iters, best_sample (5), status, err)."""
    px_prev = np.asarray(px_prev, float).reshape(-1, 2)
    px_cur = np.asarray(px_cur, float).reshape(-1, 2)
    n = len(px_prev)
    out = dict(mask=np.ones(n, np.uint8), E=np.zeros((3, 3)), n_inliers=0, n_iters=0, best_sample=-np.ones(5, np.int32),
               status=STATUS_TOO_FEW, err=None)
    if n < 5:
        return out
    x1, x2 = normalize_pixels(px_prev, K), normalize_pixels(px_cur, K)
    thr = threshold_px / (0.5 * (K[0] + K[1]))
    thr2 = thr * thr
    niters, best, s = max_iters, 0, 0
    out["status"] = STATUS_NO_MODEL
    while s < niters:
        idx = sample_indices(seed, set_index, s, n)
        for E in five_point(x1[idx], x2[idx]):
            err = sampson_sq(E, x1, x2)
            inl = err <= thr2
            good = int(inl.sum())
            if good > max(best, 4):
                best = good
                out.update(mask=inl.astype(np.uint8), E=E, n_inliers=good, best_sample=np.array(idx, np.int32), status=STATUS_OK,
                           err=err)
                niters = update_niters(prob, (n - good) / n, niters)
        s += 1
    out["n_iters"] = s
    out["thr2"] = thr2
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def make_motion(rng):
    """(R, t) of X_cur = R X_prev + t: a few degrees, baseline 0.1-0.5 m."""
    w = rng.normal(size=3)
    w *= np.deg2rad(rng.uniform(1.0, 5.0)) / np.linalg.norm(w)
    t = rng.normal(size=3)
    t *= rng.uniform(0.1, 0.5) / np.linalg.norm(t)
    return rodrigues(w), t


def make_matches(rng, n, R, t, K=K_DEFAULT):
    """n noise-free matches (pixels) with both projections inside the image, depth 2-10 m in the previous frame."""
    fx, fy, cx, cy = K
    prev, cur = [], []
    while len(prev) < n:
        u, v, d = rng.uniform(0, WIDTH), rng.uniform(0, HEIGHT), rng.uniform(2.0, 10.0)
        X = np.array([(u - cx) / fx * d, (v - cy) / fy * d, d])
        Y = R @ X + t
        if Y[2] <= 0.5:
            continue
        u2, v2 = fx * Y[0] / Y[2] + cx, fy * Y[1] / Y[2] + cy
        if 0 <= u2 < WIDTH and 0 <= v2 < HEIGHT:
            prev.append((u, v))
            cur.append((u2, v2))
    return np.array(prev, float).reshape(-1, 2), np.array(cur, float).reshape(-1, 2)


def sampson_px(E, px_prev, px_cur, K):
    """Sampson distance in pixels under E (a matrix on normalised coordinates)."""
    return np.sqrt(sampson_sq(E, normalize_pixels(px_prev, K), normalize_pixels(px_cur, K))) * 0.5 * (K[0] + K[1])


def make_set(seed, n, outlier_frac, K=K_DEFAULT, truncate=False):
    """A seeded match set -> dict(px_prev, px_cur, labels (1 inlier), E_true (normalised), K).  An outlier's current pixel is
    redrawn uniformly until its Sampson distance under the true E is at least 10 px."""
    rng = np.random.default_rng(seed)
    R, t = make_motion(rng)
    E_true = normalize_E(skew(t) @ R)
    prev, cur = make_matches(rng, n, R, t, K)
    labels = np.ones(n, np.uint8)
    n_out = int(round(outlier_frac * n))
    for i in rng.permutation(n):
        if n_out == 0:
            break
        for _ in range(100):   # (a match next to the epipole is within 10 px of its line wherever its partner lies: it stays an inlier)
            c = np.array([rng.uniform(0, WIDTH), rng.uniform(0, HEIGHT)])
            if sampson_px(E_true, prev[i:i + 1], c[None], K)[0] >= 10.0:
                cur[i] = c
                labels[i] = 0
                n_out -= 1
                break
    if truncate:
        prev, cur = np.trunc(prev), np.trunc(cur)
    return dict(px_prev=prev, px_cur=cur, labels=labels, E_true=E_true, K=K, R=R, t=t)


def make_random_set(seed, n):
    rng = np.random.default_rng(seed)
    return dict(px_prev=rng.uniform(0, [WIDTH, HEIGHT], size=(n, 2)), px_cur=rng.uniform(0, [WIDTH, HEIGHT], size=(n, 2)), K=K_DEFAULT)


def minimal_case(seed, K=K_DEFAULT):
    """A noise-free five-match problem in normalised coordinates -> (x1, x2, E_true, condition of the 5x5 Jacobian of the
    epipolar residuals at the truth over three rotation and two translation-direction parameters)."""
    rng = np.random.default_rng(seed)
    R, t = make_motion(rng)
    prev, cur = make_matches(rng, 5, R, t, K)
    x1, x2 = normalize_pixels(prev, K), normalize_pixels(cur, K)
    h1 = np.column_stack([x1, np.ones(5)])
    h2 = np.column_stack([x2, np.ones(5)])
    tn = t / np.linalg.norm(t)
    b1 = np.cross(tn, [1.0, 0, 0] if abs(tn[0]) < 0.9 else [0, 1.0, 0])
    b1 /= np.linalg.norm(b1)
    b2 = np.cross(tn, b1)
    J = np.zeros((5, 5))
    for k in range(3):      # R <- exp(w) R
        G = np.zeros(3)
        G[k] = 1.0
        J[:, k] = np.einsum("ni,ij,nj->n", h2, skew(tn) @ skew(G) @ R, h1)
    for k, b in enumerate((b1, b2)):
        J[:, 3 + k] = np.einsum("ni,ij,nj->n", h2, skew(b) @ R, h1)
    return x1, x2, normalize_E(skew(t) @ R), np.linalg.cond(J)


def dist_E(a, b):
    a, b = np.asarray(a).reshape(3, 3), np.asarray(b).reshape(3, 3)
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b))
