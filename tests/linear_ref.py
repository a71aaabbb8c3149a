"""Exact linear systems for the reduced system's tiled Cholesky (dense_plan.h, dim_order.h, chol_chain.h, k_chol.hip) and the measure its
solutions are held to.  Plain NumPy; deliberately none of the library's code.

Families (all entries dyadic, so every system is exactly what its float64 arrays say):
    dominant(n, bw, seed)        band of half-width bw from integers(-8, 9) / 8, diagonal = row sum of |.| + 1: cond ~ 3
    laplacian(n, bw, seed, k)    band from -integers(0, 9) / 8, diagonal = row sum of |.| + 2^-k: cond ~ 8e4 / 8e7 / 8e10 at k = 10 / 20 / 30
    vec3_graph(N, band, k, ...)  a chain of three-vectors, one weak prior 2^-k I on the first, strong relative constraints: the gauge-weak
                                 window of a SLAM back end; damped_system() is the LM step's system on it
Measure: eta(M, rhs, x) = max|M x - rhs| / (|M|_inf |x|_inf + |rhs|_inf), the normwise backward error (Rigal-Gaches), residual in extended
precision.  A backward-stable solver keeps it at a small multiple of 2^-53 whatever the condition number; eta_ref() is what
numpy.linalg.cholesky plus two substitutions reach on seeds 0..4 of a family and shape, the spread a device result is compared with
(MARGIN times it), and higham_cap(n) the a-priori bound above which a Cholesky solve is wrong, not inaccurate."""
import functools

import numpy as np

from beam_slam_amd import capi
from beam_slam_amd.problem import Problem

LD = np.longdouble
MARGIN = 8.0          # over the reference's own spread: another summation order and blocking (as gicp_ref.check, icp_ref)
SEEDS = range(5)
U = 2.0 ** -53


def longdouble_ok():
    """eta's residual needs more than double: the 64-bit significand of x87 extended (eps 1.08e-19) or better"""
    return float(np.finfo(LD).eps) < 2e-19


def higham_cap(n):
    """n * gamma_{3n+1}, gamma_m = m u / (1 - m u): Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.4 with
    || |R^T| |R| || <= n ||A||"""
    m = 3 * n + 1
    return n * m * U / (1.0 - m * U)


def _finish(A, rng, far, far_value, mass):
    n = A.shape[0]
    A = A + A.T
    if far:     # one coupling of the first tile with the last one
        A[0, n - 1] = A[n - 1, 0] = far_value
    A[np.arange(n), np.arange(n)] = np.abs(A).sum(axis=1) + mass
    b = rng.integers(-64, 65, n) / 8.0
    return A, b


def dominant(n, bw, seed, far=False):
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for i in range(n):
        j0 = max(0, i - bw)
        A[i, j0:i] = rng.integers(-8, 9, i - j0) / 8.0
    return _finish(A, rng, far, 0.625, 1.0)


def laplacian(n, bw, seed, k, far=False):
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for i in range(n):
        j0 = max(0, i - bw)
        A[i, j0:i] = -(rng.integers(0, 9, i - j0) / 8.0)
    return _finish(A, rng, far, -0.625, 2.0 ** -k)


def tile_adjacency(A, tile=64):
    """the tile structure bsgpu_dense_solve plans on: tile (i, j) is there when A has a non-zero in it"""
    n = A.shape[0]
    T = (n + tile - 1) // tile
    P = np.zeros((T * tile, T * tile), bool)
    P[:n, :n] = A != 0.0
    return P.reshape(T, tile, T, tile).any(axis=(1, 3))


@functools.lru_cache(maxsize=None)     # (built once, shared by the tests and by eta_ref; nobody writes to what it returns)
def vec3_graph(N, band, k, seed, loop=False, hub=False):
    """N three-vector blocks at 0; F_ABS_VEC3 prior 2^-k I on block 0; F_REL_VEC3 (i, j) for 0 < j - i <= band, plus the loop closure
    (0, N - 1) and / or a hub (every third block with the last one).  Returns (Problem, J, r): the dense Jacobian and the residuals at
    the start, formed here from the factor constants as include/bsgpu.h pins them (r = A (x - b); r = A ((x2 - x1) - d); rows: the prior,
    then the relative factors in order; columns: the blocks in order)."""
    rng = np.random.default_rng(seed)
    pairs = [(i, j) for i in range(N) for j in range(i + 1, min(N, i + band + 1))]
    extra = ([(0, N - 1)] if loop else []) + ([(i, N - 1) for i in range(0, N - 1, 3)] if hub else [])
    for p in extra:
        if p not in pairs:
            pairs.append(p)
    pr = Problem()
    blocks = pr.add_blocks(np.zeros((N, 3)))
    b0 = rng.integers(-2, 3, 3).astype(float)           # whole numbers: 2^-2k b0 stays on the 2^-40 grid of the exactness argument
    A0 = 2.0 ** -k * np.eye(3)
    pr.add_factors(capi.F_ABS_VEC3, [[blocks[0]]], [np.concatenate([b0, A0.ravel()])])
    m = 3 + 3 * len(pairs)
    J, r = np.zeros((m, 3 * N)), np.zeros(m)
    J[0:3, 0:3] = A0
    r[0:3] = A0 @ (0.0 - b0)
    idx, consts = [], []
    for f, (i, j) in enumerate(pairs):
        A = np.triu(rng.integers(-8, 9, (3, 3)) / 8.0, 1) + np.diag(rng.integers(4, 9, 3) / 8.0)
        z = rng.integers(-16, 17, 3) / 8.0
        idx.append([blocks[i], blocks[j]])
        consts.append(np.concatenate([z, A.ravel()]))
        rows = slice(3 + 3 * f, 6 + 3 * f)
        J[rows, 3 * i:3 * i + 3] = -A
        J[rows, 3 * j:3 * j + 3] = A
        r[rows] = A @ (0.0 - z)
    pr.add_factors(capi.F_REL_VEC3, idx, consts)
    J.setflags(write=False)
    r.setflags(write=False)
    return pr, J, r


def normal_equations(J, r):
    """H = J^T J and g = J^T r, exact in double whatever the order of addition; asserts why.  Every entry of J and r is a whole multiple
    of 2^-20 (vec3_graph with k <= 20), so every product is one of 2^-40; the sums of the products' absolute values stay below 2^12, so
    every partial sum of every order is a whole multiple of 2^-40 below 2^12 — 52 bits, a double.  (That covers the sums formed here,
    those of the absolute values first: they only grow, each is exact while it is below 2^12, and the last one is.)"""
    for a in (J, r):
        scaled = a * 2.0 ** 20
        assert (scaled == np.rint(scaled)).all()
    assert max(np.abs(np.abs(J).T @ np.abs(J)).max(), np.abs(np.abs(J).T @ np.abs(r)).max()) < 2.0 ** 12
    H, g = J.T @ J, J.T @ r
    for a in (H, g):
        scaled = a * 2.0 ** 40
        assert (scaled == np.rint(scaled)).all() and np.abs(scaled).max() < 2.0 ** 52
    return H, g


def damped_system(J, r, radius, jacobi, lm_lo=1e-6, lm_hi=1e32):
    """(M, rhs) of the LM step from the start: (H + diag(d) / radius) delta = -g with d = clamp(sc^2 h, lo, hi) / sc^2, h = diag H and
    sc = 1 / (1 + sqrt(h)) under Jacobi scaling, else 1 (Ceres' LevenbergMarquardtStrategy on the scaled Jacobian, stated for the
    unscaled step).  Extended precision: the diagonal is not a double."""
    H, g = normal_equations(J, r)
    h = np.diag(H).astype(LD)
    sc = 1.0 / (1.0 + np.sqrt(h)) if jacobi else np.ones_like(h)
    d = np.clip(sc * sc * h, LD(lm_lo), LD(lm_hi)) / (sc * sc)
    M = H.astype(LD)
    M[np.arange(len(h)), np.arange(len(h))] += d / LD(radius)
    return M, -g.astype(LD)


def step_options(solver, log2_radius, jacobi):
    o = solver.options_default()
    o.max_num_iterations = 1
    o.initial_trust_region_radius = 2.0 ** log2_radius
    o.jacobi_scaling = int(jacobi)
    return o


def lm_step(solver, pr, log2_radius, jacobi):
    """one LM iteration of `solver` (a capi.Solver) on the graph -> (summary, the step: every value starts at 0, so the values after
    the solve are the step itself, with no rounding in x + delta)"""
    pr.load(solver)
    summary = solver.solve(step_options(solver, log2_radius, jacobi))
    return summary, solver.get_blocks()


def evaluate_at_start(solver, pr):
    """(residuals, dense Jacobian) of `solver` on the graph at its start"""
    pr.load(solver)
    _, r, _, J = solver.evaluate(residuals=True, gradient=False, jacobian=True)
    return r, J


def eta(M, rhs, x):
    """normwise backward error of x as a solution of M x = rhs, the residual formed in numpy.longdouble"""
    M, rhs, x = np.asarray(M, LD), np.asarray(rhs, LD), np.asarray(x, np.float64).astype(LD)
    res = np.abs(M @ x - rhs).max()
    return float(res / (np.abs(M).sum(axis=1).max() * np.abs(x).max() + np.abs(rhs).max()))


def eta_between(M, rhs, x, y):
    """the difference of two solutions on eta's scale: max|M (x - y)| / (|M|_inf |x|_inf + |rhs|_inf)"""
    M, rhs = np.asarray(M, LD), np.asarray(rhs, LD)
    x, y = np.asarray(x, np.float64).astype(LD), np.asarray(y, np.float64).astype(LD)
    return float(np.abs(M @ (x - y)).max() / (np.abs(M).sum(axis=1).max() * np.abs(x).max() + np.abs(rhs).max()))


def cholesky_solve(M, rhs):
    """the reference: numpy.linalg.cholesky and two substitutions, row by row, in double"""
    M, rhs = np.asarray(M, np.float64), np.asarray(rhs, np.float64)
    L = np.linalg.cholesky(M)
    n = len(rhs)
    y = np.zeros(n)
    for i in range(n):
        y[i] = (rhs[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def system(family, shape, seed):
    """(M, rhs) of one member.  shape: (n, bw, far) for "dominant", (n, bw, k, far) for "laplacian" and (N, band, k, loop, hub,
    log2 radius, jacobi) for "graph"."""
    if family == "dominant":
        n, bw, far = shape
        return dominant(n, bw, seed, far)
    if family == "laplacian":
        n, bw, k, far = shape
        return laplacian(n, bw, seed, k, far)
    N, band, k, loop, hub, log2_radius, jacobi = shape
    _, J, r = vec3_graph(N, band, k, seed, loop, hub)
    return damped_system(J, r, 2.0 ** log2_radius, jacobi)


@functools.lru_cache(maxsize=None)
def eta_ref(family, shape):
    """the largest eta of cholesky_solve over seeds 0..4 of the family and shape: the reference's own spread"""
    worst = 0.0
    for seed in SEEDS:
        M, rhs = system(family, shape, seed)
        worst = max(worst, eta(M, rhs, cholesky_solve(M, rhs)))
    return worst


# the shapes of the hook's test: (n, scalar half-width, max_chains, far) and what the planner must make of them (tests/test_linear_ref.py
# asserts it from dense_plan.h itself): n_chains, appendix-tile tasks (kFusedExt), K-chunk tasks (kFusedSplit), level-synchronised
# back-substitution.  None: not asserted.
HOOK_SHAPES = [
    # n, bw, max_chains, far   chains  ext    split  level-sync
    ((63, 62, 4, False),       (1,     False, False, False)),     # one partial tile
    ((64, 40, 4, False),       (1,     False, False, False)),     # one full tile
    ((65, 30, 4, False),       (1,     True,  False, False)),     # a full tile and an appendix tile of one column
    ((128, 40, 4, False),      (1,     None,  None,  False)),     # two full tiles, no padding
    ((200, 40, 4, False),      (2,     False, True,  True)),
    ((449, 60, 4, False),      (4,     False, True,  True)),      # last tile one column
    ((520, 60, 4, False),      (4,     False, True,  True)),
    ((450, 60, 4, True),       (1,     True,  True,  False)),     # the far coupling keeps it one chain, with its fill
    ((450, 60, 1, False),      (1,     True,  True,  False)),     # natural order forced
    ((900, 100, 4, False),     (4,     False, True,  True)),      # tile half-width 2
]
LAPLACIAN_K = (10, 20, 30)

# the graphs of the production path's test, by tangent dimension: (N, band, loop, hub)
GRAPHS = {
    "63": (21, 4, False, False),        # one tile
    "66": (22, 4, False, False),        # one tile plus 2 columns
    "192": (64, 4, False, False),       # three full tiles
    "450": (150, 4, False, False),
    "450-loop": (150, 4, True, False),
    "450-hub": (150, 4, False, True),
    "522-loop": (174, 4, True, False),
    "522": (174, 4, False, False),      # (plain, for the n_chains assertion)
}
GRAPH_K = (10, 20)
GRAPH_LOG2_RADIUS = (20, 40)


def graph_shape(name, k, log2_radius, jacobi):
    N, band, loop, hub = GRAPHS[name]
    return (N, band, k, loop, hub, log2_radius, jacobi)
