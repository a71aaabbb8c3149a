"""bsgpu_register_scans_gicp on the CPU: beam_slam_amd/csrc/gicp.h (through tests/plan/test_gicp.cpp, the kernels' arithmetic and order
of addition on one core) against the NumPy restatement of the contract (tests/gicp_ref.py: brute-force neighbours, numpy.linalg.eigh
and inv, plain sums).

Scenes (icp_ref.scene): the 600- and 4 000-point box scenes at k 10 / max_corr 5, k 10 / max_corr 1 (589 of 600 kept: the threshold is
exercised) and k 20.  Before anything is compared every case asserts that its input can be compared: the three distance margins of
gicp_ref exceed 1e-9 m^2 and the eigenvalue gap 1e-6, and the restatement's three variants agree on status and counts.

Accuracy criterion (test_icp.py's): status, n_iters, n_inner and n_corr equal; rotation block, translation, cost and every C' within
8 x the restatement's own spread (the largest difference among its variants: plain, reversed sums, SVD for eigh), and not below 2^-52 of
the quantity's largest magnitude.
"""
import os
import subprocess

import numpy as np
import pytest

import gicp_ref as ref
import icp_ref
from test_icp import grid_clouds, run_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plan", "test_gicp.cpp")
INC = os.path.join(ROOT, "beam_slam_amd", "csrc")
MAX_CELLS = float(1 << 22)
GRID_CELL = 0.5


def reg_command(S, Q, T_init=None, max_cells=MAX_CELLS, grid_cell=GRID_CELL, want_cov=False, **kw):
    d = dict(ref.DEFAULTS, **kw)
    S, Q = np.asarray(S, float).reshape(-1, 3), np.asarray(Q, float).reshape(-1, 3)
    head = [1, len(S), len(Q), 0 if T_init is None else 1, d["k_neighbors"], d["gicp_epsilon"], d["max_corr"], d["max_iter"], d["r_eps"], d["t_eps"],
            d["max_inner"], d["inner_eps"], grid_cell, max_cells, 1 if want_cov else 0]
    return np.concatenate([np.array(head, float), S.ravel(), Q.ravel(), np.zeros(0) if T_init is None else np.asarray(T_init, float).ravel()])


def knn_command(P, k, h):
    return np.concatenate([np.array([2, len(P), k, h], float), np.asarray(P, float).ravel()])


def nn_command(S, Q, h, max_corr):
    return np.concatenate([np.array([3, len(S), len(Q), h, max_corr], float), np.asarray(S, float).ravel(), np.asarray(Q, float).ravel()])


def parse_reg(tok, n_src=0, n_tgt=0):
    """A REG line -> dict; the covariances too when the command asked for them (n_src, n_tgt: the clouds' sizes)."""
    v = [float(x) for x in tok[8:]]
    out = dict(ok=int(tok[2]), status=int(tok[3]), n_iters=int(tok[4]), n_inner=int(tok[5]), n_corr=int(tok[6]), cost=float(tok[7]),
               T=np.array(v[0:12]).reshape(3, 4), T_ref_tgt=np.array(v[12:24]).reshape(3, 4))
    if len(v) > 24:
        out["ref_cov"] = np.array(v[24:24 + 6 * n_src]).reshape(-1, 6)
        out["tgt_cov"] = np.array(v[24 + 6 * n_src:]).reshape(-1, 6)
        assert len(out["tgt_cov"]) == n_tgt
    return out


def _compile(tmp_path_factory, flags, name):
    exe = str(tmp_path_factory.mktemp("gicp") / name)
    # -ffp-contract=off: the header's pragma is clang's; GCC gets the same rule from the command line (icp.h, "Bits")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", INC, SRC, "-o", exe] + flags, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"], "test_gicp")


def comparable(name):
    """The condition on the input: every neighbour, correspondence and threshold decision of the case is far above rounding, the
    covariances' smallest direction is well separated, and the restatement's variants made the same decisions."""
    S, Q, kw, results = ref.case(name)
    for v, r in results.items():
        assert r["knn_gap"] > 1e-9 and r["gap"] > 1e-9 and r["margin"] > 1e-9 and r["eig_gap"] > 1e-6, (name, v, r["knn_gap"], r["gap"], r["margin"], r["eig_gap"])
    keys = ("status", "n_iters", "n_inner", "n_corr")
    assert len({tuple(r[k] for k in keys) for r in results.values()}) == 1, name
    return S, Q, kw, results


def search_fixtures():
    """(knn fixtures [(P, k)], nn fixtures [(S, Q, max_corr)]): the grid_clouds() of test_icp — integer coordinates, so that there are
    ties at the k-th place, targets on cell faces and squared distances of exactly max_corr^2 (which the strict < drops); a cloud one
    cell thick; queries far outside the box; real-valued clouds — and k = |P|."""
    clouds = grid_clouds()
    rng = np.random.default_rng(5)
    knn = []
    for S, Q, h in clouds:
        if len(Q) >= 10:
            knn.append((Q, 10))
            knn.append((Q, 1))
    flat = clouds[12][1]
    knn += [(flat, 32), (flat, len(flat)), (rng.uniform(-2, 2, size=(33, 3)), 33), (rng.integers(0, 3, size=(50, 3)).astype(float), 7)]
    nn = [(S, Q, h) for S, Q, h in clouds]
    nn.append((rng.uniform(-9, 9, size=(200, 3)), clouds[15][1], 5.0))
    nn.append((rng.integers(-6, 7, size=(200, 3)).astype(float), clouds[0][1], 3.0))
    return knn, nn


CELLS = (1.0, 0.37, 2.5, 1000.0)


# ---- the header against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.CASES))
def test_header_against_restatement(name, core, tmp_path):
    """Measured (CPU build, g++ -O2), per case: outer / inner iterations, kept, the margins (knn gap, correspondence gap, threshold
    margin, eigenvalue gap) and the largest difference / bound:
        n600_k10_c5    5 / 15  600   1.4e-4  5.3e-5  2.3e+1  0.011    R 0.80  t 0.03  cost 0.10  ref_cov 0.04  tgt_cov 0.11
        n600_k10_c1    5 / 15  589   1.4e-4  4.8e-5  2.8e-3  0.011    R 0.13  t 0.04  cost 0.28  ref_cov 0.04  tgt_cov 0.11
        n4000_k10_c5   6 / 18  4000  1.4e-5  2.0e-6  2.4e+1  0.023    R 0.50  t 0.09  cost 0.00  ref_cov 0.02  tgt_cov 0.03
        n4000_k20_c5   5 / 14  4000  3.2e-6  3.0e-6  2.4e+1  0.081    R 0.25  t 0.13  cost 0.22  ref_cov 0.03  tgt_cov 0.03
    all TRANSFORM.  The restatement's own spread is 1e-17 .. 2.2e-16 in R (the bound is then its floor, 2^-52), 4e-16 .. 1.3e-15 in t,
    3e-17 .. 5e-16 in cost and 3e-15 .. 1.1e-14 in C' (the eigenvectors of a covariance whose two smallest eigenvalues lie 1 % of the
    largest apart).
    """
    S, Q, kw, results = comparable(name)
    res = results["plain"]
    got = parse_reg(run_program(core, [reg_command(S, Q, want_cov=True, **kw)], tmp_path)[0], len(S), len(Q))
    print(f"{name}: {res['n_iters']} / {res['n_inner']} iterations, status {res['status']}, n_corr {res['n_corr']}, knn gap {res['knn_gap']:.3e}, "
          f"gap {res['gap']:.3e}, margin {res['margin']:.3e}, eigenvalue gap {res['eig_gap']:.3e}")
    assert got["ok"] == 1
    assert (got["status"], got["n_iters"], got["n_inner"], got["n_corr"]) == (res["status"], res["n_iters"], res["n_inner"], res["n_corr"])
    assert res["status"] == ref.TRANSFORM
    ref.check(got, results, "header " + name, quantities=("R", "t", "cost", "ref_cov", "tgt_cov"))
    assert np.abs(got["T_ref_tgt"] - res["T_ref_tgt"]).max() < 1e-12


def test_search_is_exact(core, tmp_path):
    """The header's k nearest and its nearest below max_corr, through the grid at four cell edges, are brute force's by (d^2, index)."""
    knn, nn = search_fixtures()
    cmds = [knn_command(P, k, h) for P, k in knn for h in CELLS] + [nn_command(S, Q, h, mc) for S, Q, mc in nn for h in CELLS]
    rows = iter(run_program(core, cmds, tmp_path))
    ties = on_threshold = 0
    for P, k in knn:
        idx, kth, nxt = ref.knn(np.asarray(P, float), k)
        ties += int((kth == nxt).sum())
        for h in CELLS:
            assert [int(t) for t in next(rows)[2:]] == list(idx.ravel()), (len(P), k, h)
    for S, Q, mc in nn:
        j, d2, _ = icp_ref.nearest(np.asarray(S, float), np.asarray(Q, float))
        want = np.where(d2 < mc * mc, j, -1)
        on_threshold += int((d2 == mc * mc).sum())
        for h in CELLS:
            assert [int(t) for t in next(rows)[2:]] == list(want), (len(S), len(Q), mc, h)
    assert ties > 50 and on_threshold > 50      # the fixtures do exercise the tie rule and the strict threshold


def test_grid_cell_is_a_performance_knob_only(core, tmp_path):
    """The n600 case at cell edges 0.25, 0.5, 3 and 1000 (one cell): every output, covariances included, has the same bytes."""
    S, Q, kw, _ = ref.case("n600_k10_c5")
    rows = run_program(core, [reg_command(S, Q, grid_cell=h, want_cov=True, **kw) for h in (0.25, 0.5, 3.0, 1000.0)], tmp_path)
    assert rows[0][2] == "1" and len(rows[0]) == 8 + 24 + 12 * 600
    for tok in rows[1:]:
        assert tok[2:] == rows[0][2:]


def status_runs():
    """(name, S, Q, keyword arguments, the status it must end with)"""
    S, Q = ref.scene(600)
    small = np.asarray(Q)[:40] * 0.2                                   # a 4 x 3 x 1 m cloud
    far = np.asarray(S)[:9] * 0.2 + [100.0, 0.0, 0.0]
    three = np.concatenate([small[:3] + [0.01, -0.02, 0.015], far])   # twelve points (>= k), nine of them 100 m from the target
    same = np.tile([[1.0, 2.0, 3.0]], (12, 1))
    return [("max_iter", S, Q, dict(max_iter=2), ref.MAX_ITERATIONS), ("one iteration", S, Q, dict(max_iter=1), ref.MAX_ITERATIONS),
            ("transform", S, Q, {}, ref.TRANSFORM), ("three kept", three, small, {}, ref.TOO_FEW), ("k - 1 sources", S[:9], Q, {}, ref.TOO_FEW),
            ("k - 1 targets", S, Q[:9], {}, ref.TOO_FEW), ("no source", S[:0], Q, {}, ref.TOO_FEW), ("no target", S, Q[:0], {}, ref.TOO_FEW),
            ("degenerate", same, same + [0.1, 0.0, 0.0], {}, ref.DEGENERATE)]


def test_every_status(core, tmp_path):
    runs = status_runs()
    rows = run_program(core, [reg_command(s, q, **kw) for _, s, q, kw, _ in runs], tmp_path)
    for (name, s, q, kw, want), tok in zip(runs, rows):
        got, res = parse_reg(tok), ref.run(s, q, **dict(ref.DEFAULTS, **kw))
        assert got["ok"] == 1 and got["status"] == res["status"] == want, (name, got["status"], res["status"])
        assert (got["n_iters"], got["n_inner"], got["n_corr"]) == (res["n_iters"], res["n_inner"], res["n_corr"]), name
        if want in (ref.TOO_FEW, ref.DEGENERATE):
            assert got["n_iters"] == 0 and (got["T"] == ref.EYE).all(), name          # T stays as it was
        else:
            assert np.abs(got["T"] - res["T"]).max() < 1e-12, name
        if name == "three kept":
            assert got["n_corr"] == 3
        if want == ref.DEGENERATE:
            assert res["pivot"] < 1e-14 and got["n_corr"] == 12, res["pivot"]        # the decision is far from the 1e-12 threshold


def test_truth_recovery(core, tmp_path):
    """target = T reference exactly, every point, no noise: the result is T to 1e-10."""
    S = ref.box_points(500, np.random.default_rng(3))
    T = np.hstack([icp_ref.MOTION_R, icp_ref.MOTION_T[:, None]])
    got = parse_reg(run_program(core, [reg_command(S, ref.transform(T, S))], tmp_path)[0])
    print(f"truth: {got['n_iters']} / {got['n_inner']} iterations, status {got['status']}, |T - truth| {np.abs(got['T'] - T).max():.3e}, cost {got['cost']:.3e}")
    assert got["status"] == ref.TRANSFORM and got["n_corr"] == 500 and np.abs(got["T"] - T).max() < 1e-10


def test_initial_transform_and_composition(core, tmp_path):
    """T_init is applied to the target first (its covariances are those of the moved cloud); T_ref_tgt = inv(T_refest_ref) T_init."""
    S, Q = ref.scene(600)
    Ti = np.hstack([ref.rotvec([0.0, 0.0, 0.02]), np.array([[0.1], [-0.05], [0.0]])])
    got = parse_reg(run_program(core, [reg_command(S, Q, T_init=Ti, want_cov=True)], tmp_path)[0], 600, 600)
    res = ref.run(S, Q, T_init=Ti, **ref.DEFAULTS)
    assert (got["status"], got["n_iters"], got["n_inner"], got["n_corr"]) == (res["status"], res["n_iters"], res["n_inner"], res["n_corr"])
    assert res["gap"] > 1e-9 and res["knn_gap"] > 1e-9
    assert np.abs(got["T"] - res["T"]).max() < 1e-12 and np.abs(got["T_ref_tgt"] - res["T_ref_tgt"]).max() < 1e-12
    assert np.abs(got["tgt_cov"] - res["tgt_cov"]).max() < 1e-11
    T4, Ti4 = np.vstack([got["T"], [0, 0, 0, 1]]), np.vstack([Ti, [0, 0, 0, 1]])
    assert np.abs(np.linalg.inv(T4) @ Ti4 - np.vstack([got["T_ref_tgt"], [0, 0, 0, 1]])).max() < 1e-13


def test_cell_cap(core, tmp_path):
    """A grid of more cells than the cap is refused, not built."""
    S, Q = ref.scene(600)
    tok = run_program(core, [reg_command(S, Q, max_cells=100.0), reg_command(S, Q, max_cells=42 * 30 * 12)], tmp_path)
    assert parse_reg(tok[0])["ok"] == 0 and parse_reg(tok[1])["ok"] == 1


def test_header_under_sanitizers(tmp_path_factory, tmp_path):
    """The header as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, arrays of exact size: the
    600-point cases, every status, the empty clouds, the cell edges and the search fixtures run clean."""
    exe = _compile(tmp_path_factory, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "test_gicp_san")
    S, Q = ref.scene(600)
    cmds = [reg_command(S, Q, want_cov=True), reg_command(S, Q, max_corr=1.0), reg_command(S, Q, k_neighbors=32, max_iter=3),
            reg_command(S[:129], Q[:10], k_neighbors=10), reg_command(S, Q, max_cells=100.0), reg_command(S, Q, grid_cell=0.25, max_iter=2),
            reg_command(S, Q, grid_cell=1000.0, max_iter=2), reg_command(S, Q, T_init=np.hstack([np.eye(3), [[30.0], [0.0], [0.0]]]))]
    cmds += [reg_command(s, q, want_cov=True, **kw) for _, s, q, kw, _ in status_runs()]
    knn, nn = search_fixtures()
    cmds += [knn_command(P, k, h) for P, k in knn for h in CELLS] + [nn_command(s, q, h, mc) for s, q, mc in nn for h in CELLS]
    run_program(exe, cmds, tmp_path)


def test_declared_and_bound():
    """The C-ABI declares the entry point and the Python side binds it with the contract's constants."""
    from beam_slam_amd import capi, gpu
    text = open(os.path.join(ROOT, "include", "bsgpu.h")).read()
    assert "int bsgpu_register_scans_gicp(int device, int32_t n_pairs" in text and "register_scans_gicp" in capi.SYMBOLS
    assert (capi.GICP_MAX_ITERATIONS, capi.GICP_TRANSFORM, capi.GICP_TOO_FEW_CORRESPONDENCES, capi.GICP_DEGENERATE) == \
        (ref.MAX_ITERATIONS, ref.TRANSFORM, ref.TOO_FEW, ref.DEGENERATE)
    for name, k in (("MAX_ITERATIONS", 1), ("TRANSFORM", 2), ("TOO_FEW_CORRESPONDENCES", 5), ("DEGENERATE", 6)):
        assert f"BSGPU_GICP_{name} = {k}" in text
    assert capi.GICP_MAX_K == 32 and "#define BSGPU_GICP_MAX_K 32" in text
    assert capi.GICP_MAX_INNER == 64 and "#define BSGPU_GICP_MAX_INNER 64" in text
    header = open(os.path.join(INC, "gicp.h")).read()
    assert "constexpr int kGicpMaxK = 32;" in header and "constexpr int kGicpMaxInner = 64;" in header and "kGicpPivot = 1e-12;" in header
    assert len(capi.REGISTER_SCANS_GICP_ARGTYPES) == 25 and callable(gpu.register_scans_gicp)
    assert {k: capi.GICP_DEFAULTS[k] for k in ref.DEFAULTS} == ref.DEFAULTS and capi.GICP_DEFAULTS["grid_cell"] == 0.5
