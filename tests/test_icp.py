"""bsgpu_register_scans on the CPU: beam_slam_amd/csrc/icp.h (through tests/plan/test_icp.cpp, the kernels' arithmetic and order of
addition on one core) against the NumPy restatement of the contract (tests/icp_ref.py: brute-force nearest neighbour, numpy.linalg.svd,
plain sums).

Scenes (icp_ref.scene): points on the faces of a 20 x 14 x 5 m box seen from inside, two independent 80 % subsamples, the target moved
by rotation vector (0.01, -0.02, 0.04) and translation (0.25, -0.15, 0.05), 1 cm noise, max_corr 1; 600 and 4 000 points, at the
shipped fit_eps 1e-2 and at fit_eps 0.  Before anything is compared every case asserts that its input can be compared: the smallest gap
between a source point's best and second-best squared distance, and the smallest distance of a squared distance from max_corr^2, over
all iterations, exceed 1e-9 m^2 (measured: see test_header_against_restatement).

Accuracy criterion: n_iters, status and n_corr equal; the rotation block, the translation and mse within 8 x the restatement's own
difference when its source points are summed in reversed order (not below 2^-52 of the quantity's largest magnitude).
"""
import os
import subprocess

import numpy as np
import pytest

import icp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plan", "test_icp.cpp")
INC = os.path.join(ROOT, "beam_slam_amd", "csrc")
MAX_CELLS = float(1 << 22)


def reg_command(S, Q, T_init=None, max_cells=MAX_CELLS, **kw):
    d = dict(ref.DEFAULTS, **kw)
    S, Q = np.asarray(S, float).reshape(-1, 3), np.asarray(Q, float).reshape(-1, 3)
    head = [1, len(S), len(Q), 0 if T_init is None else 1, d["max_corr"], d["max_iter"], d["t_eps"], d["fit_eps"], d["rotation_threshold"],
            d["rel_mse_eps"], max_cells]
    return np.concatenate([np.array(head, float), S.ravel(), Q.ravel(), np.zeros(0) if T_init is None else np.asarray(T_init, float).ravel()])


def nn_command(S, Q, h):
    return np.concatenate([np.array([2, len(S), len(Q), h], float), np.asarray(S, float).ravel(), np.asarray(Q, float).ravel()])


def run_program(exe, commands, tmp_path):
    """commands: arrays of doubles -> per command the program's output line as a token list."""
    path = tmp_path / "commands.bin"
    np.concatenate(commands).astype(np.float64).tofile(str(path))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"DONE {len(commands)}" in r.stdout and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if not ln.startswith("DONE")]
    assert [int(t[1]) for t in rows] == list(range(len(commands)))
    return rows


def parse_reg(tok):
    v = [float(x) for x in tok[6:]]
    return dict(ok=int(tok[2]), status=int(tok[3]), n_iters=int(tok[4]), n_corr=int(tok[5]), mse=v[0], T=np.array(v[1:13]).reshape(3, 4),
                T_ref_tgt=np.array(v[13:25]).reshape(3, 4))


def _compile(tmp_path_factory, flags, name):
    exe = str(tmp_path_factory.mktemp("icp") / name)
    # -ffp-contract=off: the header's pragma is clang's; GCC gets the same rule from the command line (icp.h, "Bits")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", INC, SRC, "-o", exe] + flags, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"], "test_icp")


def comparable(name):
    """The condition on the input: every nearest-neighbour and threshold decision of the case is far above rounding."""
    S, Q, kw, res, rev = ref.case(name)
    assert res["gap"] > 1e-9 and rev["gap"] > 1e-9 and res["margin"] > 1e-9, (name, res["gap"], res["margin"])
    assert (res["status"], res["n_iters"], res["n_corr"]) == (rev["status"], rev["n_iters"], rev["n_corr"]), name
    return S, Q, kw, res, rev


def grid_clouds():
    """Clouds on which a grid search can go wrong: integer coordinates with max_corr = 1, so that targets lie exactly on cell faces,
    exactly max_corr away, and at equal distances (the tie rule); half-integer sources; a target cloud one cell thick; sources far
    outside the target's box; one target; real-valued clouds."""
    rng = np.random.default_rng(11)
    out = []
    for k in range(6):
        Q = rng.integers(-3, 4, size=(40 + 30 * k, 3)).astype(float)
        S = rng.integers(-5, 6, size=(120, 3)).astype(float)
        out.append((S, Q, 1.0))
        out.append((S + 0.5 * rng.integers(0, 2, size=S.shape), Q, 1.0))
    flat = rng.integers(-4, 5, size=(60, 3)).astype(float)
    flat[:, 2] = 2.0
    out.append((rng.integers(-5, 6, size=(150, 3)).astype(float), flat, 1.0))
    out.append((np.array([[100.0, 0, 0], [0, -100.0, 0], [0.0, 0, 0], [1.0, 0, 0], [0, 0, 1e150], [2.0, 2, 3]]), flat, 1.0))
    out.append((rng.integers(-2, 3, size=(30, 3)).astype(float), np.array([[1.0, 0.0, -1.0]]), 1.0))
    Q = rng.uniform(-3, 3, size=(500, 3))
    out.append((rng.uniform(-4, 4, size=(300, 3)), Q, 0.7))
    out.append((Q[::-1] + 0.0, Q, 0.25))
    return out


# ---- the header against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.CASES))
def test_header_against_restatement(name, core, tmp_path):
    """Measured (CPU build, g++ -O2), per case: iterations / status, gap, margin, and the largest difference / bound:
        n600_fit     4 / ABS_MSE    gap 7.2e-5  margin 3.0e-3   R 0.056  t 0.125  mse 0.083
        n600_nofit   6 / TRANSFORM  gap 6.4e-6  margin 3.0e-3   R 0.050  t 0.080  mse 0.000
        n4000_fit    6 / ABS_MSE    gap 6.3e-6  margin 3.4e-1   R 0.234  t 0.055  mse 0.313
        n4000_nofit 10 / TRANSFORM  gap 1.2e-7  margin 3.2e-1   R 0.208  t 0.068  mse 0.188
    The restatement's own difference (reversed source order) is 8e-16 .. 1.4e-15 in R and t and 3e-18 .. 4e-17 in mse.
    """
    S, Q, kw, res, rev = comparable(name)
    got = parse_reg(run_program(core, [reg_command(S, Q, **kw)], tmp_path)[0])
    print(f"{name}: {res['n_iters']} iterations, status {res['status']}, n_corr {res['n_corr']}, gap {res['gap']:.3e}, margin {res['margin']:.3e}")
    assert got["ok"] == 1 and (got["status"], got["n_iters"], got["n_corr"]) == (res["status"], res["n_iters"], res["n_corr"])
    ref.check(got["T"], got["mse"], res, rev, "header " + name)
    assert np.abs(got["T_ref_tgt"] - res["T_ref_tgt"]).max() < 1e-12


def test_grid_search_is_exact(core, tmp_path):
    """For every source point the header's thresholded nearest neighbour through the grid is brute force's, ties to the lowest index."""
    clouds = grid_clouds()
    rows = run_program(core, [nn_command(S, Q, h) for S, Q, h in clouds], tmp_path)
    ties = on_threshold = 0
    for (S, Q, h), tok in zip(clouds, rows):
        j, d2, second = ref.nearest(S, Q)
        want = np.where(d2 <= h * h, j, -1)
        assert [int(t) for t in tok[2:]] == list(want), (len(S), len(Q), h)
        ties += int(((second == d2) & (d2 <= h * h)).sum())
        on_threshold += int((d2 == h * h).sum())
    assert ties > 50 and on_threshold > 50      # the fixtures do exercise the tie rule and the closed threshold


def test_every_status(core, tmp_path):
    S, Q = ref.scene(600)
    inside = np.asarray(S)[:40] * 0.2              # a small cloud; its copy 5 m above it
    runs = [("apart", inside, inside + [0.0, 0.0, 5.0], {}, ref.TOO_FEW), ("two points", S[:2], Q, {}, ref.TOO_FEW),
            ("no source", S[:0], Q, {}, ref.TOO_FEW), ("no target", S, Q[:0], {}, ref.TOO_FEW),
            ("max_iter", S, Q, dict(max_iter=2), ref.MAX_ITERATIONS), ("one iteration", S, Q, dict(max_iter=1), ref.MAX_ITERATIONS),
            ("transform", S, Q, dict(fit_eps=0.0), ref.TRANSFORM), ("abs mse", S, Q, {}, ref.ABS_MSE),
            ("rel mse", S, Q, dict(fit_eps=0.0, rel_mse_eps=0.5), ref.REL_MSE)]
    rows = run_program(core, [reg_command(s, q, **kw) for _, s, q, kw, _ in runs], tmp_path)
    for (name, s, q, kw, want), tok in zip(runs, rows):
        got, res = parse_reg(tok), ref.run(s, q, **dict(ref.DEFAULTS, **kw))
        assert got["ok"] == 1 and got["status"] == res["status"] == want, (name, got["status"], res["status"])
        assert (got["n_iters"], got["n_corr"]) == (res["n_iters"], res["n_corr"]), name
        if want == ref.TOO_FEW:
            assert got["n_iters"] == 0 and (got["T"] == ref.EYE).all() and got["n_corr"] < 3, name   # T stays as it was
        else:
            assert np.abs(got["T"] - res["T"]).max() < 1e-12, name


def test_truth_recovery(core, tmp_path):
    """target = T reference exactly, every point, no noise: the result is T to 1e-10."""
    S = ref.box_points(500, np.random.default_rng(3))
    T = np.hstack([ref.MOTION_R, ref.MOTION_T[:, None]])
    got = parse_reg(run_program(core, [reg_command(S, ref.transform(T, S), fit_eps=0.0)], tmp_path)[0])
    print(f"truth: {got['n_iters']} iterations, status {got['status']}, |T - truth| {np.abs(got['T'] - T).max():.3e}, mse {got['mse']:.3e}")
    assert got["status"] == ref.TRANSFORM and got["n_corr"] == 500 and np.abs(got["T"] - T).max() < 1e-10


def test_initial_transform_and_composition(core, tmp_path):
    """T_init is applied to the target first; T_ref_tgt = inv(T_refest_ref) T_init."""
    S, Q = ref.scene(600)
    Ti = np.hstack([ref.rotvec([0.0, 0.0, 0.02]), np.array([[0.1], [-0.05], [0.0]])])
    got = parse_reg(run_program(core, [reg_command(S, Q, T_init=Ti)], tmp_path)[0])
    res = ref.run(S, Q, T_init=Ti, **ref.DEFAULTS)
    assert (got["status"], got["n_iters"], got["n_corr"]) == (res["status"], res["n_iters"], res["n_corr"]) and res["gap"] > 1e-9
    assert np.abs(got["T"] - res["T"]).max() < 1e-12 and np.abs(got["T_ref_tgt"] - res["T_ref_tgt"]).max() < 1e-12
    T4, Ti4 = np.vstack([got["T"], [0, 0, 0, 1]]), np.vstack([Ti, [0, 0, 0, 1]])
    assert np.abs(np.linalg.inv(T4) @ Ti4 - np.vstack([got["T_ref_tgt"], [0, 0, 0, 1]])).max() < 1e-13


def test_cell_cap(core, tmp_path):
    """A grid of more cells than the cap is refused, not built."""
    S, Q = ref.scene(600)
    tok = run_program(core, [reg_command(S, Q, max_cells=100.0), reg_command(S, Q, max_cells=21 * 15 * 6)], tmp_path)
    assert parse_reg(tok[0])["ok"] == 0 and parse_reg(tok[1])["ok"] == 1


def test_header_under_sanitizers(tmp_path_factory, tmp_path):
    """The header as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, arrays of exact size: the
    600-point cases, every status, the empty clouds and the grid fixtures run clean."""
    exe = _compile(tmp_path_factory, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "test_icp_san")
    S, Q = ref.scene(600)
    cmds = [reg_command(S, Q), reg_command(S, Q, fit_eps=0.0), reg_command(S[:2], Q), reg_command(S[:0], Q), reg_command(S, Q[:0]),
            reg_command(S, Q, max_iter=2), reg_command(S[:129], Q[:1]), reg_command(S, Q, max_cells=100.0),
            reg_command(S, Q, T_init=np.hstack([np.eye(3), [[30.0], [0.0], [0.0]]]))]
    cmds += [nn_command(s, q, h) for s, q, h in grid_clouds()]
    run_program(exe, cmds, tmp_path)


def test_declared_and_bound():
    """The C-ABI declares the entry point and the Python side binds it with the contract's constants."""
    from beam_slam_amd import capi, gpu
    text = open(os.path.join(ROOT, "include", "bsgpu.h")).read()
    assert "int bsgpu_register_scans(int device, int32_t n_pairs" in text and "register_scans" in capi.SYMBOLS
    assert (capi.ICP_MAX_ITERATIONS, capi.ICP_TRANSFORM, capi.ICP_ABS_MSE, capi.ICP_REL_MSE, capi.ICP_TOO_FEW_CORRESPONDENCES) == \
        (ref.MAX_ITERATIONS, ref.TRANSFORM, ref.ABS_MSE, ref.REL_MSE, ref.TOO_FEW)
    for k, name in enumerate(("MAX_ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "TOO_FEW_CORRESPONDENCES"), start=1):
        assert f"BSGPU_ICP_{name} = {k}" in text
    assert capi.ICP_MAX_CELLS == 1 << 22 and "#define BSGPU_ICP_MAX_CELLS (1 << 22)" in text
    assert len(capi.REGISTER_SCANS_ARGTYPES) == 19 and callable(gpu.register_scans)
    assert {k: capi.ICP_DEFAULTS[k] for k in ref.DEFAULTS} == ref.DEFAULTS
