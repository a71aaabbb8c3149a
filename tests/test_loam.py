"""bsgpu_register_scans_loam on the CPU: beam_slam_amd/csrc/loam.h (through tests/plan/test_loam.cpp, the kernel's arithmetic and order
of addition on one core) against the NumPy restatement of the contract (tests/loam_ref.py: brute-force neighbours, plain sums, the
Levenberg-Marquardt loop written out, numpy.linalg for the 6 x 6, numpy's sines).

Scenes (loam_ref.scene): features at random positions on the 12 edges and the 6 faces of icp_ref's 20 x 14 x 5 m box, the target drawn
separately, moved by icp_ref's motion, 1 cm noise: a small one (target 150 + 300 features against 600 + 1 200) and one of several chunks
(700 + 1 500 against 3 000 + 6 000).  The reference clouds are sparse (a surface point per 0.75 m^2 in the small scene), so the cases
widen max_corr from the shipped 0.5 m to what the third-nearest surface point needs.  Before anything is compared every case asserts
that its input can be compared: the four margins of loam_ref exceed 1e-9 and the restatement's variants agree on status and counts.

Accuracy criterion (test_icp.py's): status and all counts equal; rotation block and translation of T_refest_ref, cost and covariance
within 8 x the restatement's own spread (the largest difference among its three orders of summation), and not below 2^-52 of the quantity's largest magnitude.
"""
import os
import subprocess

import numpy as np
import pytest

import loam_ref as ref
from test_icp import grid_clouds, run_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plan", "test_loam.cpp")
INC = os.path.join(ROOT, "beam_slam_amd", "csrc")
MAX_CELLS = float(1 << 22)
GRID_CELL = 0.5
CELLS = (1.0, 0.37, 2.5, 1000.0)


def reg_command(clouds, T_init=None, max_cells=MAX_CELLS, grid_cell=GRID_CELL, inner=None, **kw):
    d, o = dict(ref.DEFAULTS, **kw), dict(ref.INNER, **(inner or {}))
    clouds = [np.asarray(c, float).reshape(-1, 3) for c in clouds]
    head = [1] + [len(c) for c in clouds] + [0 if T_init is None else 1, d["max_corr"], d["min_measurements"], d["max_outer"], d["conv_translation_m"],
                                             d["conv_rotation_deg"], d["loss_kind"], d["loss_a"], grid_cell, max_cells, o["max_num_iterations"],
                                             o["function_tolerance"], o["gradient_tolerance"], o["parameter_tolerance"]]
    return np.concatenate([np.array(head, float)] + [c.ravel() for c in clouds] + [np.zeros(0) if T_init is None else np.asarray(T_init, float).ravel()])


def nn_command(k, P, X, h, max_corr):
    return np.concatenate([np.array([2, k, len(P), len(X), h, max_corr], float), np.asarray(P, float).ravel(), np.asarray(X, float).ravel()])


def parse_reg(tok):
    v = [float(x) for x in tok[9:]]
    return dict(ok=int(tok[2]), status=int(tok[3]), n_iters=int(tok[4]), n_inner=int(tok[5]), n_edge=int(tok[6]), n_surf=int(tok[7]), cost=float(tok[8]),
                T_refest_ref=np.array(v[0:12]).reshape(3, 4), T_ref_tgt=np.array(v[12:24]).reshape(3, 4), cov=np.array(v[24:60]).reshape(6, 6))


def _compile(tmp_path_factory, flags, name):
    exe = str(tmp_path_factory.mktemp("loam") / name)
    # -ffp-contract=off: the header's pragma is clang's; GCC gets the same rule from the command line (loam.h, "Bits").  The HIP
    # include path: frame_lm.h reaches bsgpu_internal.h, whose declarations name HIP types.
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", INC, SRC, "-o", exe] + flags,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"], "test_loam")


def comparable(name):
    """The condition on the input: every neighbour, threshold, trust-region and outer decision of the case is far above rounding, and the
    restatement's variants made the same decisions."""
    clouds, kw, Ti, results, want = ref.case(name)
    for v, r in results.items():
        assert min(r["knn_gap"], r["margin"], r["lm_margin"], r["outer_margin"]) > 1e-9, (name, v, r["knn_gap"], r["margin"], r["lm_margin"], r["outer_margin"])
    assert len({tuple(r[k] for k in ref.COUNTS) for r in results.values()}) == 1, name
    return clouds, kw, Ti, results, want


def counts(r):
    return tuple(r[k] for k in ref.COUNTS)


def search_fixtures():
    """[(k, searched cloud, queries, max_corr)]: the grid_clouds() of test_icp as (queries S, cloud Q) — integer coordinates, so that
    there are ties at the k-th place, points on cell faces, k-th neighbours at exactly max_corr (which the strict < drops), duplicate
    points (a == b) and collinear triples; a cloud one cell thick; queries far outside the box — and clouds of 0, 1 and 2 points."""
    out = []
    for S, Q, h in grid_clouds():
        for k in (2, 3):
            out.append((k, Q, S, 1.0))
            out.append((k, Q, S, np.sqrt(2.0)))
            out.append((k, Q, S, 3.0))
    X = grid_clouds()[0][0]
    for n in (0, 1, 2):
        for k in (2, 3):
            out.append((k, np.array([[1.0, 0.0, -1.0], [0.0, 0.0, -1.0]])[:n], X, 5.0))
    dup = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [3.0, 0.0, 0.0]])     # duplicates; all collinear
    out += [(2, dup, X, 9.0), (3, dup, X, 9.0)]
    return out


def search_expected(k, P, X, max_corr):
    """(kept, indices) by brute force; also how many queries met a tie at the k-th place, the threshold exactly, a degenerate set"""
    P, X = np.asarray(P, float).reshape(-1, 3), np.asarray(X, float).reshape(-1, 3)
    idx, d2, nxt = ref.knn(P, X, k)
    kept = (ref.keep_edges if k == 2 else ref.keep_surfaces)(P, idx, d2, max_corr * max_corr)
    below = d2[:, k - 1] < max_corr * max_corr
    return kept, idx, int((d2[:, k - 1] == nxt).sum()), int((d2[:, k - 1] == max_corr * max_corr).sum()), int((below & ~kept).sum())


# ---- the header against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.CASES))
def test_header_against_restatement(name, core, tmp_path):
    """Measured (CPU build, g++ -O2), per case: status, outer / inner iterations, kept edges + surfaces, the margins (knn gap, threshold
    margin, LM margin, outer margin), rejected LM steps / residuals beyond the Huber scale, and the largest difference / bound:
        small_trivial  TRANSFORM  5 / 70   150 + 299   4.8e-5  1.0e-3  2.1e-2  4.5e-1   0 / 0      R 0.11  t 0.13  cost 0.09  cov 0.20
        small_huber    TRANSFORM  3 / 19   150 + 299   5.8e-5  5.0e-2  5.1e-2  3.8e-1   0 / 411    R 0.04  t 0.02  cost 0.13  cov 0.23
        small_one      MAX_ITER   1 / 31   150 + 299   5.8e-5  2.2e-1  2.1e-2  -        0 / 0      R 0.01  t 0.02  cost 0.00  cov 0.01
        small_three    MAX_ITER   3 / 19   150 + 299   5.7e-6  4.9e-2  3.0e-2  2.5e-3   0 / 386    R 0.06  t 0.13  cost 0.03  cov 0.18
        small_offset   TRANSFORM  7 / 127  150 + 300   1.1e-4  3.6e-2  3.1e-2  3.0e-1   4 / 0      R 0.25  t 0.21  cost 0.06  cov 0.09
        large_huber    TRANSFORM  5 / 35   700 + 1500  7.3e-7  4.0e-3  1.1e-1  1.5e-1   0 / 1995   R 0.03  t 0.07  cost 0.11  cov 0.04
    The restatement's own spread is 0 .. 5.2e-15 in R (the bound is then mostly its floor, 2^-52), 9e-16 .. 4.4e-15 in t, 2e-16 .. 1.8e-15
    in cost and 4e-17 .. 9.6e-16 in the covariance.
    """
    clouds, kw, Ti, results, want = comparable(name)
    res = results["plain"]
    got = parse_reg(run_program(core, [reg_command(clouds, T_init=Ti, **kw)], tmp_path)[0])
    print(f"{name}: status {res['status']}, {res['n_iters']} / {res['n_inner']} iterations, kept {res['n_edge']} + {res['n_surf']}, knn gap {res['knn_gap']:.3e}, "
          f"margin {res['margin']:.3e}, LM margin {res['lm_margin']:.3e}, outer margin {res['outer_margin']:.3e}, rejected {res['fates'].count('rejected')}, "
          f"beyond the Huber scale {res['huber_active']}")
    assert got["ok"] == 1 and counts(got) == counts(res) and res["status"] == want
    ref.check(got, results, "header " + name)
    assert np.abs(got["T_ref_tgt"] - res["T_ref_tgt"]).max() < 1e-12
    if name == "small_offset":
        assert res["fates"].count("rejected") >= 1
    if "huber" in name:
        assert res["huber_active"] > 0.2 * (res["n_edge"] + res["n_surf"])
    if name == "small_one":
        assert kw["max_outer"] == 1 and got["n_iters"] == 1


def test_search_is_exact(core, tmp_path):
    """The header's 2 and 3 nearest through the grid at four cell edges, and its two correspondence rules, are brute force's by
    (d^2, index)."""
    fixtures = search_fixtures()
    rows = iter(run_program(core, [nn_command(k, P, X, h, mc) for k, P, X, mc in fixtures for h in CELLS], tmp_path))
    ties = on_threshold = degenerate = 0
    for k, P, X, mc in fixtures:
        kept, idx, a, b, c = search_expected(k, P, X, mc)
        ties, on_threshold, degenerate = ties + a, on_threshold + b, degenerate + c
        want = np.concatenate([kept[:, None].astype(int), idx], axis=1).ravel()
        for h in CELLS:
            assert [int(t) for t in next(rows)[2:]] == list(want), (k, len(P), mc, h)
    assert ties > 50 and on_threshold > 50 and degenerate > 50      # the fixtures do exercise the tie rule, the strict threshold, the degeneracies


def status_runs():
    """(name, clouds, keyword arguments, the status it must end with)"""
    RE, RS, TE, TS = ref.scene(*ref.SMALL)
    none = RE[:0]
    kw = dict(max_corr=1.5)
    line = np.array([[0.0, 0.0, 0.0], [1e-200, 0.0, 0.0]])       # a != b, |a - b|^2 underflows: the residual is 0 / 0
    near = np.random.default_rng(1).uniform(-0.5, 0.5, size=(40, 3))
    few = (RE, RS, TE[:10], TS[:19])
    kept = ref.run(*few, **dict(ref.DEFAULTS, max_corr=1.5, min_measurements=1, max_outer=1))
    kept = kept["n_edge"] + kept["n_surf"]                           # (28 of the 29: a feature near a corner has no third neighbour in reach)
    return [("max_outer", (RE, RS, TE, TS), dict(kw, max_outer=2, conv_translation_m=0.0), ref.MAX_ITERATIONS),
            ("one iteration", (RE, RS, TE, TS), dict(kw, max_outer=1), ref.MAX_ITERATIONS),
            ("transform", (RE, RS, TE, TS), kw, ref.TRANSFORM),
            ("edges only", (RE, none, TE, none), kw, ref.TRANSFORM),
            ("surfaces only", (none, RS, none, TS), kw, ref.TRANSFORM),
            ("no features", (RE, RS, none, none), kw, ref.TOO_FEW),
            ("no reference", (none, none, TE, TS), kw, ref.TOO_FEW),
            ("one too few", few, dict(kw, min_measurements=kept + 1), ref.TOO_FEW),
            ("just enough", few, dict(kw, min_measurements=kept, max_outer=2), ref.MAX_ITERATIONS),
            ("solver failed", (line, none, near, none), dict(kw, min_measurements=1), ref.SOLVER_FAILED)]


def test_every_status(core, tmp_path):
    runs = status_runs()
    rows = run_program(core, [reg_command(c, **kw) for _, c, kw, _ in runs], tmp_path)
    for (name, c, kw, want), tok in zip(runs, rows):
        got, res = parse_reg(tok), ref.run(*c, **dict(ref.DEFAULTS, **kw))
        assert got["ok"] == 1 and got["status"] == res["status"] == want, (name, got["status"], res["status"])
        assert counts(got) == counts(res), (name, counts(got), counts(res))
        if want in (ref.TOO_FEW, ref.SOLVER_FAILED):
            assert got["n_iters"] == 0 and (got["T_refest_ref"] == ref.EYE).all() and np.isnan(got["cov"]).all(), name      # T stays as it was
        else:
            assert np.abs(got["T_refest_ref"] - res["T_refest_ref"]).max() < 1e-11 and np.isfinite(got["cov"]).all(), name
            assert np.abs(got["cov"] - res["cov"]).max() <= 1e-9 * np.abs(res["cov"]).max(), name
        if name == "one too few":
            assert got["n_edge"] + got["n_surf"] == kw["min_measurements"] - 1 > 20
        if name == "solver failed":
            assert got["n_edge"] == 40 and not np.isfinite(got["cost"])


def test_grid_cell_is_a_performance_knob_only(core, tmp_path):
    """The small Huber case at cell edges 0.25, 0.5 and 1000 (one cell): every output, the covariance included, has the same bytes."""
    clouds, kw, Ti, _, _ = ref.case("small_huber")
    rows = run_program(core, [reg_command(clouds, grid_cell=h, **kw) for h in (0.25, 0.5, 1000.0)], tmp_path)
    assert rows[0][2] == "1" and len(rows[0]) == 9 + 60
    for tok in rows[1:]:
        assert tok[2:] == rows[0][2:]


def quarter_turn(P, Ti):
    """The points that the exact quarter turn Ti takes to P"""
    back = np.asarray(P) - Ti[:, 3]
    return np.stack([back[:, 1], -back[:, 0], back[:, 2]], axis=1)


QUARTER = np.array([[0.0, -1.0, 0.0, 0.25], [1.0, 0.0, 0.0, -1.5], [0.0, 0.0, 1.0, 0.125]])


def test_initial_transform_and_composition(core, tmp_path):
    """T_init is applied to the target features first: a quarter turn about z and a translation, whose products are exact, give the
    bits of the call on the features transformed beforehand; T_ref_tgt = T T_init = inv(T_refest_ref) T_init."""
    clouds, kw, _, _, _ = ref.case("small_huber")
    RE, RS, TE, TS = clouds
    raw = (RE, RS, quarter_turn(TE, QUARTER), quarter_turn(TS, QUARTER))
    moved = (RE, RS, ref.transform(QUARTER, raw[2]), ref.transform(QUARTER, raw[3]))
    a, b = (parse_reg(t) for t in run_program(core, [reg_command(raw, T_init=QUARTER, **kw), reg_command(moved, **kw)], tmp_path))
    assert a["status"] == ref.TRANSFORM and counts(a) == counts(b)
    assert a["T_refest_ref"].tobytes() == b["T_refest_ref"].tobytes() and a["cost"] == b["cost"] and a["cov"].tobytes() == b["cov"].tobytes()
    T4, Ti4 = np.vstack([a["T_refest_ref"], [0, 0, 0, 1]]), np.vstack([QUARTER, [0, 0, 0, 1]])
    assert np.abs(np.linalg.inv(T4) @ Ti4 - np.vstack([a["T_ref_tgt"], [0, 0, 0, 1]])).max() < 1e-13


def test_cell_cap(core, tmp_path):
    """A grid of more cells than the cap is refused, not built."""
    clouds, kw, _, _, _ = ref.case("small_huber")
    tok = run_program(core, [reg_command(clouds, max_cells=100.0, **kw), reg_command(clouds, max_cells=42 * 30 * 12, **kw)], tmp_path)
    assert parse_reg(tok[0])["ok"] == 0 and parse_reg(tok[1])["ok"] == 1


def test_truth_recovery(core, tmp_path):
    """The header's distance to the truth (the scene's motion) on the small Huber scene is the restatement's own: the bound is twice the
    restatement's distance, which its 1 cm noise decides (measured: 2.4e-3 in the largest entry of T_ref_tgt), and the two agree to
    1e-12."""
    clouds, kw, Ti, results, _ = ref.case("small_huber")
    res = results["plain"]
    own = np.abs(res["T_ref_tgt"] - ref.MOTION).max()
    got = parse_reg(run_program(core, [reg_command(clouds, **kw)], tmp_path)[0])
    err = np.abs(got["T_ref_tgt"] - ref.MOTION).max()
    print(f"truth: the restatement's distance {own:.3e}, the header's {err:.3e}")
    assert own < 0.01 and err <= 2.0 * own and abs(err - own) < 1e-12


def test_header_under_sanitizers(tmp_path_factory, tmp_path):
    """The header as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, arrays of exact size: the small
    cases, every status, the empty clouds, the cell edges and the search fixtures run clean."""
    exe = _compile(tmp_path_factory, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "test_loam_san")
    cmds = []
    for name in ("small_trivial", "small_huber", "small_one", "small_offset"):
        clouds, kw, Ti, _, _ = ref.case(name)
        cmds.append(reg_command(clouds, T_init=Ti, **kw))
    clouds, kw, _, _, _ = ref.case("small_huber")
    cmds += [reg_command(clouds, max_cells=100.0, **kw), reg_command(clouds, grid_cell=0.25, **dict(kw, max_outer=2)),
             reg_command(clouds, grid_cell=1000.0, **dict(kw, max_outer=2)), reg_command(tuple(c[:129] for c in clouds), **dict(kw, max_outer=2))]
    cmds += [reg_command(c, **kw) for _, c, kw, _ in status_runs()]
    cmds += [nn_command(k, P, X, h, mc) for k, P, X, mc in search_fixtures() for h in CELLS]
    run_program(exe, cmds, tmp_path)


def test_declared_and_bound():
    """The C-ABI declares the entry point and the Python side binds it with the contract's constants."""
    from beam_slam_amd import capi, gpu
    text = open(os.path.join(ROOT, "include", "bsgpu.h")).read()
    assert "int bsgpu_register_scans_loam(int device, int32_t n_pairs" in text and "register_scans_loam" in capi.SYMBOLS
    assert (capi.LOAM_MAX_ITERATIONS, capi.LOAM_TRANSFORM, capi.LOAM_TOO_FEW_MEASUREMENTS, capi.LOAM_SOLVER_FAILED) == \
        (ref.MAX_ITERATIONS, ref.TRANSFORM, ref.TOO_FEW, ref.SOLVER_FAILED)
    for name, k in (("MAX_ITERATIONS", 1), ("TRANSFORM", 2), ("TOO_FEW_MEASUREMENTS", 5), ("SOLVER_FAILED", 6)):
        assert f"BSGPU_LOAM_{name} = {k}" in text
    header = open(os.path.join(INC, "loam.h")).read()
    for name, value, const in (("MAX_OUTER", 100, "kLoamMaxOuter"), ("MAX_INNER", 1000, "kLoamMaxInner"), ("MAX_FEATURES", 65536, "kLoamMaxFeatures")):
        assert getattr(capi, "LOAM_" + name) == value and f"#define BSGPU_LOAM_{name} {value}" in text and f"constexpr int {const} = {value};" in header
    assert "RECALLED" in text[text.index("LOAM feature registration"):] and "NOT MODELLED" in text
    assert len(capi.REGISTER_SCANS_LOAM_ARGTYPES) == 29 and callable(gpu.register_scans_loam)
    assert {k: capi.LOAM_DEFAULTS[k] for k in ref.DEFAULTS} == ref.DEFAULTS and capi.LOAM_DEFAULTS["inner"] == ref.INNER
    assert capi.LOAM_DEFAULTS["grid_cell"] == 0.5 and (capi.LOSS_TRIVIAL, capi.LOSS_CAUCHY, capi.LOSS_HUBER) == (ref.TRIVIAL, ref.CAUCHY, ref.HUBER)
