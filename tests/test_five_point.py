"""The five-point RANSAC core (beam_slam_amd/csrc/five_point.h) on the CPU against tests/essential_ref.py, an independent NumPy
restatement (SVD null space, dictionary polynomials, eigenvalues of the action matrix): tests/plan/test_five_point.cpp runs the
header's serial compositions, fpr_five_point / fpr_sample / fpr_ransac_serial.

Minimal solver, 500 seeded noise-free five-match problems.  Cases whose 5x5 epipolar Jacobian at the truth has a condition number
above 1e5 are left out (at most 2 % may be; with these seeds none is).  The tolerance is not fixed
in advance: it is 100 x the reference's own worst distance to the true E over the kept cases, floor 1e-12, and the same margin over
the reference's worst constraint residual.  Measured: the reference's worst distance to the truth is 1.107e-05 (median 2.750e-13),
the header's 2.097e-12 (median 1.129e-14); the reference's worst residual is 2.014e-08, the header's 3.990e-16; the two find the
same number of solutions in all 500 cases."""
import os
import subprocess

import numpy as np
import pytest

import essential_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("five_point") / "test_five_point")
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                          os.path.join(ROOT, "tests", "plan", "test_five_point.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]

    def run(lines, tmp_path):
        path = tmp_path / "commands.txt"
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        res = {}
        for line in r.stdout.splitlines():
            t = line.split()
            if t[0] == "DONE":
                continue
            res.setdefault(int(t[1]), {}).setdefault(t[0], []).append(t[2:])
        return res
    return run


def _f(v):
    return " ".join(repr(float(x)) for x in np.ravel(v))


def _residuals(E, x1, x2):
    h1 = np.column_stack([x1, np.ones(5)])
    h2 = np.column_stack([x2, np.ones(5)])
    epi = np.abs(np.einsum("ni,ij,nj->n", h2, E, h1)).max()
    return max(epi, np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max())


def test_minimal_solver_against_reference(core, tmp_path):
    cases = [ref.minimal_case(seed) for seed in range(500)]
    kept = [c for c in cases if c[3] <= 1e5]
    assert len(kept) >= 0.98 * len(cases)
    got = core(["SOLVE " + _f(np.column_stack([x1, x2])) for x1, x2, _, _ in kept], tmp_path)
    refs = [ref.five_point(x1, x2) for x1, x2, _, _ in kept]
    ref_err = np.array([min(ref.dist_E(E, c[2]) for E in sols) for c, sols in zip(kept, refs)])
    ref_res = max(_residuals(E, c[0], c[1]) for c, sols in zip(kept, refs) for E in sols)
    tol, tol_res = max(100.0 * ref_err.max(), 1e-12), max(100.0 * ref_res, 1e-12)
    errs, ress = [], []
    for k, (c, sols) in enumerate(zip(kept, refs)):
        mine = [np.array([float(v) for v in e]).reshape(3, 3) for e in got[k].get("E", [])]
        assert int(got[k]["SOL"][0][0]) == len(mine) == len(sols), (k, len(mine), len(sols))
        errs.append(min(ref.dist_E(E, c[2]) for E in mine))
        for E in mine:
            assert abs(np.linalg.norm(E) - 1.0) <= 1e-14 and E.flat[np.argmax(np.abs(E))] > 0
            assert min(ref.dist_E(E, S) for S in sols) <= tol, k
            ress.append(_residuals(E, c[0], c[1]))
        assert all(a[0, 0] <= b[0, 0] for a, b in zip(mine, mine[1:])), k
    print(f"kept {len(kept)} of {len(cases)}; reference distance to the truth: max {ref_err.max():.3e} median {np.median(ref_err):.3e}; "
          f"header: max {max(errs):.3e} median {np.median(errs):.3e}; residuals: reference max {ref_res:.3e}, header max {max(ress):.3e}")
    assert max(errs) <= tol
    assert max(ress) <= tol_res


def test_sampler_matches_restatement(core, tmp_path):
    rng = np.random.default_rng(5)
    tuples = [(int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 200)), int(rng.integers(0, 5000)),
               5 if k % 10 == 0 else int(rng.integers(5, 5000))) for k in range(1000)]
    got = core([f"SAMPLE {seed} {st} {s} {n}" for seed, st, s, n in tuples], tmp_path)
    for k, (seed, st, s, n) in enumerate(tuples):
        idx = [int(v) for v in got[k]["IDX"][0]]
        assert idx == ref.sample_indices(seed, st, s, n), (seed, st, s, n)
        assert len(set(idx)) == 5 and all(0 <= i < n for i in idx)
        if n == 5:
            assert sorted(idx) == [0, 1, 2, 3, 4]


def _ransac_cmd(st, prob, thr, max_iters, seed, set_index):
    n = len(st["px_prev"])
    lines = [f"RANSAC {n} {prob!r} {thr!r} {max_iters} {seed} {set_index} " + _f(st["K"])]
    lines += [_f([*a, *b]) for a, b in zip(st["px_prev"], st["px_cur"])]
    return lines


def _parse_ransac(g):
    t = [int(v) for v in g["RES"][0]]
    mask = np.array([int(ch) for ch in (g["MASK"][0][0] if g["MASK"][0] else "")], np.uint8)
    return dict(status=t[0], n_inliers=t[1], n_iters=t[2], best_sample=np.array(t[3:8]), mask=mask,
                E=np.array([float(v) for v in g["EBEST"][0]]).reshape(3, 3))


@pytest.mark.parametrize("n,frac", [(40, 0.3), (40, 0.5), (300, 0.3), (300, 0.5)])
def test_serial_loop_on_gap_data(core, tmp_path, n, frac):
    st = ref.make_set(1000 + n + int(100 * frac), n, frac)
    seed = 77
    r = ref.ransac_serial(st["px_prev"], st["px_cur"], st["K"], 0.99, 1.0, 1000, seed, 3)
    g = _parse_ransac(core(_ransac_cmd(st, 0.99, 1.0, 1000, seed, 3), tmp_path)[0])
    assert r["status"] == ref.STATUS_OK and g["status"] == ref.STATUS_OK
    assert np.array_equal(r["mask"], st["labels"])
    assert np.array_equal(g["mask"], st["labels"])
    assert g["n_inliers"] == r["n_inliers"] == int(st["labels"].sum())
    assert g["n_iters"] == r["n_iters"]
    assert np.array_equal(g["best_sample"], r["best_sample"])


def test_serial_loop_too_few(core, tmp_path):
    st = ref.make_set(9, 4, 0.0)
    g = _parse_ransac(core(_ransac_cmd(st, 0.99, 1.0, 1000, 1, 0), tmp_path)[0])
    assert g["status"] == ref.STATUS_TOO_FEW and g["n_iters"] == 0 and g["n_inliers"] == 0
    assert np.all(g["mask"] == 1) and np.all(g["E"] == 0) and np.all(g["best_sample"] == -1)
