"""The P3P RANSAC core (beam_slam_amd/csrc/p3p.h) on the CPU against tests/p3p_ref.py, an independent NumPy restatement (the quartic
from the resultant of two conics, poses by Kabsch): tests/plan/test_p3p.cpp runs the header's serial compositions, p3p_solve /
p3p_sample / p3p_ransac_serial.

Minimal solver, 500 seeded noise-free triplets.  Cases in which two roots of the reference's quartic lie within a relative 1e-3 of
each other are left out (at most 2 % may be).  The tolerance is not fixed in advance: it is 100 x the reference's own worst distance
to the true pose over the kept cases (largest absolute difference of an entry of [R|t]), floor 1e-12, and the same margin over the
reference's worst constraint residual (|depth * bearing - P_c| / depth).  Measured values: see test_minimal_solver_against_reference."""
import os
import subprocess

import numpy as np
import pytest

import p3p_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("p3p") / "test_p3p")
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                          os.path.join(ROOT, "tests", "plan", "test_p3p.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
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


def test_minimal_solver_against_reference(core, tmp_path):
    """Measured (500 seeds, 498 kept): the reference's worst distance to the truth 1.127e-08 (median 6.006e-14), the header's
    9.124e-12 (median 8.882e-15); the reference's worst constraint residual 6.398e-10, the header's 1.182e-13; the two find the same
    number of solutions in every kept case."""
    K = ref.K_DEFAULT
    cases = [ref.minimal_case(seed) for seed in range(500)]
    full = [ref.p3p(c[0], c[1], K, with_roots=True) for c in cases]
    keep = [k for k in range(len(cases)) if not ref.near_double(full[k][1])]
    assert len(keep) >= 0.98 * len(cases)
    kept = [cases[k] for k in keep]
    refs = [full[k][0] for k in keep]
    got = core(["SOLVE " + _f(K) + " " + _f(c[0]) + " " + _f(c[1]) for c in kept], tmp_path)
    ref_err = np.array([min(ref.pose_dist(s, c[2], c[3]) for s in sols) for c, sols in zip(kept, refs)])
    ref_res = max(ref.constraint_residual(R, t, c[0], c[1], K) for c, sols in zip(kept, refs) for R, t in sols)
    tol, tol_res = max(100.0 * ref_err.max(), 1e-12), max(100.0 * ref_res, 1e-12)
    errs, ress = [], []
    for k, (c, sols) in enumerate(zip(kept, refs)):
        mine = [np.array([float(v) for v in e]).reshape(3, 4) for e in got[k].get("T", [])]
        mine = [(T[:, :3], T[:, 3]) for T in mine]
        assert int(got[k]["SOL"][0][0]) == len(mine) == len(sols), (keep[k], len(mine), len(sols))
        assert 1 <= len(mine) <= 4
        errs.append(min(ref.pose_dist(s, c[2], c[3]) for s in mine))
        depth = [(R @ c[1][0] + t)[2] for R, t in mine]
        assert all(a <= b for a, b in zip(depth, depth[1:])), keep[k]
        for R, t in mine:
            assert np.all((c[1] @ R.T + t)[:, 2] > 0)
            assert min(ref.pose_dist((R, t), *s) for s in sols) <= tol, keep[k]
            ress.append(ref.constraint_residual(R, t, c[0], c[1], K))
    print(f"kept {len(kept)} of {len(cases)}; reference distance to the truth: max {ref_err.max():.3e} median {np.median(ref_err):.3e}; "
          f"header: max {max(errs):.3e} median {np.median(errs):.3e}; residuals: reference max {ref_res:.3e}, header max {max(ress):.3e}")
    assert max(errs) <= tol
    assert max(ress) <= tol_res


def test_sampler_matches_restatement(core, tmp_path):
    rng = np.random.default_rng(5)
    tuples = [(int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 200)), int(rng.integers(0, 5000)),
               3 if k % 10 == 0 else int(rng.integers(3, 5000))) for k in range(1000)]
    got = core([f"SAMPLE {seed} {fr} {s} {n}" for seed, fr, s, n in tuples], tmp_path)
    for k, (seed, fr, s, n) in enumerate(tuples):
        idx = [int(v) for v in got[k]["IDX"][0]]
        assert idx == ref.sample_indices(seed, fr, s, n), (seed, fr, s, n)
        assert len(set(idx)) == 3 and all(0 <= i < n for i in idx)
        if n == 3:
            assert sorted(idx) == [0, 1, 2]


def _ransac_cmd(fr, prob, thr, max_iters, seed, frame_index, truncate=0):
    n = len(fr["pixels"])
    lines = [f"RANSAC {n} {prob!r} {thr!r} {max_iters} {seed} {frame_index} {truncate} " + _f(fr["K"])]
    lines += [_f([*a, *b]) for a, b in zip(fr["pixels"], fr["points"])]
    return lines


def _parse_ransac(g):
    t = [int(v) for v in g["RES"][0]]
    mask = np.array([int(ch) for ch in (g["MASK"][0][0] if g["MASK"][0] else "")], np.uint8)
    return dict(status=t[0], n_inliers=t[1], n_iters=t[2], best_sample=np.array(t[3:6]), mask=mask,
                T=np.array([float(v) for v in g["TBEST"][0]]).reshape(3, 4))


@pytest.mark.parametrize("prob,max_iters", [(0.99, 1000), (0.0, 100)])
@pytest.mark.parametrize("n,n_out", [(40, 12), (300, 90), (300, 150)])
def test_serial_loop_on_gap_data(core, tmp_path, n, n_out, prob, max_iters):
    """Noise-free inliers, outliers at least 10 px off or behind the camera, 5 px: the mask is the labels, and n_iters, n_inliers and
    best_sample are the reference loop's — with early termination and with libbeam's fixed 100 iterations (prob = 0)."""
    fr = ref.make_frame(1000 + n + n_out, n, n_out)
    seed = 77
    r = ref.ransac_serial(fr["pixels"], fr["points"], fr["K"], prob, 5.0, max_iters, seed, 3)
    g = _parse_ransac(core(_ransac_cmd(fr, prob, 5.0, max_iters, seed, 3), tmp_path)[0])
    assert r["status"] == ref.STATUS_OK and g["status"] == ref.STATUS_OK
    assert np.array_equal(r["mask"], fr["labels"])
    assert np.array_equal(g["mask"], fr["labels"])
    assert g["n_inliers"] == r["n_inliers"] == int(fr["labels"].sum())
    assert g["n_iters"] == r["n_iters"]
    if prob == 0.0:
        assert g["n_iters"] == 100
    assert np.array_equal(g["best_sample"], r["best_sample"])
    assert ref.pose_dist((g["T"][:, :3], g["T"][:, 3]), fr["R"], fr["t"]) <= max(100.0 * ref.pose_dist((r["R"], r["t"]), fr["R"], fr["t"]), 1e-12)


def test_serial_loop_too_few(core, tmp_path):
    fr = ref.make_frame(9, 3, 0)
    g = _parse_ransac(core(_ransac_cmd(fr, 0.99, 5.0, 1000, 1, 0), tmp_path)[0])
    assert g["status"] == ref.STATUS_TOO_FEW and g["n_iters"] == 0 and g["n_inliers"] == 0
    assert np.all(g["mask"] == 0) and np.all(np.isnan(g["T"])) and np.all(g["best_sample"] == -1)
