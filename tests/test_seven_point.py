"""The seven-point RANSAC core (beam_slam_amd/csrc/seven_point.h) on the CPU against tests/seven_point_ref.py, an independent NumPy
restatement (null space, decomposition and triangulation by LAPACK's SVD, the cubic by numpy.roots): tests/plan/test_seven_point.cpp
runs the header's serial compositions, sp7_solve / sp7_sample / sp7_ransac_serial.

Minimal solver, 500 seeded noise-free 7-tuples.  Cases in which two roots of the reference's cubic lie within a relative 1e-3 of each
other, or the seventh singular value of the 7 x 9 system is below 1e-6 of the first, are left out (at most 2 % may be).  The tolerance
is not fixed in advance: it is 100 x the reference's own worst distance to the truth over the kept cases (largest absolute difference of
an entry of E, and of [R|t] for the pose), floor 1e-12.  Measured values: see test_minimal_solver_against_reference."""
import os
import subprocess

import numpy as np
import pytest

import seven_point_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = ref.K_DEFAULT


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sp7") / "test_seven_point")
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                          os.path.join(ROOT, "tests", "plan", "test_seven_point.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
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


def _in_front(R, t, x0, x1):
    X = ref.triangulate(R, t, x0, x1)
    return bool(np.all(np.isfinite(X)) and np.all(X[:, 2] > 0) and np.all((X @ R.T + t)[:, 2] > 0))


def test_minimal_solver_against_reference(core, tmp_path):
    """Measured (500 seeds, none left out; 436 cases with three real solutions, 64 with one): the reference's worst distance of its
    best E to the true E 1.914e-12 (median 6.6e-15), the header's 8.7e-13 (median 4.3e-15); the pose of the decomposition in front of
    both cameras: reference worst 2.8e-12, header 1.2e-12; the two find the same number of solutions in every case."""
    cases = [ref.minimal_case(seed) for seed in range(500)]
    norm = [(ref.normalise(c[0], K), ref.normalise(c[1], K)) for c in cases]
    full = [ref.seven_point(x0, x1, with_detail=True) for x0, x1 in norm]
    keep = [k for k in range(len(cases)) if not ref.near_double(full[k][1]) and full[k][2][6] >= 1e-6 * full[k][2][0]]
    assert len(keep) >= 0.98 * len(cases)
    got = core(["SOLVE " + _f(np.column_stack(norm[k])) for k in keep], tmp_path)

    def best_E(Es, Et):
        return min(np.abs(E - Et).max() for E in Es)

    def front_pose(Es, Et, x0, x1, R, t):
        E = min(Es, key=lambda E: np.abs(E - Et).max())
        front = [Rt for Rt in ref.decompose(E) if _in_front(*Rt, x0, x1)]
        assert len(front) == 1
        return ref.pose_dist(front[0], R, t)

    truth = [ref.essential(cases[k][2], cases[k][3]) for k in keep]
    ref_E = np.array([best_E(full[k][0], Et) for k, Et in zip(keep, truth)])
    ref_pose = np.array([front_pose(full[k][0], Et, *norm[k], cases[k][2], cases[k][3]) for k, Et in zip(keep, truth)])
    tol_E, tol_pose = max(100.0 * ref_E.max(), 1e-12), max(100.0 * ref_pose.max(), 1e-12)
    err_E, err_pose, nsol = [], [], []
    for j, k in enumerate(keep):
        g = got[j]
        Es = [np.array([float(v) for v in e]).reshape(3, 3) for e in g.get("E", [])]
        Ts = [np.array([float(v) for v in e]).reshape(3, 4) for e in g.get("T", [])]
        assert int(g["SOL"][0][0]) == len(Es) == len(full[k][0]), (k, len(Es), len(full[k][0]))
        assert len(Es) in (1, 3) and len(Ts) == 4 * len(Es)
        nsol.append(len(Es))
        firsts = [E[0, 0] for E in Es]
        assert all(a <= b for a, b in zip(firsts, firsts[1:])), k
        for E in Es:
            assert abs(np.linalg.norm(E) - 1.0) < 1e-14 and E.flat[np.argmax(np.abs(E))] > 0
        err_E.append(best_E(Es, truth[j]))
        b = int(np.argmin([np.abs(E - truth[j]).max() for E in Es]))
        poses = [(T[:, :3], T[:, 3]) for T in Ts[4 * b:4 * b + 4]]
        front = [Rt for Rt in poses if _in_front(*Rt, *norm[k])]
        assert len(front) == 1, k
        err_pose.append(ref.pose_dist(front[0], cases[k][2], cases[k][3]))
        # the canonical order: (R_a, +t), (R_a, -t), (R_b, +t), (R_b, -t)
        for i in range(len(Es)):
            (Ra, t0), (Ra2, t1), (Rb, t2), (Rb2, t3) = [(T[:, :3], T[:, 3]) for T in Ts[4 * i:4 * i + 4]]
            assert np.array_equal(Ra, Ra2) and np.array_equal(Rb, Rb2) and np.array_equal(t0, -t1) and np.array_equal(t0, t2) and np.array_equal(t1, t3)
            assert np.trace(Ra) >= np.trace(Rb) and t0[np.argmax(np.abs(t0))] > 0 and abs(np.linalg.norm(t0) - 1.0) < 1e-14
            assert abs(np.linalg.det(Ra) - 1.0) < 1e-9 and abs(np.linalg.det(Rb) - 1.0) < 1e-9
            # and they are the SVD's poses of the same E: both routes are backward stable, so they differ by rounding times the
            # ratio of E's two singular values, far below 1e-9 in the kept cases
            assert max(ref.pose_dist((T[:, :3], T[:, 3]), *w) for T, w in zip(Ts[4 * i:4 * i + 4], ref.decompose(Es[i]))) <= 1e-9, k
    print(f"kept {len(keep)} of {len(cases)}; solutions {np.bincount(nsol)}; distance of the best E to the truth: reference max "
          f"{ref_E.max():.3e} median {np.median(ref_E):.3e}, header max {max(err_E):.3e} median {np.median(err_E):.3e}; pose in front: "
          f"reference max {ref_pose.max():.3e}, header max {max(err_pose):.3e}")
    assert max(err_E) <= tol_E
    assert max(err_pose) <= tol_pose


def test_sampler_matches_restatement(core, tmp_path):
    rng = np.random.default_rng(7)
    tuples = [(int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 200)), int(rng.integers(0, 5000)),
               (7, 8, 9, 300)[k % 4]) for k in range(1000)]
    got = core([f"SAMPLE {seed} {st} {s} {n}" for seed, st, s, n in tuples], tmp_path)
    for k, (seed, st, s, n) in enumerate(tuples):
        idx = [int(v) for v in got[k]["IDX"][0]]
        assert idx == ref.sample_indices(seed, st, s, n), (seed, st, s, n)
        assert len(set(idx)) == 7 and all(0 <= i < n for i in idx)
        if n == 7:
            assert sorted(idx) == list(range(7))


def _ransac_cmd(pr, prob, thr, max_iters, seed, set_index, truncate=0, val=10.0, ratio=0.8):
    n = len(pr["px_first"])
    lines = [f"RANSAC {n} {prob!r} {thr!r} {max_iters} {seed} {set_index} {truncate} {val!r} {ratio!r} " + _f(pr["K"])]
    lines += [_f([*a, *b]) for a, b in zip(pr["px_first"], pr["px_last"])]
    return lines


def _parse_ransac(g):
    t = [int(v) for v in g["RES"][0]]
    bits = lambda key: np.array([int(ch) for ch in (g[key][0][0] if g[key][0] else "")], np.uint8)   # noqa: E731
    return dict(status=t[0], n_inliers=t[1], n_iters=t[2], pair_valid=t[3], best_sample=np.array(t[4:11]), mask=bits("MASK"),
                valid_mask=bits("VALID"), inlier_ratio=float(g["RATIO"][0][0]), T=np.array([float(v) for v in g["TBEST"][0]]).reshape(3, 4),
                points=np.array([float(v) for v in g["PTS"][0]]).reshape(-1, 3))


@pytest.mark.parametrize("prob,max_iters", [(0.99, 2000), (0.0, 100)])
@pytest.mark.parametrize("n,n_out", [(40, 12), (257, 77)])
def test_serial_loop_on_gap_data(core, tmp_path, n, n_out, prob, max_iters):
    """Noise-free inliers, outliers at least 40 px off the true epipolar line, 5 px / 10 px: mask and valid_mask are the labels, the
    ratio is the inlier share, and n_iters, n_inliers and best_sample are the reference loop's.  Measured: n_iters 54 (40, 12) and 53
    (257, 77) with prob 0.99, 100 with prob 0; the header's pose is within 9.3e-15 of the truth, the reference's within 3.6e-15 (the
    floor of 1e-12 decides)."""
    pr = ref.make_pair(2000 + n + n_out, n, n_out)
    seed = 91
    r = ref.ransac_serial(pr["px_first"], pr["px_last"], K, prob, 5.0, max_iters, seed, 3)
    g = _parse_ransac(core(_ransac_cmd(pr, prob, 5.0, max_iters, seed, 3), tmp_path)[0])
    assert r["status"] == ref.STATUS_OK and g["status"] == ref.STATUS_OK
    assert np.array_equal(r["mask"], pr["labels"]) and np.array_equal(r["valid_mask"], pr["labels"])
    assert np.array_equal(g["mask"], pr["labels"]) and np.array_equal(g["valid_mask"], pr["labels"])
    assert g["n_inliers"] == r["n_inliers"] == int(pr["labels"].sum())
    assert g["n_iters"] == r["n_iters"]
    if prob == 0.0:
        assert g["n_iters"] == 100
    assert np.array_equal(g["best_sample"], r["best_sample"])
    assert g["inlier_ratio"] == r["inlier_ratio"] == (n - n_out) / n
    assert g["pair_valid"] == r["pair_valid"] == (0 if (n - n_out) / n < 0.8 else 1)
    d_ref, d_got = ref.pose_dist((r["R"], r["t"]), pr["R"], pr["t"]), ref.pose_dist((g["T"][:, :3], g["T"][:, 3]), pr["R"], pr["t"])
    print(f"n_iters {g['n_iters']}; distance to the true pose: header {d_got:.3e}, reference {d_ref:.3e}")
    assert d_got <= max(100.0 * d_ref, 1e-12)
    inl = pr["labels"] == 1
    p_ref = np.abs(r["points"][inl] - pr["points"][inl]).max()
    assert np.abs(g["points"][inl] - pr["points"][inl]).max() <= max(100.0 * p_ref, 1e-12)


def test_serial_loop_too_few_and_no_model(core, tmp_path):
    pr = ref.make_pair(9, 7, 0)
    g = _parse_ransac(core(_ransac_cmd(pr, 0.99, 5.0, 1000, 1, 0), tmp_path)[0])
    assert g["status"] == ref.STATUS_TOO_FEW and g["n_iters"] == 0 and g["n_inliers"] == 0 and g["pair_valid"] == 0
    assert np.all(g["mask"] == 0) and np.all(g["valid_mask"] == 0) and np.all(np.isnan(g["T"])) and np.all(g["best_sample"] == -1)
    assert np.all(np.isnan(g["points"])) and np.isnan(g["inlier_ratio"])
    rp = ref.make_random_pair(5, 64)
    r = ref.ransac_serial(rp["px_first"], rp["px_last"], K, 0.0, 0.05, 20, 3, 0)
    g = _parse_ransac(core(_ransac_cmd(rp, 0.0, 0.05, 20, 3, 0), tmp_path)[0])
    assert r["status"] == g["status"] == ref.STATUS_NO_MODEL and g["n_iters"] == 20
    assert np.all(g["mask"] == 0) and np.all(np.isnan(g["T"])) and np.all(np.isnan(g["points"])) and g["pair_valid"] == 0
