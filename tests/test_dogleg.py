"""DOGLEG on the CPU: the numpy restatement (tests/dogleg_ref.py) on problems whose answer is known, and beam_slam_amd/csrc/dogleg.h — the
arithmetic the device solve uses — against the restatement (tests/plan/test_dogleg.cpp, compiled by g++)."""
import os
import subprocess

import numpy as np

import dogleg_ref
import helpers
from beam_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(J, r, lo=1e-6, hi=1e32):
    scale = 1.0 / (1.0 + np.linalg.norm(J, axis=0))
    return dogleg_ref.DoglegModel(J, r, scale, lo, hi, dogleg_ref.MIN_MU)


def test_linear_least_squares_in_one_gauss_newton_step():
    rng = np.random.default_rng(0)
    J = rng.normal(size=(40, 7))
    b = rng.normal(size=40)
    m = _model(J, -b)   # r(x) = J x - b at x = 0
    delta, _, case = m.step(1e12)
    assert case == 1 and m.factorizations == 1
    x_ls = np.linalg.lstsq(J, b, rcond=None)[0]
    assert np.abs(delta - x_ls).max() <= 1e-7 * np.abs(x_ls).max()   # (mu = 1e-8 regularises the solve)


def test_case_three_lands_on_the_boundary():
    rng = np.random.default_rng(1)
    hits = 0
    for _ in range(200):
        J = rng.normal(size=(30, 6)) * rng.uniform(0.1, 10.0, 6)
        m = _model(J, rng.normal(size=30))
        g_norm = np.linalg.norm(m.gradient)
        lo, hi = m.alpha * g_norm, np.linalg.norm(m.gn)
        if not lo < hi:
            continue
        radius = lo + rng.uniform(0.05, 0.95) * (hi - lo)
        delta, norm, case = m.step(radius)
        assert case == 3
        scaled = delta * m.diag / m.scale   # back to the trust region's coordinates: |D S^-1 delta|
        assert abs(np.linalg.norm(scaled) - radius) <= 1e-12 * radius
        assert abs(norm - radius) <= 1e-12 * radius
        hits += 1
    assert hits > 50


def _far_start():
    pr = helpers.mixed_problem(seed=1, n_state=5, n_lm=30, consistent=True)
    rng = np.random.default_rng(1)
    v = pr.values.copy()
    for b in range(pr.n_blocks):
        if pr.is_const[b]:
            continue
        o, n = pr.offset[b], pr.size[b]
        if pr.manifold[b] == capi.MANIFOLD_QUAT_RIGHT:
            v[o:o + 4] = helpers.quat_mul(v[o:o + 4], helpers.quat_from_aa(rng.normal(0, 0.3, 3)))
        else:
            v[o:o + n] += rng.normal(0, 0.3, n)
    pr.values = v
    return pr


def test_rejection_halves_the_radius_without_a_new_linearisation(oracle_cls):
    o = oracle_cls(threads=1)
    opt = o.options_default()
    opt.trust_region_strategy_type = capi.TR_DOGLEG
    opt.initial_trust_region_radius = 1e8
    ref = dogleg_ref.solve(_far_start(), o, opt)
    rec = ref["records"]
    rejected = [i for i in range(1, len(rec)) if rec[i]["valid"] and not rec[i]["successful"]]
    assert len(rejected) >= 5
    for i in rejected:
        assert rec[i]["radius"] == 0.5 * rec[i - 1]["radius"]
    # a rejected step's successor reuses the Gauss-Newton step: one linear system per new point only
    assert ref["reused"] == len([i for i in rejected if i + 1 < len(rec)])
    assert ref["factorizations"] == ref["steps"] - ref["reused"]
    assert rec[-1]["cost"] < 1e-3 * rec[0]["cost"]


def test_dogleg_header_matches_restatement(tmp_path):
    exe = str(tmp_path / "test_dogleg")
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                          os.path.join(ROOT, "tests", "plan", "test_dogleg.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    rng = np.random.default_rng(7)
    cases, vecs = [], []
    for k in range(3000):
        n = int(rng.integers(2, 12))
        g = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3)
        gn = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3)
        if k % 3 == 0:
            gn = -g * rng.uniform(0.5, 5.0) + 0.1 * gn   # (roughly downhill: case 3 most of the time)
        alpha = 10.0 ** rng.uniform(-2, 2)
        radius = 10.0 ** rng.uniform(-4, 4) * np.linalg.norm(gn)
        w = (float(g @ g), float(gn @ gn), float(g @ gn), float(g @ g) / alpha, radius)
        cases.append(w)
        vecs.append((g, gn, alpha, radius))
    path = tmp_path / "cases.txt"
    path.write_text("".join("%.17g %.17g %.17g %.17g %.17g\n" % w for w in cases))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == len(cases) + 4
    seen = set()
    for line, (g, gn, alpha, radius) in zip(lines, vecs):
        kase, a, b, norm, measured = line.split()
        s_ref, norm_ref, case_ref = dogleg_ref.traditional_step(g, gn, alpha, radius)
        assert int(kase) == case_ref
        seen.add(case_ref)
        # the header's step with D = S = I: a v + b gn, v = g
        s = float(a) * g + float(b) * gn
        assert np.linalg.norm(s - s_ref) <= 1e-14 * np.linalg.norm(s_ref) * 4, (kase, s, s_ref)
        if not int(measured):
            assert abs(float(norm) - norm_ref) <= 1e-14 * norm_ref
    assert seen == {1, 2, 3}
    tail = [list(map(float, t.split())) for t in lines[len(cases):]]
    assert tail[0] == [4.0, 1e-8]
    assert tail[1] == [6.0, 2.0 * 1e-3 / 10.0]
    assert tail[2] == [3.0, 2.0 * 1e-3 / 10.0 * 10.0]
    assert tail[3][0] == 0.0 and tail[3][1] == 0.1 * 10.0
