"""Frame localisation's host/device core (beam_slam_amd/csrc/frame_lm.h) on the CPU against the oracle: tests/plan/test_frame_lm.cpp
solves seeded one-pose problems serially with flm_localize; the oracle solves the same BSGPU_F_REPROJ problem.  Same accept/reject
sequence and iteration count, final cost to 1e-10 relative, pose to 1e-9, covariance to 1e-8 of its diagonal scale; the
required_points_to_refine gate."""
import os
import subprocess

import numpy as np
import pytest

from beam_slam_amd import capi
from frame_cases import CASES, camera, compare, make_frame, options, oracle_localize, WIDTH, HEIGHT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opt_fields(o):
    return [o.max_num_iterations, o.jacobi_scaling, o.max_num_consecutive_invalid_steps, o.function_tolerance, o.gradient_tolerance,
            o.parameter_tolerance, o.initial_trust_region_radius, o.max_trust_region_radius, o.min_trust_region_radius,
            o.min_relative_decrease, o.min_lm_diagonal, o.max_lm_diagonal]


def _run_core(tmp_path, cases):
    """cases: list of (frame, loss_kind, loss_a, w, truncate, min_points, options) -> list of result dicts of the C++ core."""
    exe = str(tmp_path / "test_frame_lm")
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I",
                          os.path.join(ROOT, "beam_slam_amd", "csrc"), os.path.join(ROOT, "tests", "plan", "test_frame_lm.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    cam = camera()
    lines = []
    for fr, lk, la, w, trunc, min_pts, o in cases:
        n = len(fr["points"])
        lines.append(f"{n} {lk} {la!r} {w!r} {int(trunc)} {min_pts} {WIDTH} {HEIGHT}")
        lines.append(" ".join(repr(float(v)) for v in [cam.fx, cam.fy, cam.cx, cam.cy, *cam.R_cam_baselink, *cam.t_cam_baselink]))
        lines.append(" ".join(repr(float(v)) for v in [*fr["q_init"], *fr["p_init"]]))
        lines.append(" ".join(repr(v) if isinstance(v, float) else str(v) for v in _opt_fields(o)))
        for z, P in zip(fr["pixels"], fr["points"]):
            lines.append(" ".join(repr(float(v)) for v in [*z, *P]))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and f"DONE {len(cases)}" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    res, traces = {}, {}
    for line in run.stdout.splitlines():
        t = line.split()
        if t[0] == "CASE":
            v = np.array([float(x) for x in t[5:]])
            res[int(t[1])] = dict(status=int(t[2]), iterations=int(t[3]), cost=float(t[4]), avg=v[0], q=v[1:5], p=v[5:8],
                                  cov=v[8:44].reshape(6, 6))
        elif t[0] == "TRACE":
            traces[int(t[1])] = [int(x) for x in t[2:]]
    for i in res:
        res[i]["trace"] = traces[i]
    return [res[i] for i in range(len(cases))]


def test_core_matches_oracle(tmp_path, oracle_cls):
    cases, refs = [], []
    for seed, n, rot, tr, lk, la, okind, outl in CASES:
        fr = make_frame(seed, n, rot, tr, outlier_frac=outl)
        o = options(oracle_cls, okind)
        cases.append((fr, lk, la, 1.0, False, 20, o))
        refs.append(oracle_localize(oracle_cls, fr, lk, la, 1.0, o))
    got = _run_core(tmp_path, cases)
    for c, g, r in zip(CASES, got, refs):
        assert r["usable"] == 1
        assert g["status"] == 0, (c, g["status"])
        assert g["iterations"] >= 2, c
        compare(g, r, c)


def test_core_truncated_pixels_and_gate(tmp_path, oracle_cls):
    o = options(oracle_cls, "default")
    fr = make_frame(11, 150, 3.0, 0.2)
    small = make_frame(12, 19, 3.0, 0.2)
    got = _run_core(tmp_path, [(fr, capi.LOSS_HUBER, 1.5, 0.7, True, 20, o), (small, capi.LOSS_TRIVIAL, 1.0, 1.0, False, 20, o)])
    ref = oracle_localize(oracle_cls, fr, capi.LOSS_HUBER, 1.5, 0.7, o, truncate=True)
    compare(got[0], ref, "truncated")
    # required_points_to_refine: 19 < 20 -> nothing solved, the pose as given, no covariance
    g = got[1]
    assert g["status"] == 1 and g["iterations"] == 0
    assert np.array_equal(g["q"], small["q_init"]) and np.array_equal(g["p"], small["p_init"])
    assert np.all(np.isnan(g["cov"]))


@pytest.mark.parametrize("w", [0.0])
def test_core_zero_information_is_singular(tmp_path, oracle_cls, w):
    """sqrt_info = 0: J^T J is exactly zero, the gradient test ends the solve at once, no covariance (status 3)."""
    o = options(oracle_cls, "default")
    fr = make_frame(13, 40, 2.0, 0.1)
    g = _run_core(tmp_path, [(fr, capi.LOSS_TRIVIAL, 1.0, w, False, 20, o)])[0]
    assert g["status"] == 3 and g["iterations"] == 0 and g["cost"] == 0.0
    assert np.array_equal(g["q"], fr["q_init"]) and np.array_equal(g["p"], fr["p_init"])
    assert np.all(np.isnan(g["cov"]))
