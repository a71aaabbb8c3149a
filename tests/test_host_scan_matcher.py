"""bs_models::scan_registration::ScanMatcher (beam_slam_amd/host/scan_matcher.h) — PassedMotionThresholds with its three returns, the
batched call for the pairs that pass, T_LIDARREF_LIDARTGT = inv(T_RefEst_Ref) T_LidarRefEst_LidarTgt, RegistrationValidation's initial
and windowed branches on a hand-made metric list (its sums start at 0, where the reference reads them uninitialised) — built with a
stand-in back-end (tests/host/test_host_scan.cpp answers bsgpu_register_scans with icp.h on one core), with no back-end at all (nothing
is matched, nothing is computed on the host) and, on the GPU, against libbsgpu.so."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_scan.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST SCAN MATCHER DONE" in out.stdout
    rows = [ln.split() for ln in out.stdout.splitlines()]
    status = {int(r[1]): [int(v) for v in r[2:9]] for r in rows if r[0] == "STATUS"}
    mats = {(r[0], int(r[1])): np.vstack([np.array([float(v) for v in r[2:]]).reshape(3, 4), [0, 0, 0, 1]]) for r in rows if r[0].startswith("T")}
    return status, mats


def _check_matches(status, mats):
    # pair 1 is 20 m away: refused by the motion gate, never sent; pairs 0 and 2 are matched in one call
    assert status[1][:4] == [0, 0, 0, 0] and status[1][4] == -1
    for k in (0, 2):
        matched, passed, converged, validated, st, n_iters, n_corr = status[k]
        assert (matched, passed, converged, validated) == (1, 1, 1, 1) and st in (2, 3, 4) and n_iters >= 2 and n_corr >= 1400, status[k]
        composed = np.linalg.inv(mats[("TEST", k)]) @ mats[("TINIT", k)]
        assert np.abs(composed - mats[("TOUT", k)]).max() < 1e-13
        # the clouds are noise-free views of one point set: the true relative pose comes back
        assert np.abs(mats[("TOUT", k)] - mats[("TRUE", k)]).max() < 1e-9


def test_matcher_against_standin_backend(tmp_path):
    _check_matches(*_run(_build(tmp_path, "test_host_scan_standin", ["-DSCAN_STANDIN", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc")])))


def test_matcher_without_backend_matches_nothing(tmp_path):
    status, mats = _run(_build(tmp_path, "test_host_scan_none", ["-DSCAN_NO_BACKEND"]))
    assert all(s[0] == 0 and s[2] == 0 and s[4] == -1 for s in status.values()) and status[0][1] == 1 and not mats


@pytest.mark.gpu
def test_matcher_through_libbsgpu(tmp_path):
    cdir = os.path.join(ROOT, "beam_slam_amd", "csrc")
    _check_matches(*_run(_build(tmp_path, "test_host_scan_gpu", ["-L" + cdir, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + cdir,
                                                               "-Wl,-rpath,/opt/rocm/lib"])))
