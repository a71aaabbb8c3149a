"""bs_models::reloc::LoopClosureAligner (beam_slam_amd/host/loop_closure_aligner.h) — T_Candidate_Query_Init formed as the reference
forms it and passed as T_init, one bsgpu_register_scans_gicp call for all ranked pairs, the first pair in rank order whose status is
converged, T_CandidateSubmap_QuerySubmap = T_SubmapCandidate_Lidar T_Candidate_Query inv(T_SubmapQuery_Lidar) — built with a stand-in
back-end (tests/host/test_host_loop_closure.cpp answers the call with gicp.h on one core), with no back-end at all (nothing is aligned,
nothing is computed on the host) and, on the GPU, against libbsgpu.so."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_loop_closure.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST LOOP CLOSURE DONE" in out.stdout
    rows = [ln.split() for ln in out.stdout.splitlines()]
    taken = [[int(v) for v in r[1:3]] for r in rows if r[0] == "TAKEN"][0]
    status = {int(r[1]): [int(v) for v in r[2:6]] + [float(r[6])] for r in rows if r[0] == "STATUS"}
    mats = {(r[0], int(r[1])): np.vstack([np.array([float(v) for v in r[2:]]).reshape(3, 4), [0, 0, 0, 1]]) for r in rows if r[0].startswith("T") and r[0] != "TAKEN"}
    return taken, status, mats


def _check_alignment(taken, status, mats):
    # rank 0 has a query cloud of 5 points (fewer than k): the matcher fails and the next pair is tried; rank 1 is the answer
    assert taken == [1, 8]
    assert status[0][0] == 5 and status[0][1] == 0
    for k in (1, 2):
        st, n_iters, n_inner, n_corr, cost = status[k]
        assert st in (1, 2) and n_iters >= 2 and n_inner >= n_iters and n_corr == 1500 and cost < 1e-20, status[k]
    assert np.abs(mats[("TINIT", 1)] - mats[("TINITWANT", 1)]).max() < 1e-15
    # the clouds are noise-free views of one point set: the true transform between the submaps comes back
    assert np.abs(mats[("TOUT", 1)] - mats[("TRUE", 1)]).max() < 1e-9
    assert np.abs(mats[("TCQ", 1)] - mats[("TINIT", 1)]).max() > 1e-2      # (the initial guess was off: the match did the work)


def test_aligner_against_standin_backend(tmp_path):
    _check_alignment(*_run(_build(tmp_path, "test_host_loop_closure_standin", ["-DLC_STANDIN", "-ffp-contract=off", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc")])))


def test_aligner_without_backend_aligns_nothing(tmp_path):
    taken, status, mats = _run(_build(tmp_path, "test_host_loop_closure_none", ["-DLC_NO_BACKEND"]))
    assert taken == [-1, -1] and all(s[0] == -1 for s in status.values()) and not any(k[0] in ("TOUT", "TCQ") for k in mats)


@pytest.mark.gpu
def test_aligner_through_libbsgpu(tmp_path):
    cdir = os.path.join(ROOT, "beam_slam_amd", "csrc")
    _check_alignment(*_run(_build(tmp_path, "test_host_loop_closure_gpu", ["-L" + cdir, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + cdir,
                                                                          "-Wl,-rpath,/opt/rocm/lib"])))
