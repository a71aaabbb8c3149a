"""Online calibration through the host mirror (beam_slam_amd/host/): bs_variables::Orientation3D / Position3D released with
setHoldConstant(false), the calibration prior of VisualMap::AddCameraCalibration (bs_constraints::AbsolutePose3DConstraint), and
EuclideanReprojectionConstraintOnlineCalib factors in a GpuGraph (tests/host/test_host_calib.cpp) — against the oracle back-end on the CPU
and through libbsgpu.so on the GPU: the optimised extrinsic is read back from the graph and has moved towards the truth; with the
default holdConstant() == true it does not move."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_calib.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + extra,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe, mode):
    out = subprocess.run([exe, mode], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "HOST CALIB DONE" in out.stdout, out.stdout[-4000:] + out.stderr[-2000:]
    rec = {}
    for line in out.stdout.splitlines():
        t = line.split()
        if t and t[0] in ("TRUE", "X0", "X", "cost", "OBS"):
            rec[t[0]] = np.array([float(v) for v in t[1:]])
    return rec


def _oracle_exe(tmp_path):
    from oracle import build
    build()
    odir = os.path.join(ROOT, "oracle")
    return _build(tmp_path, "test_host_calib_oracle", ["-include", os.path.join(ROOT, "tests", "host", "oracle_backend.h"), "-L" + odir,
                                                       "-lbs_oracle", "-Wl,-rpath," + odir])


def _gpu_exe(tmp_path):
    cdir = os.path.join(ROOT, "beam_slam_amd", "csrc")
    return _build(tmp_path, "test_host_calib_gpu", ["-L" + cdir, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + cdir,
                                                    "-Wl,-rpath,/opt/rocm/lib"])


def _check_released(rec):
    assert rec["OBS"][0] >= 60
    assert rec["cost"][1] < rec["cost"][0]
    e0, e1 = np.abs(rec["X0"] - rec["TRUE"]), np.abs(rec["X"] - rec["TRUE"])
    assert np.linalg.norm(rec["X"][4:] - rec["X0"][4:]) > 1e-3          # p_BASELINK_CAM moved by more than a millimetre ...
    assert np.linalg.norm(e1[4:]) < np.linalg.norm(e0[4:])              # ... towards the truth,
    assert np.linalg.norm(e1[:4]) < np.linalg.norm(e0[:4])              # and so did q_BASELINK_CAM
    assert abs(np.linalg.norm(rec["X"][:4]) - 1.0) < 1e-9


def test_released_pair_moves_and_held_pair_stays_oracle_backend(tmp_path):
    exe = _oracle_exe(tmp_path)
    _check_released(_run(exe, "free"))
    held = _run(exe, "held")
    assert np.array_equal(held["X"], held["X0"])


@pytest.mark.gpu
def test_released_pair_through_libbsgpu(tmp_path):
    ref = _run(_oracle_exe(tmp_path), "free")
    exe = _gpu_exe(tmp_path)
    rec = _run(exe, "free")
    _check_released(rec)
    # the same graph in the oracle back-end: same optimum (final cost as tests/test_host_unicycle.py compares it, values to 1e-6)
    assert abs(rec["cost"][1] - ref["cost"][1]) <= 1e-6 * ref["cost"][1]
    assert np.abs(rec["X"] - ref["X"]).max() <= 1e-6
    held = _run(exe, "held")
    assert np.array_equal(held["X"], held["X0"])
