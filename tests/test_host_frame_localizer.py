"""bs_models::FrameLocalizer (beam_slam_amd/host/frame_localizer.h) — LocalizeFrame's gate, fallback covariance, pose conversions and
covariance order — built against the oracle back-end (tests/host/test_host_loc.cpp's stand-in answers bsgpu_localize_frames with the
oracle's one-pose solve) and, on the GPU, against libbsgpu.so: both runs pass the same checks and agree on the refined frame."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_loc.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST FRAME LOCALIZER DONE" in out.stdout
    pose, cov = None, np.zeros(36)
    for line in out.stdout.splitlines():
        t = line.split()
        if t[0] == "POSE":
            pose = np.array([float(x) for x in t[1:]])
        elif t[0] == "COV":
            cov[int(t[1])] = float(t[2])
    return pose, cov.reshape(6, 6)


def _oracle_exe(tmp_path):
    from oracle import build
    build()
    odir = os.path.join(ROOT, "oracle")
    return _build(tmp_path, "test_host_loc_oracle", ["-include", os.path.join(ROOT, "tests", "host", "oracle_backend.h"), "-L" + odir,
                                                     "-lbs_oracle", "-Wl,-rpath," + odir])


def test_frame_localizer_against_oracle_backend(tmp_path):
    pose, cov = _run(_oracle_exe(tmp_path))
    assert np.allclose(cov, cov.T, rtol=1e-9, atol=0) and np.all(np.linalg.eigvalsh(cov) > 0)


@pytest.mark.gpu
def test_frame_localizer_through_libbsgpu(tmp_path):
    ref_pose, ref_cov = _run(_oracle_exe(tmp_path))
    cdir = os.path.join(ROOT, "beam_slam_amd", "csrc")
    pose, cov = _run(_build(tmp_path, "test_host_loc_gpu", ["-L" + cdir, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + cdir,
                                                            "-Wl,-rpath,/opt/rocm/lib"]))
    assert np.abs(pose - ref_pose).max() <= 1e-9
    assert np.abs(cov - ref_cov).max() <= 1e-8 * np.abs(np.diag(ref_cov)).max()
