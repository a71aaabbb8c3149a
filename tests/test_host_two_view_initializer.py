"""bs_models::TwoViewInitializer (beam_slam_amd/host/two_view_initializer.h) — ComputePathWithVision's id intersection of the last
image with the first, its order, the pixel truncation, the reference's RANSACEstimator(..., SEVENPOINT, 100) defaults, the 10 px / 80 %
gate and "no value" below eight matches — built with a stand-in back-end (tests/host/test_host_two_view.cpp answers
bsgpu_relative_pose_ransac with seven_point.h's serial loop) and, on the GPU, against libbsgpu.so: both runs pass the same checks and
print the same ids, inlier sets, landmark sets, statuses and gate decisions."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_two_view.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST TWO VIEW INITIALIZER DONE" in out.stdout
    res = {}
    for line in out.stdout.splitlines():
        t = line.split()
        if t[0] in ("IDS", "INLIERS", "LANDMARKS", "GATE"):
            res[(t[0], t[1])] = [int(x) for x in t[2:]]
    return res


def _standin_exe(tmp_path):
    return _build(tmp_path, "test_host_two_view_standin", ["-DSP7_STANDIN", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc")])


def test_two_view_initializer_against_standin_backend(tmp_path):
    res = _run(_standin_exe(tmp_path))
    assert res[("GATE", "good")] == [0, 1, 1] and res[("GATE", "bad")] == [0, 0, 0]
    assert res[("GATE", "few")] == [1, 0, 0] and res[("GATE", "none")] == [1, 0, 0]
    ids, inl, lms = res[("IDS", "good")], res[("INLIERS", "good")], res[("LANDMARKS", "good")]
    assert ids == sorted(ids) and inl == sorted(inl) and set(inl) < set(ids) and set(lms) < set(ids) and len(lms) >= 0.8 * len(ids)
    assert res[("LANDMARKS", "bad")] == [] and len(res[("IDS", "few")]) == 7 and res[("IDS", "none")] == []


@pytest.mark.gpu
def test_two_view_initializer_through_libbsgpu(tmp_path):
    ref = _run(_standin_exe(tmp_path))
    cdir = os.path.join(ROOT, "beam_slam_amd", "csrc")
    got = _run(_build(tmp_path, "test_host_two_view_gpu", ["-L" + cdir, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + cdir,
                                                           "-Wl,-rpath,/opt/rocm/lib"]))
    assert got == ref
