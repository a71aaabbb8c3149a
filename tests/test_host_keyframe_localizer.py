"""bs_models::KeyframeRansacLocalizer (beam_slam_amd/host/keyframe_ransac_localizer.h) — ComputePathWithVision's per-keyframe id
intersection, its order, the pixel truncation, the reference's RANSACEstimator(..., 100) defaults and "no pose" below four pairs —
built with a stand-in back-end (tests/host/test_host_p3p.cpp answers bsgpu_absolute_pose_ransac with p3p.h's serial loop) and, on the
GPU, against libbsgpu.so: both runs pass the same checks and print the same ids, inlier sets and statuses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_p3p.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST KEYFRAME LOCALIZER DONE" in out.stdout
    res = {}
    for line in out.stdout.splitlines():
        t = line.split()
        if t[0] in ("IDS", "INLIERS"):
            res[(t[0], int(t[1]))] = [int(x) for x in t[2:]]
        elif t[0] == "STATUS":
            res["STATUS"] = [int(x) for x in t[1:]]
    return res


def _standin_exe(tmp_path):
    return _build(tmp_path, "test_host_p3p_standin", ["-DP3P_STANDIN", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc")])


def test_keyframe_localizer_against_standin_backend(tmp_path):
    res = _run(_standin_exe(tmp_path))
    assert res["STATUS"] == [0, 0, 1, 1]
    for k in (0, 1):
        ids, inl = res[("IDS", k)], res[("INLIERS", k)]
        assert ids == sorted(ids) and inl == sorted(inl) and set(inl) < set(ids) and len(inl) >= 40


@pytest.mark.gpu
def test_keyframe_localizer_through_libbsgpu(tmp_path):
    ref = _run(_standin_exe(tmp_path))
    cdir = os.path.join(ROOT, "beam_slam_amd", "csrc")
    got = _run(_build(tmp_path, "test_host_p3p_gpu", ["-L" + cdir, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + cdir,
                                                      "-Wl,-rpath,/opt/rocm/lib"]))
    assert got == ref
