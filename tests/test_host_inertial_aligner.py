"""bs_models::InertialAligner (beam_slam_amd/host/inertial_aligner.h) — the reference's map-keyed path in stamp order, nanosecond stamps,
the quaternion of the rotation block, the reference's defaults, the aligned path and velocities map — built with a stand-in back-end
(tests/host/test_host_align.cpp answers bsgpu_inertial_alignment with inertial_align.h on one lane), with no back-end at all (nothing
is initialised, nothing is computed on the host) and, on the GPU, against libbsgpu.so.  In each build the class hands back exactly what
the same C-ABI call wrote."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_align.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST INERTIAL ALIGNER DONE" in out.stdout
    return [ln.split() for ln in out.stdout.splitlines() if ln.startswith("STATUS")]


def test_aligner_against_standin_backend(tmp_path):
    res = _run(_build(tmp_path, "test_host_align_standin", ["-DALIGN_STANDIN", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc")]))
    assert res[0][1:3] == ["0", "1"] and abs(float(res[0][4]) - 0.37) < 0.02 * 0.37


def test_aligner_without_backend_is_not_initialised(tmp_path):
    assert _run(_build(tmp_path, "test_host_align_none", ["-DALIGN_NO_BACKEND"])) == []


@pytest.mark.gpu
def test_aligner_through_libbsgpu(tmp_path):
    cdir = os.path.join(ROOT, "beam_slam_amd", "csrc")
    res = _run(_build(tmp_path, "test_host_align_gpu", ["-L" + cdir, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + cdir,
                                                        "-Wl,-rpath,/opt/rocm/lib"]))
    assert res[0][1:3] == ["0", "1"] and abs(float(res[0][4]) - 0.37) < 0.02 * 0.37
