"""bs_models::TrackOutlierFilter (beam_slam_amd/host/track_outlier_filter.h) — AddMeasurementsToContainer's id intersection, its
order, the pixel truncation and "erase nothing" below five matches — built with a stand-in back-end (tests/host/test_host_ransac.cpp
answers bsgpu_essential_ransac with five_point.h's serial loop) and, on the GPU, against libbsgpu.so: both runs pass the same checks
and erase the same ids."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_ransac.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST TRACK FILTER DONE" in out.stdout
    erase = stats = None
    for line in out.stdout.splitlines():
        t = line.split()
        if t[0] == "ERASE":
            erase = [int(x) for x in t[1:]]
        elif t[0] == "STATS":
            stats = [int(x) for x in t[1:]]
    return erase, stats


def _standin_exe(tmp_path):
    return _build(tmp_path, "test_host_ransac_standin", ["-DRANSAC_STANDIN", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc")])


def test_track_filter_against_standin_backend(tmp_path):
    erase, stats = _run(_standin_exe(tmp_path))
    assert len(erase) >= 16 and erase == sorted(erase)


@pytest.mark.gpu
def test_track_filter_through_libbsgpu(tmp_path):
    ref_erase, ref_stats = _run(_standin_exe(tmp_path))
    cdir = os.path.join(ROOT, "beam_slam_amd", "csrc")
    erase, stats = _run(_build(tmp_path, "test_host_ransac_gpu", ["-L" + cdir, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + cdir,
                                                                  "-Wl,-rpath,/opt/rocm/lib"]))
    assert erase == ref_erase
    assert stats == ref_stats
