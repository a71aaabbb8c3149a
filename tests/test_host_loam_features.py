"""bs_models::scan_registration::LoamFeatureExtractor (beam_slam_amd/host/loam_feature_extractor.h) — the stand-in for
feature_extractor->ExtractFeatures(cloud) and the batched ExtractAll — gives the same clouds three ways: through the shared header on one
core, through libbsgpu.so one scan per call, and through libbsgpu.so as one batch (tests/host/test_host_loam_features.cpp prints them;
the rows are compared as text, i.e. bit for bit).  The scans' beams sit in the middle of their rings, so the ring field and the elevation
rule give the same clouds.  Without a GPU: the header's batch against its lone calls, and a build without a back-end, in which a device
extractor extracts nothing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_loam_features.cpp")
CSRC = os.path.join(ROOT, "beam_slam_amd", "csrc")
# the shared header's bits need contraction off (loam_features.h, "Bits")
COMMON = ["-ffp-contract=off"]


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + COMMON + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST LOAM FEATURE EXTRACTOR DONE" in out.stdout
    rows = {}
    for ln in out.stdout.splitlines():
        tok = ln.split()
        if tok and tok[0] == "ROW":
            rows.setdefault(tok[1], {})[int(tok[2])] = tok[3:]
    return rows


def _check(rows, ways):
    for way in ways:
        assert sorted(rows[way]) == [0, 1, 2], way
        assert [rows[way][k][0] for k in range(3)] == ["1", "1", "1"] and rows[way][2][1:5] == ["0", "0", "0", "0"], way      # scan 2 is empty
        assert int(rows[way][0][1]) > 10 and int(rows[way][0][2]) > 100
        for k in range(3):
            assert rows[way][k] == rows[ways[0]][k], (way, k)


def test_extractor_through_the_header(tmp_path):
    rows = _run(_build(tmp_path, "test_host_loam_features_header", ["-DLOAM_NO_DEVICE"]))
    _check(rows, ["HEADER", "HEADER_LONE", "HEADER_RING"])


def test_extractor_without_backend_extracts_nothing_on_a_device(tmp_path):
    rows = _run(_build(tmp_path, "test_host_loam_features_none", ["-DLOAM_NO_BACKEND"]))
    _check(rows, ["HEADER", "HEADER_LONE"])
    assert all(r[:5] == ["0", "0", "0", "0", "0"] for r in rows["NONE"].values())


@pytest.mark.gpu
def test_extractor_three_ways_through_libbsgpu(tmp_path):
    rows = _run(_build(tmp_path, "test_host_loam_features_gpu", ["-L" + CSRC, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + CSRC,
                                                                  "-Wl,-rpath,/opt/rocm/lib"]))
    _check(rows, ["HEADER", "HEADER_LONE", "HEADER_RING", "DEVICE_LONE", "DEVICE", "DEVICE_RING"])
