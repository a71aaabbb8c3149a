"""bs_models::scan_registration::LoamMatcher (beam_slam_amd/host/loam_matcher.h) — the stand-in for the matcher's interface (SetRef,
SetTarget, Match, GetResult, ApplyResult, GetCovariance) and the batched MatchAll of a scan against its neighbours — gives the same
matches three ways: through the shared header on one core, through libbsgpu.so one pair per call, and through libbsgpu.so as one batch
(tests/host/test_host_loam.cpp prints them; the rows are compared as text, i.e. bit for bit).  Without a GPU: the header's batch against
its lone calls, and a build without any back-end, in which nothing matches."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_loam.cpp")
CSRC = os.path.join(ROOT, "beam_slam_amd", "csrc")
# the shared header reaches bsgpu_internal.h, whose declarations name HIP types; its bits need contraction off (loam.h, "Bits")
HEADER = ["-DLOAM_MATCHER_WITH_HEADER", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC]


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST LOAM MATCHER DONE" in out.stdout
    rows = {}
    for ln in out.stdout.splitlines():
        tok = ln.split()
        if tok and tok[0] == "ROW":
            rows.setdefault(tok[1], {})[int(tok[2])] = tok[3:]
    return rows


def _check(rows, ways):
    for way in ways:
        assert sorted(rows[way]) == [0, 1, 2], way
        assert [rows[way][k][0] for k in range(3)] == ["1", "1", "0"] and rows[way][2][1] == "5", (way, rows[way][2][:2])      # pair 2 has no reference
        for k in range(3):
            assert rows[way][k] == rows[ways[0]][k], (way, k)


def test_matcher_through_the_header(tmp_path):
    rows = _run(_build(tmp_path, "test_host_loam_header", HEADER + ["-DLOAM_NO_DEVICE"]))
    _check(rows, ["HEADER", "HEADER_LONE"])


def test_matcher_without_backend_matches_nothing(tmp_path):
    rows = _run(_build(tmp_path, "test_host_loam_none", ["-DLOAM_NO_BACKEND"]))
    assert all(r[0] == "0" and r[1] == "-1" for way in ("NONE", "OFF") for r in rows[way].values())


@pytest.mark.gpu
def test_matcher_three_ways_through_libbsgpu(tmp_path):
    rows = _run(_build(tmp_path, "test_host_loam_gpu", HEADER + ["-L" + CSRC, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + CSRC,
                                                                 "-Wl,-rpath,/opt/rocm/lib"]))
    _check(rows, ["HEADER", "HEADER_LONE", "DEVICE_LONE", "DEVICE"])
