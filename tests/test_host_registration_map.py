"""bs_models::scan_registration::RegistrationMap (beam_slam_amd/host/registration_map.h) — the stand-in for the reference's scan store
and its GetLoamCloudMap / GetPointCloudMap — gives the same maps through the shared header on one core and through libbsgpu.so
(tests/host/test_host_registration_map.cpp prints them; the rows are compared as text, i.e. bit for bit).  Both ways: trimming at
map_size by stamp, UpdateScan below and above ArePosesEqual's two thresholds, GetLoamCloudMap as ONE call with two maps that equals
registration_map_serial on the two classes, the whole-cloud map with the voxel filter and merged only.  Without a GPU: the header
alone, and a build without a back-end, in which a device map builds nothing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_registration_map.cpp")
CSRC = os.path.join(ROOT, "beam_slam_amd", "csrc")
# the shared header's bits need contraction off (point_grid.h, "Bits")
COMMON = ["-ffp-contract=off"]
TAGS = ["trim", "update", "loam", "before", "cloud", "merged", "shrunk"]


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + COMMON + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST REGISTRATION MAP DONE" in out.stdout
    rows = {}
    for ln in out.stdout.splitlines():
        tok = ln.split()
        if tok and tok[0] == "ROW":
            rows.setdefault(tok[1], {})[tok[2]] = tok[3:]
    return rows


def _check(rows, ways):
    for way in ways:
        r = rows[way]
        assert sorted(r) == sorted(TAGS), way
        assert r["trim"] == ["4", "0", "0", "1", "1", "1", "1"], way             # stamps 100 and 200, the oldest, are gone
        assert r["update"] == ["0", "0", "1", "1"], way
        assert r["loam"][0] == "1" and 100 < int(r["loam"][1]) < 4 * 200 and 100 < int(r["loam"][2]) < 4 * 400, way
        assert len(r["loam"]) == 3 + 3 * (int(r["loam"][1]) + int(r["loam"][2])), way
        assert int(r["before"][0]) > 100 and r["cloud"][0] == "1" and r["merged"][:2] == ["1", str(1500 + 2000 + 1900 + 1800)], way
        assert int(r["cloud"][1]) < int(r["merged"][1]) and r["shrunk"] == ["2", "1", "1"], way
        for tag in TAGS:
            assert r[tag] == rows[ways[0]][tag], (way, tag)


def test_map_through_the_header(tmp_path):
    rows = _run(_build(tmp_path, "test_host_registration_map_header", ["-DMAP_NO_DEVICE"]))
    _check(rows, ["HEADER"])


def test_map_without_backend_builds_nothing_on_a_device(tmp_path):
    rows = _run(_build(tmp_path, "test_host_registration_map_none", ["-DMAP_NO_BACKEND"]))
    _check(rows, ["HEADER"])
    assert rows["NONE"]["loam"] == ["0", "0", "0"]


@pytest.mark.gpu
def test_map_through_libbsgpu_equals_the_header(tmp_path):
    rows = _run(_build(tmp_path, "test_host_registration_map_gpu", ["-L" + CSRC, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + CSRC,
                                                                     "-Wl,-rpath,/opt/rocm/lib"]))
    _check(rows, ["HEADER", "DEVICE"])
