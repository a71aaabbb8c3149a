"""The layout layer of beam_slam_amd/csrc/staging.h (what the front-end entry points of bsgpu_frontend.cpp pack their arrays with) as a
stand-alone host program, tests/plan/test_staging.cpp: 400 random segment lists from a fixed seed (sizes 0, 1, 7, 255, 256, 257 and
4 097 bytes, a quarter of the outputs not asked for) and the seven entry points' own layouts with one item, with three items of which
only the middle one holds anything, and with nothing in any item.  Per list: offsets on 256-byte boundaries, disjoint and in declaration
order; inputs, outputs and scratch contiguous in that order; every byte back through scatter() and through the accessor after a copy that
stands in for the device; guard bytes around every output array intact and an output not asked for skipped; a segment of no bytes never
dereferenced.  The program also walks check_start_table's verdicts and their order."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plan", "test_staging.cpp")
INC = os.path.join(ROOT, "beam_slam_amd", "csrc")


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]), ("sanitizers", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_layout(tmp_path, name, flags):
    exe = str(tmp_path / f"test_staging_{name}")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", INC, SRC, "-o", exe] + flags, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK ") and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[1]) == 400 + 6 * 8
