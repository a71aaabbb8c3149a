"""The host mirror's DOGLEG options (beam_slam_amd/host/gpu_graph.h): tests/host/test_host_dogleg.cpp against the CPU oracle, with the
back-end's solve wrapped so that the options it receives are recorded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpu_graph_hands_the_strategy_to_the_backend(tmp_path):
    from oracle import build
    build()
    odir = os.path.join(ROOT, "oracle")
    exe = str(tmp_path / "test_host_dogleg")
    cmd = ["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "tests", "host"),
           os.path.join(ROOT, "tests", "host", "test_host_dogleg.cpp"), "-o", exe, "-L" + odir, "-lbs_oracle", "-Wl,-rpath," + odir]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "ALL HOST DOGLEG TESTS PASSED" in run.stdout, run.stdout[-4000:] + run.stderr[-2000:]
