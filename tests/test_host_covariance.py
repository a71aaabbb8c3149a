"""GpuGraph::getCovariance (beam_slam_amd/host/gpu_graph.h) with landmark requests among pose requests: one
bsgpu_covariance_requests call through libbsgpu.so against the oracle-backed build of the same program
(tests/host/test_host_cov.cpp; the oracle answers pair by pair from its dense (J^T J)^-1)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_host_cov.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wno-unused-function", SRC, "-o", exe] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "HOST COVARIANCE DONE" in out.stdout
    cov = {}
    for line in out.stdout.splitlines():
        if line.startswith("COV "):
            _, i, j, v = line.split()
            cov.setdefault(int(i), {})[int(j)] = float(v)
    return [np.array([m[j] for j in range(9)]).reshape(3, 3) for _, m in sorted(cov.items())]


def _oracle_exe(tmp_path):
    from oracle import build
    build()
    odir = os.path.join(ROOT, "oracle")
    return _build(tmp_path, "test_host_cov_oracle", ["-include", os.path.join(ROOT, "tests", "host", "oracle_backend.h"), "-L" + odir,
                                                     "-lbs_oracle", "-Wl,-rpath," + odir])


def test_host_covariance_against_oracle_backend(tmp_path):
    """The per-pair fallback (a back-end without bsgpu_covariance_requests) answers every request, landmarks included."""
    cov = _run(_oracle_exe(tmp_path))
    assert len(cov) == 7
    for k in (0, 2, 6):   # (p2, p2), (l5, l5), (q3, q3): symmetric positive definite
        assert np.allclose(cov[k], cov[k].T, rtol=1e-9, atol=0)
        assert np.all(np.linalg.eigvalsh(cov[k]) > 0)


@pytest.mark.gpu
def test_host_covariance_through_libbsgpu(tmp_path):
    ref = _run(_oracle_exe(tmp_path))
    cdir = os.path.join(ROOT, "beam_slam_amd", "csrc")
    got = _run(_build(tmp_path, "test_host_cov_gpu", ["-L" + cdir, "-lbsgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + cdir,
                                                      "-Wl,-rpath,/opt/rocm/lib"]))
    assert len(got) == len(ref) == 7
    scale = max(np.abs(m).max() for m in ref)
    for g, o in zip(got, ref):
        assert np.abs(g - o).max() <= 1e-6 * scale, (g, o)
