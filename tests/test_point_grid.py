"""beam_slam_amd/csrc/point_grid.h, the grid and the fixed-order sums that icp.h and gicp.h share, on the CPU.

test_headers_keep_their_bits: tests/plan/test_icp.cpp and tests/plan/test_gicp.cpp, built from the working tree, print the bits that
tests/golden/scan_registration_bits.json records (written once, from the commit before point_grid.h existed, by
`python tests/test_point_grid.py --record`): every double as its 16 hex digits, every integer, the covariances as a SHA-256 of their
bytes.  The inputs are the registration commands of icp_ref.CASES and gicp_ref.CASES, the 257-point pair, a pair without a target,
and the first 13 grid_clouds() as nearest-neighbour and k-NN commands.

test_chunked_sums_follow_the_tree: grid_chunked_sums (through tests/plan/test_point_grid.cpp) against the tree written out below.
"""
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import gicp_ref
import icp_ref
import test_gicp
import test_icp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "beam_slam_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "scan_registration_bits.json")


def _hex(tokens):
    """the program's %.17g tokens (which round-trip) -> each double's 16 hex digits"""
    return [struct.pack(">d", float(t)).hex() for t in tokens]


def _inputs():
    """{name: (program, command)} in a fixed order"""
    out = {}
    S6, Q6 = icp_ref.scene(600)
    for name, (n, kw) in icp_ref.CASES.items():
        out["icp " + name] = ("icp", test_icp.reg_command(*icp_ref.scene(n), **kw))
    out["icp n257"] = ("icp", test_icp.reg_command(S6[:257], Q6))
    out["icp no target"] = ("icp", test_icp.reg_command(S6, Q6[:0]))
    for name, (n, kw) in gicp_ref.CASES.items():
        out["gicp " + name] = ("gicp", test_gicp.reg_command(*icp_ref.scene(n), want_cov=True, **kw))
    out["gicp n257"] = ("gicp", test_gicp.reg_command(S6[:257], Q6, want_cov=True))
    out["gicp no target"] = ("gicp", test_gicp.reg_command(S6, Q6[:0], want_cov=True))
    for i, (S, Q, h) in enumerate(test_icp.grid_clouds()[:13]):
        out[f"icp nn {i}"] = ("icp", test_icp.nn_command(S, Q, h))
        out[f"gicp nn {i}"] = ("gicp", test_gicp.nn_command(S, Q, 0.37 if i % 2 else h, h))
        out[f"gicp knn {i}"] = ("gicp", test_gicp.knn_command(Q, 1 if i % 2 else 8, 0.37 if i % 4 > 1 else h))   # (two fixtures share a Q)
    return out


def _record(tok):
    """One output line -> what is compared."""
    if tok[0] != "REG":
        return " ".join(tok[2:])
    n_int = 4 if len(tok) == 6 + 25 else 5          # icp: ok status n_iters n_corr; gicp: n_inner too
    doubles = tok[2 + n_int:]
    rec = dict(ints=[int(t) for t in tok[2:2 + n_int]], doubles=_hex(doubles[:25]))
    if len(doubles) > 25:
        rec["cov_sha256"] = hashlib.sha256(np.array([float(t) for t in doubles[25:]]).tobytes()).hexdigest()
    return rec


def collect(exes, tmp_path):
    inputs = _inputs()
    got = {}
    for prog in ("icp", "gicp"):
        names = [k for k, (p, _) in inputs.items() if p == prog]
        rows = test_icp.run_program(exes[prog], [inputs[k][1] for k in names], tmp_path)
        got.update({k: _record(tok) for k, tok in zip(names, rows)})
    return got


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return dict(icp=test_icp._compile(tmp_path_factory, ["-O2"], "test_icp"), gicp=test_gicp._compile(tmp_path_factory, ["-O2"], "test_gicp"))


def test_headers_keep_their_bits(exes, tmp_path):
    want = json.load(open(GOLDEN))
    got = collect(exes, tmp_path)
    assert list(got) == list(want)
    for k in want:
        assert got[k] == want[k], k
    assert want["icp no target"]["ints"] == [1, icp_ref.TOO_FEW, 0, 0] and want["gicp no target"]["ints"] == [1, gicp_ref.TOO_FEW, 0, 0, 0]


# ---- the summation template ---------------------------------------------------------------------------------------------------------------
CHUNK, WAVE = 128, 64


def _terms(n, rec):
    """Exact in double, and wide enough in exponent that a sum in another order rounds differently: small integers times powers of
    two, another pattern in every lane."""
    i, t = np.arange(n)[:, None], np.arange(rec)[None, :]
    return ((((7 * i + 3 * t) % 31) - 15) * 2.0 ** ((11 * (i % WAVE) + 5 * t + i // WAVE) % 80 - 40)).astype(np.float64)


def _tree(terms):
    """The order of point_grid.h: chunks of 128 points; in a chunk each wave's 64 values by the shuffle-down tree (offsets 32 .. 1),
    the waves in order onto 0; the chunks in order onto 0."""
    n, rec = terms.shape
    total = np.zeros(rec)
    for c in range(0, n, CHUNK):
        lanes = np.zeros((CHUNK, rec))
        lanes[:min(CHUNK, n - c)] = terms[c:c + CHUNK]
        part = np.zeros(rec)
        for w in range(0, CHUNK, WAVE):
            v = lanes[w:w + WAVE].copy()
            off = WAVE // 2
            while off >= 1:
                v[:off] = v[:off] + v[off:2 * off]
                off //= 2
            part = part + v[0]
        total = total + part
    return total


def test_chunked_sums_follow_the_tree(tmp_path_factory, tmp_path):
    exe = str(tmp_path_factory.mktemp("point_grid") / "test_point_grid")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-O2", "-ffp-contract=off", "-I", INC, os.path.join(ROOT, "tests", "plan", "test_point_grid.cpp"),
                          "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    shapes = [(n, rec) for rec in (17, 28) for n in (1, 63, 64, 65, 128, 129, 257)]
    cmds = [np.concatenate([[n, rec], _terms(n, rec).ravel()]) for n, rec in shapes]
    rows = test_icp.run_program(exe, cmds, tmp_path)
    differs = 0
    for (n, rec), tok in zip(shapes, rows):
        terms = _terms(n, rec)
        assert _hex(tok[2:]) == _hex([repr(float(v)) for v in _tree(terms)]), (n, rec)
        differs += int((terms.sum(axis=0) != _tree(terms)).any() or (np.add.reduce(terms[::-1], axis=0) != _tree(terms)).any())
    assert differs >= 8          # the terms do tell the tree from other orders


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    import pathlib
    import tempfile

    class _Factory:
        def mktemp(self, name):
            return pathlib.Path(tempfile.mkdtemp(prefix=name))

    f = _Factory()
    exes_ = dict(icp=test_icp._compile(f, ["-O2"], "test_icp"), gicp=test_gicp._compile(f, ["-O2"], "test_gicp"))
    with open(GOLDEN, "w") as fh:
        json.dump(collect(exes_, f.mktemp("run")), fh, indent=0)
        fh.write("\n")
