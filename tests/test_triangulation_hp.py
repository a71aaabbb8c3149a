"""Landmark triangulation against a 50-digit reference (tests/triangulation_hp.py: mp.svd_r of the DLT matrix A), on the CPU through
beam_slam_amd/csrc/triangulate_core.h (tests/plan/test_triangulate.cpp) and on the device through bsgpu_triangulate.

Tracks: 2 / 3 / 12 / 40 views, baseline / depth 0.5 / 6, 0.05 / 30 and 0.01 / 30 m, the whole scene 0, 1e2, 1e3, 1e4 and 1e5 m from the world
origin along a generic direction, 8 points per cell, exact projections and the same pixels truncated to integers; per offset 9
deliberate rejections (behind a camera, too far, re-projection bound); one call per offset and truncation, 257 tracks with an empty
and a single-view track in front.  Statuses must be the 50-digit decisions, none of which lies within a relative 1e-6 of its
threshold.

Tolerance, per cell (offset x parallax x views): with e_ref the largest coordinate error of oracle/triangulation.py (float64 LAPACK
SVD of A) against the 50-digit point over the cell's tracks, the largest error of the core / the kernel must be at most
max(16 e_ref, 1e-14 |P|_inf) — 16 for the other operation order in T and A and a Jacobi instead of LAPACK's SVD, both backward stable.

Measured, exact and truncated pixels together.  Largest coordinate error in metres over the cells of an offset, and in brackets
the largest error / max(e_ref, 1e-14 |P|_inf / 16) over its cells, which the bound keeps at 16 or less:
    offset   e_ref     parent commit's Gram body (CPU)   core (CPU)       kernel (MI355X)
    0        6.4e-08   1.1e-07  (13.4)                   1.6e-08 (0.97)   1.3e-08 (1.13)
    1e2      1.3e-09   2.9e-06  (31 388)                 8.5e-11 (1.01)   7.2e-11 (0.70)
    1e3      1.5e-07   3.2e-05  (65 311)                 8.3e-10 (0.48)   8.6e-10 (0.62)
    1e4      1.4e-05   2.5e-04  (15 276)                 9.2e-09 (0.17)   1.2e-08 (0.17)
    1e5      2.0e-03   4.6e-03  (1 757)                  9.2e-08 (0.06)   9.5e-08 (0.07)
The parent commit's body (smallest eigenvector of A^T A by cyclic Jacobi), run through the same driver, fails every call but the two
at offset 0: at 1e2 m already in the 0.5 m / 6 m cell of 40 views (3.2e-11 against e_ref 1.2e-12), by offset x parallax
(0.5/6, 0.05/30, 0.01/30) 5.6e-11 4.0e-07 2.9e-06 at 1e2, 6.1e-10 1.2e-06 3.2e-05 at 1e3, 4.6e-09 9.1e-05 2.5e-04 at 1e4 and
4.5e-08 6.5e-05 4.6e-03 at 1e5.  (LAPACK's own error grows with the offset because it scales no columns; one-sided Jacobi does not.)
"""
import os
import subprocess

import numpy as np
import pytest

import triangulation_hp as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = [(oi, tr) for oi in range(len(hp.OFFSETS)) for tr in (0, 1)]


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(ROOT, "tests", "golden", "triangulation_hp.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("triangulate") / "test_triangulate")
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                          os.path.join(ROOT, "tests", "plan", "test_triangulate.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]

    def run(fx, oi, truncate, tmp_path):
        start, obs, _ = hp.call_layout(fx, oi)
        f = lambda v: " ".join(repr(float(x)) for x in np.ravel(v))
        lines = [f"TRACKS {len(start) - 1} {len(obs)} {fx['values'].size} {truncate} {hp.MAX_DIST!r} {hp.MAX_REPROJ!r}", f(fx["camera"]),
                 f(fx["values"]), " ".join(str(int(s)) for s in start)]
        lines += [f"{int(fx['q_off'][o])} {int(fx['p_off'][o])} " + f(fx["pixels"][o]) for o in obs]
        path = tmp_path / "commands.txt"
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "DONE 1" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("PT ")]
        assert [int(t[2]) for t in rows] == list(range(len(start) - 1))
        return np.array([[float(v) for v in t[4:7]] for t in rows]), np.array([int(t[3]) for t in rows], np.int32)
    return run


def _check(fx, oi, tr, pts, st, who):
    """Statuses and the per-cell bound for the N_CALL tracks of one call; returns (e_ref, error, ratio) maxima over the cells."""
    _, _, src = hp.call_layout(fx, oi)
    assert len(src) == hp.N_CALL == len(st)
    assert (st[:2] == 1).all() and (pts[:2] == 0).all()
    s = src[2:]
    assert np.array_equal(st[2:], fx["hp_status"][tr][s])
    assert (fx["hp_status"][tr][s] != 5).all()
    err = hp.error(pts[2:], fx["hp_hi"][tr][s], fx["hp_lo"][tr][s])
    cells = fx["cell"][s]
    worst = (0.0, 0.0, 0.0)
    for c in np.unique(cells[cells >= 0]):
        m = cells == c
        assert m.sum() >= hp.SEEDS
        e_ref = fx["e_ref"][tr][s[m]].max()
        floor = 1e-14 * np.abs(fx["hp_hi"][tr][s[m]]).max()
        e = err[m].max()
        worst = (max(worst[0], e_ref), max(worst[1], e), max(worst[2], e / max(e_ref, floor / 16.0)))
        assert e <= max(16.0 * e_ref, floor), (who, hp.OFFSETS[oi], tr, int(c), e, e_ref, floor)
    print(f"{who}: offset {hp.OFFSETS[oi]:g} truncate {tr}: e_ref {worst[0]:.3e} error {worst[1]:.3e} largest error / e_ref {worst[2]:.2f}")
    return worst


def test_every_decision_has_margin(fx):
    """No case left out: every track of the fixture, exact and truncated pixels, decides each of its statuses at least a relative
    1e-6 from the threshold; the deliberate rejections are the statuses they were built for, with either kind of pixels, and every
    offset's call holds all three; the yardstick (float64) decides like the 50-digit reference."""
    assert fx["hp_margin"].min() >= hp.MARGIN, fx["hp_margin"].min()
    kind = fx["kind"]
    for tr in (0, 1):
        assert np.array_equal(fx["hp_status"][tr][kind > 0], kind[kind > 0])
        assert np.array_equal(fx["hp_status"][tr], fx["ref_status"][tr])
    assert (fx["hp_status"][0][kind == 0] == 0).all()           # exact projections of the grid: all triangulated
    for oi in range(len(hp.OFFSETS)):
        assert sorted(kind[(fx["offset_id"] == oi) & (kind > 0)]) == [2, 2, 2, 3, 3, 3, 4, 4, 4]
    n_cells = len(hp.OFFSETS) * len(hp.PARALLAX) * len(hp.VIEWS)
    assert np.array_equal(np.bincount(fx["cell"][kind == 0], minlength=n_cells), np.full(n_cells, hp.SEEDS))


def test_fixture_matches_its_generator(fx):
    """The inputs and every 50-digit entry of tests/golden/triangulation_hp.npz, regenerated: the same bits.  The yardstick goes
    through LAPACK, whose last bits belong to the library build: it must reproduce within the bound it sets."""
    pytest.importorskip("mpmath")
    inp = hp.build_inputs()
    for k, v in inp.items():
        assert v.dtype == fx[k].dtype and v.tobytes() == fx[k].tobytes(), k
    out = hp.evaluate(inp)
    for k in ("hp_hi", "hp_lo", "hp_status", "hp_margin"):
        assert out[k].dtype == fx[k].dtype and out[k].tobytes() == fx[k].tobytes(), k
    assert np.array_equal(out["ref_status"], fx["ref_status"])
    cell = fx["cell"]
    for tr in (0, 1):
        # per track the bound the core and the kernel are held to: 16 x the cell's e_ref (the track's own outside the grid)
        e_cell = np.array([fx["e_ref"][tr][cell == c].max() if c >= 0 else fx["e_ref"][tr][t] for t, c in enumerate(cell)])
        bound = np.maximum(16.0 * e_cell, 1e-14 * np.abs(fx["ref"][tr]).max(axis=1))
        assert (np.abs(out["ref"][tr] - fx["ref"][tr]).max(axis=1) <= bound).all()
        assert (out["e_ref"][tr] <= bound).all()


@pytest.mark.parametrize("oi,truncate", CALLS)
def test_core_against_50_digits(fx, core, tmp_path, oi, truncate):
    """The header on the CPU, one command per call.  Measured: the table of the module docstring, column "core"."""
    pts, st = core(fx, oi, truncate, tmp_path)
    _check(fx, oi, truncate, pts, st, "core")


@pytest.mark.gpu
@pytest.mark.parametrize("oi,truncate", CALLS)
def test_device_against_50_digits(fx, gpu_solver_cls, oi, truncate):
    """One bsgpu_triangulate call of 257 tracks on a window holding the offset's keyframes.  Measured: the table of the module
    docstring, column "kernel"."""
    from beam_slam_amd import capi
    from beam_slam_amd.problem import Problem
    start, obs, src = hp.call_layout(fx, oi)
    # the offset's keyframes and tracks as a window: orientation / position blocks, a landmark per track, its reprojection factors
    tracks = np.flatnonzero(fx["offset_id"] == oi)
    lo, hi = int(fx["track_start"][tracks[0]]), int(fx["track_start"][tracks[-1] + 1])
    v0, v1 = int(fx["q_off"][lo:hi].min()), int(fx["p_off"][lo:hi].max()) + 3
    pr = Problem()
    q_block = {}
    for off in range(v0, v1, 7):
        q_block[off] = pr.add_quat(fx["values"][off:off + 4])
        pr.add_block(fx["values"][off + 4:off + 7])
    cam = fx["camera"]
    ci = pr.add_camera(*cam[:4], cam[4:13].reshape(3, 3), cam[13:16])
    idx, consts = [], []
    for t in tracks:
        lm = pr.add_block(fx["hp_hi"][0][t])
        for o in range(int(fx["track_start"][t]), int(fx["track_start"][t + 1])):
            qb = q_block[int(fx["q_off"][o])]
            idx.append([qb, qb + 1, lm, ci]); consts.append([*fx["pixels"][o], 1.0])
    pr.add_factors(capi.F_REPROJ, idx, consts)
    g = gpu_solver_cls(0)
    pr.load(g)
    qb = np.array([q_block[int(fx["q_off"][o])] for o in obs], np.int32)
    pts, st = g.triangulate(start, qb, qb + 1, fx["pixels"][obs], ci, bool(truncate), hp.MAX_DIST, hp.MAX_REPROJ)
    _check(fx, oi, truncate, pts, st, "kernel")
