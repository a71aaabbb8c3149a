"""bsgpu_register_scans_gicp on the device (k_gicp.hip) against the NumPy restatement (tests/gicp_ref.py) and, bit for bit, against the
shared header on the CPU (beam_slam_amd/csrc/gicp.h through tests/plan/test_gicp.cpp); the CPU side of the same checks is
tests/test_gicp.py.

Shapes: the 600- and 4 000-point box scenes of gicp_ref.CASES (5 and 32 chunks of 128 source points); one call of five unequal pairs
(0, k - 1, 600, 4 000 and 257 source points) whose every pair returns the bits of its lone call; the integer grid fixtures (ties,
points on cell faces, distances on the threshold); source clouds 1, 2 and a chunk + 1 points past a chunk boundary on a target one
cell thick; k = 1, 10 and 32; three cell edges; n_pairs == 0; NULL optional outputs; every refused argument.

Accuracy criterion as on the CPU: status and counts equal; rotation block, translation, cost and covariances within 8 x the
restatement's own spread.  The device returns the header's bits, so its figures are those of test_gicp.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import gicp_ref as ref
import icp_ref
from test_gicp import INC, _compile, comparable, parse_reg, reg_command, run_program
from test_icp import grid_clouds

pytestmark = pytest.mark.gpu

CHUNK = int(re.search(r"constexpr int kGridChunk = (\d+);", open(os.path.join(INC, "point_grid.h")).read()).group(1))
K = ref.DEFAULTS["k_neighbors"]


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"], "test_gicp")


def _device(pairs, T_init=None, **kw):
    """pairs: [(S, Q)] -> per pair dict(T, T_ref_tgt, cost, n_corr, n_iters, n_inner, status, ref_cov, tgt_cov)."""
    from beam_slam_amd import gpu
    rs = np.cumsum([0] + [len(s) for s, _ in pairs])
    ts = np.cumsum([0] + [len(q) for _, q in pairs])
    rp = np.concatenate([np.asarray(s, float).reshape(-1, 3) for s, _ in pairs]) if pairs else np.zeros((0, 3))
    tp = np.concatenate([np.asarray(q, float).reshape(-1, 3) for _, q in pairs]) if pairs else np.zeros((0, 3))
    out = gpu.register_scans_gicp(rs, rp, ts, tp, T_init, **dict(ref.DEFAULTS, **kw))
    return [dict(T=out["T_refest_ref"][p], T_ref_tgt=out["T_ref_tgt"][p], cost=float(out["cost"][p]), n_corr=int(out["n_corr"][p]),
                 n_iters=int(out["n_iters"][p]), n_inner=int(out["n_inner"][p]), status=int(out["status"][p]),
                 ref_cov=out["ref_cov"][rs[p]:rs[p + 1]], tgt_cov=out["tgt_cov"][ts[p]:ts[p + 1]]) for p in range(len(pairs))]


def _same_bits(a, b, what):
    assert (a["status"], a["n_iters"], a["n_inner"], a["n_corr"]) == (b["status"], b["n_iters"], b["n_inner"], b["n_corr"]), what
    assert np.float64(a["cost"]).tobytes() == np.float64(b["cost"]).tobytes(), (what, a["cost"], b["cost"])
    for k in ("T", "T_ref_tgt", "ref_cov", "tgt_cov"):
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (what, k, np.abs(a[k] - b[k]).max())


def _header(core, tmp_path, runs):
    """runs: [(S, Q, keyword arguments)] -> the header's results, covariances included"""
    rows = run_program(core, [reg_command(S, Q, want_cov=True, **kw) for S, Q, kw in runs], tmp_path)
    return [parse_reg(tok, len(S), len(Q)) for (S, Q, _), tok in zip(runs, rows)]


def _unequal_pairs():
    """0, k - 1, 600, 4 000 and 257 source points; targets 600, 600, 600, 4 000 and 600."""
    S6, Q6 = ref.scene(600)
    S4, Q4 = ref.scene(4000)
    return [(S6[:0], Q6), (S6[:K - 1], Q6), (S6, Q6), (S4, Q4), (S6[:257], Q6)]


def _integer_runs():
    """The integer-coordinate grid fixtures as registration inputs (three outer iterations are enough to compare bits)."""
    runs = []
    for S, Q, h in grid_clouds()[:13]:
        runs.append((S, Q, dict(ref.DEFAULTS, max_corr=1.0, max_iter=3)))
    runs.append(grid_clouds()[0][:2] + (dict(ref.DEFAULTS, max_corr=5.0, max_iter=3),))
    return runs


@pytest.mark.parametrize("name", list(ref.CASES))
def test_device_against_restatement(name):
    """One pair per call.  Measured on an MI355X (2026-10-20): the header's figures (test_gicp.py), since the device returns its bits."""
    S, Q, kw, results = comparable(name)
    res = results["plain"]
    got = _device([(S, Q)], **kw)[0]
    assert (got["status"], got["n_iters"], got["n_inner"], got["n_corr"]) == (res["status"], res["n_iters"], res["n_inner"], res["n_corr"])
    ref.check(got, results, "kernel " + name, quantities=("R", "t", "cost", "ref_cov", "tgt_cov"))
    assert np.abs(got["T_ref_tgt"] - res["T_ref_tgt"]).max() < 1e-12


def test_device_equals_header_bit_for_bit(core, tmp_path):
    """The four cases, the five unequal pairs and the integer grid fixtures: T, T_ref_tgt, cost, the counts and every covariance of the
    device are the header's, bit for bit — the sums have one order on both sides and no product is fused on one side only."""
    runs = [(ref.scene(n) + (dict(ref.DEFAULTS, **kw),)) for n, kw in ref.CASES.values()] + [p + (ref.DEFAULTS,) for p in _unequal_pairs()]
    runs += _integer_runs()
    for k, ((S, Q, kw), want) in enumerate(zip(runs, _header(core, tmp_path, runs))):
        _same_bits(_device([(S, Q)], **kw)[0], want, k)


def test_batch_equals_lone_calls():
    """Five unequal pairs in one call: every pair returns the bits of its lone call."""
    pairs = _unequal_pairs()
    together = _device(pairs)
    assert [o["status"] for o in together] == [ref.TOO_FEW, ref.TOO_FEW, ref.TRANSFORM, ref.TRANSFORM, ref.TRANSFORM]
    assert together[0]["n_iters"] == 0 and (together[1]["T"] == ref.EYE).all() and not together[1]["ref_cov"].any()
    for k, o in enumerate(together):
        _same_bits(o, _device([pairs[k]])[0], k)


@pytest.mark.parametrize("n_src", [CHUNK + 1, CHUNK + 2, 2 * CHUNK + 1])
def test_chunk_boundaries_and_flat_target(n_src, core, tmp_path):
    """Source clouds that end 1, 2 and a chunk + 1 points past a chunk boundary, on a target one cell thick in z (points of the floor
    only): the restatement's decisions, the header's bits."""
    S, Q = ref.scene(4000)
    floor = lambda P: P[np.abs(P[:, 2] + 2.5) < 0.2]
    s, q = floor(S)[:n_src], floor(Q @ icp_ref.MOTION_R - icp_ref.MOTION_T @ icp_ref.MOTION_R + [0.05, -0.03, 0.0])
    assert len(s) == n_src and np.ptp(q[:, 2]) < 0.5
    kw = dict(ref.DEFAULTS, max_iter=4)
    res = ref.run(s, q, **kw)
    got = _device([(s, q)], **kw)[0]
    assert res["gap"] > 1e-9 and res["margin"] > 1e-9 and res["knn_gap"] > 1e-9
    assert (got["status"], got["n_iters"], got["n_inner"], got["n_corr"]) == (res["status"], res["n_iters"], res["n_inner"], res["n_corr"])
    assert res["n_corr"] > 4
    _same_bits(got, _header(core, tmp_path, [(s, q, kw)])[0], n_src)


@pytest.mark.parametrize("k", [1, 10, 32])
def test_neighbour_counts(k, core, tmp_path):
    """k = 1 (every C' is diag(1, 1, epsilon)), the shipped 10 and the cap 32, eight outer iterations: the header's bits."""
    S, Q = ref.scene(600)
    kw = dict(ref.DEFAULTS, k_neighbors=k, max_iter=8)
    got = _device([(S, Q)], **kw)[0]
    _same_bits(got, _header(core, tmp_path, [(S, Q, kw)])[0], k)
    assert got["n_corr"] == 600 and got["status"] in (ref.TRANSFORM, ref.MAX_ITERATIONS)
    if k == 1:
        assert (got["ref_cov"] == [1.0, 0.0, 0.0, 1.0, 0.0, ref.DEFAULTS["gicp_epsilon"]]).all()


def test_grid_cell_is_a_performance_knob_only():
    """Cell edges 0.25, 0.5 and 1000 (one cell): every output of the device, covariances included, has the same bytes."""
    S, Q, kw, _ = ref.case("n600_k10_c5")
    first = _device([(S, Q)], grid_cell=0.25, **kw)[0]
    for h in (0.5, 1000.0):
        _same_bits(first, _device([(S, Q)], grid_cell=h, **kw)[0], h)


def test_initial_transform():
    """T_init is applied to the target on the device: a quarter turn about z and a translation, whose products are exact, give the
    bits of the call on the target transformed beforehand; T_ref_tgt = inv(T_refest_ref) T_init."""
    S, Q = ref.scene(600)
    Ti = np.array([[0.0, -1.0, 0.0, 0.25], [1.0, 0.0, 0.0, -1.5], [0.0, 0.0, 1.0, 0.125]])
    back = np.asarray(Q) - Ti[:, 3]
    raw = np.stack([back[:, 1], -back[:, 0], back[:, 2]], axis=1)
    moved = ref.transform(Ti, raw)
    a, b = _device([(S, raw)], T_init=Ti[None])[0], _device([(S, moved)])[0]
    assert a["status"] == ref.TRANSFORM and a["T"].tobytes() == b["T"].tobytes() and a["cost"] == b["cost"] and a["n_corr"] == b["n_corr"]
    assert a["tgt_cov"].tobytes() == b["tgt_cov"].tobytes()
    T4, Ti4 = np.vstack([a["T"], [0, 0, 0, 1]]), np.vstack([Ti, [0, 0, 0, 1]])
    assert np.abs(np.linalg.inv(T4) @ Ti4 - np.vstack([a["T_ref_tgt"], [0, 0, 0, 1]])).max() < 1e-13


def test_no_pairs():
    from beam_slam_amd import gpu
    out = gpu.register_scans_gicp([0], np.zeros((0, 3)), [0], np.zeros((0, 3)))
    assert out["status"].shape == (0,) and out["T_refest_ref"].shape == (0, 3, 4) and out["ref_cov"].shape == (0, 6)


def _raw():
    from beam_slam_amd import capi, gpu
    fn = gpu.lib().bsgpu_register_scans_gicp
    fn.argtypes = capi.REGISTER_SCANS_GICP_ARGTYPES
    return fn, capi, gpu


def _raw_args(capi, S, Q, T, st):
    dp, ip = capi._dp, capi._ip
    rs = np.array([0, len(S)], np.int32)
    ts = np.array([0, len(Q)], np.int32)
    d = ref.DEFAULTS
    null_d, null_i = ctypes.cast(None, dp), ctypes.cast(None, ip)
    return [0, 1, rs.ctypes.data_as(ip), S.ctypes.data_as(dp), ts.ctypes.data_as(ip), Q.ctypes.data_as(dp), null_d, d["k_neighbors"],
            d["gicp_epsilon"], d["max_corr"], d["max_iter"], d["r_eps"], d["t_eps"], d["max_inner"], d["inner_eps"], 0.5, T.ctypes.data_as(dp),
            null_d, null_d, null_i, null_i, null_i, st.ctypes.data_as(ip), null_d, null_d], (rs, ts)


def test_optional_outputs_may_be_null():
    fn, capi, gpu = _raw()
    S, Q = (np.ascontiguousarray(a) for a in ref.scene(600))
    T, st = np.zeros(12), np.zeros(1, np.int32)
    args, keep = _raw_args(capi, S, Q, T, st)
    full = _device([(S, Q)])[0]
    assert fn(*args) == 0 and st[0] == full["status"] and T.tobytes() == np.ascontiguousarray(full["T"]).tobytes()
    # one covariance array alone
    cov = np.zeros((600, 6))
    args[24] = cov.ctypes.data_as(capi._dp)
    assert fn(*args) == 0 and cov.tobytes() == np.ascontiguousarray(full["tgt_cov"]).tobytes()


def test_argument_errors():
    """Every refused argument: its code and what bsgpu_register_scans_error then says; nothing is written."""
    fn, capi, gpu = _raw()
    S, Q = (np.ascontiguousarray(a) for a in ref.scene(600))
    two = lambda a: np.concatenate([a, a])

    def refused(code, message, **over):
        kw = dict(ref_start=[0, 600, 1200], ref_points=two(S), tgt_start=[0, 600, 1200], tgt_points=two(Q), T_init=None, **ref.DEFAULTS)
        kw.update(over)
        with pytest.raises(capi.SolverError) as e:
            gpu.register_scans_gicp(**kw)
        assert e.value.code == code and "register_scans_gicp: " in str(e.value) and message in str(e.value), (over.keys(), str(e.value))

    inv, uns = capi.ERR_INVALID, capi.ERR_UNSUPPORTED
    refused(inv, "ref_start[0] must be 0", ref_start=[1, 600, 1200])
    refused(inv, "ref_start must be non-decreasing", ref_start=[0, 700, 600])
    refused(inv, "tgt_start[0] must be 0", tgt_start=[2, 600, 1200])
    refused(inv, "tgt_start must be non-decreasing", tgt_start=[0, 900, 800])
    refused(inv, "name more points than were passed", ref_start=[0, 600, 1201])
    for bad in (np.nan, np.inf):
        pts = two(S)
        pts[700, 1] = bad
        refused(inv, "non-finite reference points", ref_points=pts)
        pts = two(Q)
        pts[1199, 2] = bad
        refused(inv, "non-finite target points", tgt_points=pts)
    Ti = np.stack([ref.EYE, ref.EYE])
    Ti[1, 2, 3] = np.nan
    refused(inv, "non-finite T_init", T_init=Ti)
    refused(inv, "array sizes do not agree", T_init=ref.EYE[None])
    for bad in (0.0, np.inf, np.nan):
        refused(inv, "max_corr must be positive and finite", max_corr=bad)
        refused(inv, "grid_cell must be positive and finite", grid_cell=bad)
    refused(inv, "k_neighbors must be at least 1", k_neighbors=0)
    refused(uns, "k_neighbors exceeds BSGPU_GICP_MAX_K", k_neighbors=capi.GICP_MAX_K + 1)
    for bad in (0.0, -1e-3, 1.5, np.nan):
        refused(inv, "gicp_epsilon must lie in (0, 1]", gicp_epsilon=bad)
    refused(inv, "max_iter must be at least 1", max_iter=0)
    refused(uns, "max_iter exceeds BSGPU_ICP_MAX_ITER", max_iter=capi.ICP_MAX_ITER + 1)
    refused(inv, "max_inner must be at least 1", max_inner=0)
    refused(uns, "max_inner exceeds BSGPU_GICP_MAX_INNER", max_inner=capi.GICP_MAX_INNER + 1)
    refused(inv, "must not be negative or NaN", r_eps=-1.0)
    refused(inv, "must not be negative or NaN", t_eps=np.nan)
    refused(inv, "must not be negative or NaN", inner_eps=-1e-12)
    # the cell cap: two points 100 m apart in every axis span 201^3 > 2^22 cells of 0.5 m; 50 m apart they are accepted
    wide = np.array([[0.0, 0.0, 0.0], [100.0, 100.0, 100.0]])
    refused(uns, "a cloud's grid exceeds BSGPU_ICP_MAX_CELLS cells", tgt_start=[0, 600, 602], tgt_points=np.concatenate([Q, wide]))
    refused(uns, "a cloud's grid exceeds BSGPU_ICP_MAX_CELLS cells", ref_start=[0, 600, 602], ref_points=np.concatenate([S, wide]))
    ok = gpu.register_scans_gicp([0, 600], S, [0, 2], wide * 0.5)
    assert ok["status"][0] == ref.TOO_FEW and ok["n_iters"][0] == 0
    # 17 target grids of 161^3 cells: each below the cap, together above 16 x the cap
    n = 17
    refused(uns, "the call's grids exceed 16 x BSGPU_ICP_MAX_CELLS cells", ref_start=[0] * (n + 1), ref_points=S[:0],
            tgt_start=np.arange(n + 1) * 2, tgt_points=np.tile(wide * 0.8, (n, 1)))
    # NULL where an array is needed, a negative count: through the raw entry point; the outputs stay untouched
    dp, ip = capi._dp, capi._ip
    T, st = np.full(12, 7.0), np.full(1, 7, np.int32)
    args, keep = _raw_args(capi, S, Q, T, st)
    for i, message in ((2, "null argument"), (3, "null or non-finite reference points"), (4, "null argument"), (5, "null or non-finite target points"),
                       (16, "null argument"), (22, "null argument")):
        bad = list(args)
        bad[i] = ctypes.cast(None, ip if i in (2, 4, 22) else dp)
        assert fn(*bad) == inv and message in gpu.register_scans_error(), i
    assert fn(0, -1, *args[2:]) == inv
    assert (T == 7.0).all() and st[0] == 7
    assert fn(*args) == 0 and st[0] == ref.TRANSFORM
