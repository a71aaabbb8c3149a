"""bsgpu_register_scans on the device (k_icp.hip) against the NumPy restatement (tests/icp_ref.py) and, bit for bit, against the shared
header on the CPU (beam_slam_amd/csrc/icp.h through tests/plan/test_icp.cpp); the CPU side of the same checks is tests/test_icp.py.

Shapes: the 600- and 4 000-point box scenes at fit_eps 1e-2 and 0 (5 and 32 chunks of 128 source points); one call of five unequal
pairs (0, 3, 600, 4 000 and 257 source points) whose every pair returns the bits of its lone call; source clouds 1, 2 and a chunk + 1
points past a chunk boundary; a target one cell thick; n_pairs == 0; T_init; NULL optional outputs; every refused argument.

Accuracy criterion as on the CPU: n_iters, status, n_corr equal; rotation block, translation and mse within 8 x the restatement's own
difference under a reversed summation order.  Measured on an MI355X: see test_device_against_restatement.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import icp_ref as ref
from test_icp import INC, _compile, comparable, parse_reg, reg_command, run_program

pytestmark = pytest.mark.gpu

CHUNK = int(re.search(r"constexpr int kGridChunk = (\d+);", open(os.path.join(INC, "point_grid.h")).read()).group(1))


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"], "test_icp")


def _device(pairs, T_init=None, **kw):
    """pairs: [(S, Q)] -> per pair dict(T, T_ref_tgt, mse, n_corr, n_iters, status)."""
    from beam_slam_amd import gpu
    rs = np.cumsum([0] + [len(s) for s, _ in pairs])
    ts = np.cumsum([0] + [len(q) for _, q in pairs])
    rp = np.concatenate([np.asarray(s, float).reshape(-1, 3) for s, _ in pairs]) if pairs else np.zeros((0, 3))
    tp = np.concatenate([np.asarray(q, float).reshape(-1, 3) for _, q in pairs]) if pairs else np.zeros((0, 3))
    out = gpu.register_scans(rs, rp, ts, tp, T_init, **dict(ref.DEFAULTS, **kw))
    return [dict(T=out["T_refest_ref"][p], T_ref_tgt=out["T_ref_tgt"][p], mse=float(out["mse"][p]), n_corr=int(out["n_corr"][p]),
                 n_iters=int(out["n_iters"][p]), status=int(out["status"][p])) for p in range(len(pairs))]


def _same_bits(a, b, what):
    assert (a["status"], a["n_iters"], a["n_corr"]) == (b["status"], b["n_iters"], b["n_corr"]), what
    assert np.float64(a["mse"]).tobytes() == np.float64(b["mse"]).tobytes(), (what, a["mse"], b["mse"])
    for k in ("T", "T_ref_tgt"):
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (what, k, np.abs(a[k] - b[k]).max())


def _unequal_pairs():
    """0, 3, 600, 4 000 and 257 source points; targets 600, 600, 600, 4 000 and 600."""
    S6, Q6 = ref.scene(600)
    S4, Q4 = ref.scene(4000)
    return [(S6[:0], Q6), (S6[:3], Q6), (S6, Q6), (S4, Q4), (S6[:257], Q6)]


@pytest.mark.parametrize("name", list(ref.CASES))
def test_device_against_restatement(name):
    """One pair per call.  Measured on an MI355X (2026-10-19), difference / bound per quantity — the header's figures, since the
    device returns the header's bits:
        n600_fit     R 0.056  t 0.125  mse 0.083        n600_nofit   R 0.050  t 0.080  mse 0.000
        n4000_fit    R 0.234  t 0.055  mse 0.313        n4000_nofit  R 0.208  t 0.068  mse 0.188
    """
    S, Q, kw, res, rev = comparable(name)
    got = _device([(S, Q)], **kw)[0]
    assert (got["status"], got["n_iters"], got["n_corr"]) == (res["status"], res["n_iters"], res["n_corr"])
    ref.check(got["T"], got["mse"], res, rev, "kernel " + name)
    assert np.abs(got["T_ref_tgt"] - res["T_ref_tgt"]).max() < 1e-12


def test_device_equals_header_bit_for_bit(core, tmp_path):
    """The four cases and the five unequal pairs: T, T_ref_tgt, mse and the counts of the device are the header's, bit for bit — the sums
    have one order on both sides and no product is fused on one side only."""
    runs = [(ref.scene(n) + (dict(ref.DEFAULTS, **kw),)) for n, kw in ref.CASES.values()] + [p + (ref.DEFAULTS,) for p in _unequal_pairs()]
    rows = run_program(core, [reg_command(S, Q, **kw) for S, Q, kw in runs], tmp_path)
    for k, ((S, Q, kw), tok) in enumerate(zip(runs, rows)):
        _same_bits(_device([(S, Q)], **kw)[0], parse_reg(tok), k)


def test_batch_equals_lone_calls():
    """Five unequal pairs in one call: every pair (the 600-point one is item 3) returns the bits of its lone call."""
    pairs = _unequal_pairs()
    together = _device(pairs)
    assert [o["status"] for o in together] == [ref.TOO_FEW, ref.TRANSFORM, ref.ABS_MSE, ref.ABS_MSE, ref.ABS_MSE]
    for k, o in enumerate(together):
        _same_bits(o, _device([pairs[k]])[0], k)


@pytest.mark.parametrize("n_src", [CHUNK + 1, CHUNK + 2, 2 * CHUNK + 1])
def test_chunk_boundaries_and_flat_target(n_src, core, tmp_path):
    """Source clouds that end 1, 2 and a chunk + 1 points past a chunk boundary, on a target one cell thick in z (points of the floor
    only): the restatement's decisions, the header's bits."""
    S, Q = ref.scene(4000)
    floor = lambda P: P[np.abs(P[:, 2] + 2.5) < 0.2]
    s, q = floor(S)[:n_src], floor(Q @ ref.MOTION_R - ref.MOTION_T @ ref.MOTION_R + [0.05, -0.03, 0.0])
    assert len(s) == n_src and np.ptp(q[:, 2]) < 1.0
    res = ref.run(s, q, **ref.DEFAULTS)
    got = _device([(s, q)])[0]
    assert res["gap"] > 1e-9 and res["margin"] > 1e-9
    assert (got["status"], got["n_iters"], got["n_corr"]) == (res["status"], res["n_iters"], res["n_corr"]) and res["n_corr"] > 3
    _same_bits(got, parse_reg(run_program(core, [reg_command(s, q)], tmp_path)[0]), n_src)


def test_initial_transform():
    """T_init is applied to the target on the device: a quarter turn about z and a translation, whose products are exact, give the
    bits of the call on the target transformed beforehand; T_ref_tgt = inv(T_refest_ref) T_init."""
    S, Q = ref.scene(600)
    Ti = np.array([[0.0, -1.0, 0.0, 0.25], [1.0, 0.0, 0.0, -1.5], [0.0, 0.0, 1.0, 0.125]])
    back = np.asarray(Q) - Ti[:, 3]
    raw = np.stack([back[:, 1], -back[:, 0], back[:, 2]], axis=1)          # Ti raw = Q, up to the rounding of the subtraction
    moved = ref.transform(Ti, raw)
    a, b = _device([(S, raw)], T_init=Ti[None])[0], _device([(S, moved)])[0]
    assert a["status"] == ref.ABS_MSE and a["T"].tobytes() == b["T"].tobytes() and a["mse"] == b["mse"] and a["n_corr"] == b["n_corr"]
    T4, Ti4 = np.vstack([a["T"], [0, 0, 0, 1]]), np.vstack([Ti, [0, 0, 0, 1]])
    assert np.abs(np.linalg.inv(T4) @ Ti4 - np.vstack([a["T_ref_tgt"], [0, 0, 0, 1]])).max() < 1e-13
    assert np.abs(b["T_ref_tgt"] - np.linalg.inv(T4)[:3]).max() < 1e-13


def test_no_pairs():
    from beam_slam_amd import gpu
    out = gpu.register_scans([0], np.zeros((0, 3)), [0], np.zeros((0, 3)))
    assert out["status"].shape == (0,) and out["T_refest_ref"].shape == (0, 3, 4)


def _raw():
    from beam_slam_amd import capi, gpu
    fn = gpu.lib().bsgpu_register_scans
    fn.argtypes = capi.REGISTER_SCANS_ARGTYPES
    return fn, capi, gpu


def test_optional_outputs_may_be_null():
    fn, capi, gpu = _raw()
    S, Q = ref.scene(600)
    dp, ip = capi._dp, capi._ip
    rs, ts = np.array([0, 600], np.int32), np.array([0, 600], np.int32)
    S, Q = np.ascontiguousarray(S), np.ascontiguousarray(Q)
    T, st = np.zeros(12), np.zeros(1, np.int32)
    full = _device([(S, Q)])[0]
    null_d, null_i = ctypes.cast(None, dp), ctypes.cast(None, ip)
    rc = fn(0, 1, rs.ctypes.data_as(ip), S.ctypes.data_as(dp), ts.ctypes.data_as(ip), Q.ctypes.data_as(dp), null_d, 1.0, 50, 1e-8, 1e-2, 0.99999,
            1e-5, T.ctypes.data_as(dp), null_d, null_d, null_i, null_i, st.ctypes.data_as(ip))
    assert rc == 0 and st[0] == full["status"] and T.tobytes() == np.ascontiguousarray(full["T"]).tobytes()


def test_argument_errors():
    """Every refused argument: its code and what bsgpu_register_scans_error then says; nothing is written."""
    fn, capi, gpu = _raw()
    S, Q = (np.ascontiguousarray(a) for a in ref.scene(600))
    two = lambda a: np.concatenate([a, a])

    def refused(code, message, **over):
        kw = dict(ref_start=[0, 600, 1200], ref_points=two(S), tgt_start=[0, 600, 1200], tgt_points=two(Q), T_init=None, **ref.DEFAULTS)
        kw.update(over)
        with pytest.raises(capi.SolverError) as e:
            gpu.register_scans(**kw)
        assert e.value.code == code and message in str(e.value), (over.keys(), str(e.value))

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
    refused(inv, "max_corr must be positive and finite", max_corr=0.0)
    refused(inv, "max_corr must be positive and finite", max_corr=np.inf)
    refused(inv, "max_corr must be positive and finite", max_corr=np.nan)
    refused(inv, "max_iter must be at least 1", max_iter=0)
    refused(uns, "max_iter exceeds BSGPU_ICP_MAX_ITER", max_iter=capi.ICP_MAX_ITER + 1)
    refused(inv, "must not be negative", t_eps=-1.0)
    refused(inv, "must not be negative", fit_eps=np.nan)
    refused(inv, "must not be negative", rel_mse_eps=-1e-9)
    refused(inv, "no tolerance NaN", rotation_threshold=np.nan)
    # the cell cap: two target points 200 m apart in every axis span 201^3 > 2^22 cells of 1 m; 100 m apart they are accepted
    wide = np.array([[0.0, 0.0, 0.0], [200.0, 200.0, 200.0]])
    refused(uns, "a pair's grid exceeds BSGPU_ICP_MAX_CELLS cells", tgt_start=[0, 600, 602], tgt_points=np.concatenate([Q, wide]))
    ok = gpu.register_scans([0, 600], S, [0, 2], wide * 0.5)
    assert ok["status"][0] == ref.TOO_FEW and ok["n_corr"][0] <= 2
    # 17 grids of 161^3 cells: each below the cap, together above 16 x the cap
    n = 17
    refused(uns, "the call's grids exceed 16 x BSGPU_ICP_MAX_CELLS cells", ref_start=[0] * (n + 1), ref_points=S[:0],
            tgt_start=np.arange(n + 1) * 2, tgt_points=np.tile(wide * 0.8, (n, 1)))
    # NULL where an array is needed, a negative count: through the raw entry point; the outputs stay untouched
    dp, ip = capi._dp, capi._ip
    rs = np.array([0, 600], np.int32)
    T, st = np.full(12, 7.0), np.full(1, 7, np.int32)
    args = [0, 1, rs.ctypes.data_as(ip), S.ctypes.data_as(dp), rs.ctypes.data_as(ip), Q.ctypes.data_as(dp), ctypes.cast(None, dp), 1.0, 50, 1e-8,
            1e-2, 0.99999, 1e-5, T.ctypes.data_as(dp), ctypes.cast(None, dp), ctypes.cast(None, dp), ctypes.cast(None, ip), ctypes.cast(None, ip),
            st.ctypes.data_as(ip)]
    for i, message in ((2, "null argument"), (3, "null or non-finite reference points"), (4, "null argument"), (5, "null or non-finite target points"),
                       (13, "null argument"), (18, "null argument")):
        bad = list(args)
        bad[i] = ctypes.cast(None, ip if i in (2, 4, 18) else dp)
        assert fn(*bad) == inv and message in gpu.register_scans_error(), i
    assert fn(0, -1, *args[2:]) == inv
    assert (T == 7.0).all() and st[0] == 7
    assert fn(*args) == 0 and st[0] == ref.ABS_MSE
