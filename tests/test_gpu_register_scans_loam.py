"""bsgpu_register_scans_loam on the device (k_loam.hip) against the NumPy restatement (tests/loam_ref.py) and, bit for bit, against the
shared header on the CPU (beam_slam_amd/csrc/loam.h through tests/plan/test_loam.cpp); the CPU side of the same checks is
tests/test_loam.py.

Shapes: the cases of loam_ref.CASES (target 150 + 300 features: 4 chunks of 128; 700 + 1 500: 18 chunks); every status; the integer grid
fixtures (ties, points on cell faces, neighbours on the threshold, duplicates, collinear triples); target feature counts a chunk + 1,
a chunk + 2 and two chunks + 1, and one below, at and one above the workgroup's width (which is a chunk); one call of six unequal pairs
whose every pair returns the bits of its lone call; three cell edges; T_init; n_pairs == 0; NULL optional outputs; every refused
argument.

Accuracy criterion as on the CPU: status and counts equal; rotation block, translation, cost and covariance within 8 x the
restatement's own spread.  The device returns the header's bits, so its figures are those of test_loam.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import loam_ref as ref
from test_icp import grid_clouds, run_program
from test_loam import INC, QUARTER, _compile, comparable, counts, parse_reg, quarter_turn, reg_command, status_runs

pytestmark = pytest.mark.gpu

CHUNK = int(re.search(r"constexpr int kGridChunk = (\d+);", open(os.path.join(INC, "point_grid.h")).read()).group(1))
KEYS = ("T_refest_ref", "T_ref_tgt", "cov")


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"], "test_loam")


def _device(pairs, T_init=None, **kw):
    """pairs: [(ref edges, ref surfaces, tgt edges, tgt surfaces)] -> per pair the outputs as parse_reg gives the header's"""
    from beam_slam_amd import gpu
    args = []
    for c in range(4):
        args.append(np.cumsum([0] + [len(p[c]) for p in pairs]))
        args.append(np.concatenate([np.asarray(p[c], float).reshape(-1, 3) for p in pairs]) if pairs else np.zeros((0, 3)))
    out = gpu.register_scans_loam(*args, T_init, **dict(ref.DEFAULTS, **kw))
    return [dict({k: out[k][p] for k in KEYS}, cost=float(out["cost"][p]), **{k: int(out[k][p]) for k in ref.COUNTS}) for p in range(len(pairs))]


def _same_bits(a, b, what):
    assert counts(a) == counts(b), (what, counts(a), counts(b))
    assert np.float64(a["cost"]).tobytes() == np.float64(b["cost"]).tobytes() or (np.isnan(a["cost"]) and np.isnan(b["cost"])), (what, a["cost"], b["cost"])
    for k in KEYS:
        x, y = np.ascontiguousarray(a[k], float), np.ascontiguousarray(b[k], float)
        assert (np.isnan(x) == np.isnan(y)).all(), (what, k)
        assert np.where(np.isnan(x), 0.0, x).tobytes() == np.where(np.isnan(y), 0.0, y).tobytes(), (what, k, np.nanmax(np.abs(x - y)))


def _header(core, tmp_path, runs):
    """runs: [(clouds, T_init, keyword arguments)] -> the header's results"""
    return [parse_reg(tok) for tok in run_program(core, [reg_command(c, T_init=Ti, **kw) for c, Ti, kw in runs], tmp_path)]


def _case_runs():
    return [(ref.case(name)[0], ref.case(name)[2], ref.case(name)[1]) for name in ref.CASES]


def _integer_runs():
    """The integer-coordinate grid fixtures as registration inputs: the queries as target edges and surfaces, the cloud as both reference
    clouds; two outer iterations are enough to compare bits."""
    kw = dict(ref.DEFAULTS, max_corr=1.5, min_measurements=3, max_outer=2)
    return [((Q, Q, S, S[::-1]), None, dict(kw, max_corr=mc)) for S, Q, _ in grid_clouds()[:13] for mc in (1.0, 1.5)]


def _unequal_pairs():
    """no features; min_measurements - 1 measurements; edges only; surfaces only; the small scene; the large scene"""
    RE, RS, TE, TS = ref.scene(*ref.SMALL)
    few = [r for r in status_runs() if r[0] == "one too few"][0]
    return [(RE, RS, TE[:0], TS[:0]), few[1], (RE, RS[:0], TE, TS[:0]), (RE[:0], RS, TE[:0], TS), (RE, RS, TE, TS), ref.scene(*ref.LARGE)], few[2]


@pytest.mark.parametrize("name", list(ref.CASES))
def test_device_against_restatement(name):
    """One pair per call.  The header's figures (test_loam.py), since the device returns its bits."""
    clouds, kw, Ti, results, want = comparable(name)
    res = results["plain"]
    got = _device([clouds], T_init=None if Ti is None else Ti[None], **kw)[0]
    assert counts(got) == counts(res) and got["status"] == want
    ref.check(got, results, "kernel " + name)
    assert np.abs(got["T_ref_tgt"] - res["T_ref_tgt"]).max() < 1e-12


def test_device_equals_header_bit_for_bit(core, tmp_path):
    """The cases, every status and the integer grid fixtures: every output of the device, the covariance included, is the header's, bit
    for bit — the sums have one order on both sides, no product is fused on one side only, and neither side calls a library sine."""
    runs = _case_runs() + [(c, None, dict(ref.DEFAULTS, **kw)) for _, c, kw, _ in status_runs()] + _integer_runs()
    for k, ((clouds, Ti, kw), want) in enumerate(zip(runs, _header(core, tmp_path, runs))):
        assert want["ok"] == 1
        _same_bits(_device([clouds], T_init=None if Ti is None else Ti[None], **kw)[0], want, k)


@pytest.mark.parametrize("n_tgt", [CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, 2 * CHUNK + 1])
def test_chunk_and_workgroup_boundaries(n_tgt, core, tmp_path):
    """Target feature counts one below, at and one above the workgroup's width (a chunk), a chunk + 2 and two chunks + 1, a third of them
    edges: the restatement's decisions, the header's bits."""
    RE, RS, TE, TS = ref.scene(*ref.SMALL)
    n_edge = n_tgt // 3
    clouds = (RE, RS, TE[:n_edge], TS[:n_tgt - n_edge])
    kw = dict(ref.DEFAULTS, max_corr=1.5, max_outer=3)
    res = ref.run(*clouds, **kw)
    got = _device([clouds], **kw)[0]
    assert min(res["knn_gap"], res["margin"], res["lm_margin"], res["outer_margin"]) > 1e-9
    assert counts(got) == counts(res) and res["n_edge"] + res["n_surf"] > n_tgt - 8
    _same_bits(got, _header(core, tmp_path, [(clouds, None, kw)])[0], n_tgt)


def test_batch_equals_lone_calls():
    """Six unequal pairs in one call: every pair returns the bits of its lone call."""
    pairs, kw = _unequal_pairs()
    kw = dict(ref.DEFAULTS, **kw)
    together = _device(pairs, **kw)
    assert [o["status"] for o in together] == [ref.TOO_FEW, ref.TOO_FEW, ref.TRANSFORM, ref.TRANSFORM, ref.TRANSFORM, ref.TRANSFORM]
    assert together[0]["n_iters"] == 0 and (together[1]["T_refest_ref"] == ref.EYE).all() and np.isnan(together[1]["cov"]).all()
    assert together[1]["n_edge"] + together[1]["n_surf"] == kw["min_measurements"] - 1
    assert together[2]["n_surf"] == 0 and together[3]["n_edge"] == 0
    for k, o in enumerate(together):
        _same_bits(o, _device([pairs[k]], **kw)[0], k)


def test_grid_cell_is_a_performance_knob_only():
    """Cell edges 0.25, 0.5 and 1000 (one cell): every output of the device has the same bytes."""
    clouds, kw, Ti, _, _ = ref.case("small_huber")
    first = _device([clouds], grid_cell=0.25, **kw)[0]
    for h in (0.5, 1000.0):
        _same_bits(first, _device([clouds], grid_cell=h, **kw)[0], h)


def test_initial_transform():
    """T_init is applied to the target features on the device: an exact quarter turn gives the bits of the call on the features
    transformed beforehand; T_ref_tgt = inv(T_refest_ref) T_init."""
    clouds, kw, _, _, _ = ref.case("small_huber")
    RE, RS, TE, TS = clouds
    raw = (RE, RS, quarter_turn(TE, QUARTER), quarter_turn(TS, QUARTER))
    moved = (RE, RS, ref.transform(QUARTER, raw[2]), ref.transform(QUARTER, raw[3]))
    a, b = _device([raw], T_init=QUARTER[None], **kw)[0], _device([moved], **kw)[0]
    assert a["status"] == ref.TRANSFORM and counts(a) == counts(b) and a["cost"] == b["cost"]
    assert a["T_refest_ref"].tobytes() == b["T_refest_ref"].tobytes() and a["cov"].tobytes() == b["cov"].tobytes()
    T4, Ti4 = np.vstack([a["T_refest_ref"], [0, 0, 0, 1]]), np.vstack([QUARTER, [0, 0, 0, 1]])
    assert np.abs(np.linalg.inv(T4) @ Ti4 - np.vstack([a["T_ref_tgt"], [0, 0, 0, 1]])).max() < 1e-13


def test_no_pairs():
    from beam_slam_amd import gpu
    z = np.zeros((0, 3))
    out = gpu.register_scans_loam([0], z, [0], z, [0], z, [0], z)
    assert out["status"].shape == (0,) and out["T_refest_ref"].shape == (0, 3, 4) and out["cov"].shape == (0, 6, 6)


def _raw():
    from beam_slam_amd import capi, gpu
    fn = gpu.lib().bsgpu_register_scans_loam
    fn.argtypes = capi.REGISTER_SCANS_LOAM_ARGTYPES
    return fn, capi, gpu


def _raw_args(capi, gpu, clouds, kw, T, st):
    dp, ip = capi._dp, capi._ip
    starts = [np.array([0, len(c)], np.int32) for c in clouds]
    null_d, null_i = ctypes.cast(None, dp), ctypes.cast(None, ip)
    opt = gpu.loam_options()
    args = [0, 1]
    for s, c in zip(starts, clouds):
        args += [s.ctypes.data_as(ip), c.ctypes.data_as(dp)]
    args += [null_d, kw["max_corr"], kw["min_measurements"], kw["max_outer"], kw["conv_translation_m"], kw["conv_rotation_deg"], ctypes.pointer(opt),
             kw["loss_kind"], kw["loss_a"], 0.5, T.ctypes.data_as(dp), null_d, null_d, null_d, null_i, null_i, null_i, null_i, st.ctypes.data_as(ip)]
    return args, (starts, opt)


def test_optional_outputs_may_be_null():
    fn, capi, gpu = _raw()
    clouds, kw, _, _, _ = ref.case("small_huber")
    clouds = [np.ascontiguousarray(c) for c in clouds]
    T, st = np.zeros(12), np.zeros(1, np.int32)
    args, keep = _raw_args(capi, gpu, clouds, kw, T, st)
    full = _device([clouds], **kw)[0]
    assert fn(*args) == 0 and st[0] == full["status"] and T.tobytes() == np.ascontiguousarray(full["T_refest_ref"]).tobytes()
    cov = np.zeros((6, 6))
    args[22] = cov.ctypes.data_as(capi._dp)
    assert fn(*args) == 0 and cov.tobytes() == np.ascontiguousarray(full["cov"]).tobytes()


def test_argument_errors():
    """Every refused argument: its code and what bsgpu_register_scans_error then says; nothing is written."""
    fn, capi, gpu = _raw()
    RE, RS, TE, TS = (np.ascontiguousarray(c) for c in ref.scene(*ref.SMALL))
    two = lambda a: np.concatenate([a, a])
    st2 = lambda a: [0, len(a), 2 * len(a)]

    def refused(code, message, **over):
        kw = dict(ref_edge_start=st2(RE), ref_edges=two(RE), ref_surf_start=st2(RS), ref_surfs=two(RS), tgt_edge_start=st2(TE), tgt_edges=two(TE),
                  tgt_surf_start=st2(TS), tgt_surfs=two(TS), T_init=None, **ref.DEFAULTS)
        kw.update(over)
        with pytest.raises(capi.SolverError) as e:
            gpu.register_scans_loam(**kw)
        assert e.value.code == code and "register_scans_loam: " in str(e.value) and message in str(e.value), (over.keys(), str(e.value))

    inv, uns = capi.ERR_INVALID, capi.ERR_UNSUPPORTED
    for table, cloud, words, pts in (("ref_edge_start", "ref_edges", "reference edge", RE), ("ref_surf_start", "ref_surfs", "reference surface", RS),
                                     ("tgt_edge_start", "tgt_edges", "target edge", TE), ("tgt_surf_start", "tgt_surfs", "target surface", TS)):
        n = len(pts)
        refused(inv, table + "[0] must be 0", **{table: [1, n, 2 * n]})
        refused(inv, table + " must be non-decreasing", **{table: [0, n + 1, n]})
        refused(inv, "names more points than were passed", **{table: [0, n, 2 * n + 1]})
        for bad in (np.nan, np.inf):
            p = two(pts)
            p[n + 3, 1] = bad
            refused(inv, "non-finite " + words + " points", **{cloud: p})
    Ti = np.stack([ref.EYE, ref.EYE])
    Ti[1, 2, 3] = np.nan
    refused(inv, "non-finite T_init", T_init=Ti)
    refused(inv, "array sizes do not agree", T_init=ref.EYE[None])
    for bad in (0.0, np.inf, np.nan):
        refused(inv, "max_corr must be positive and finite", max_corr=bad)
        refused(inv, "grid_cell must be positive and finite", grid_cell=bad)
    refused(inv, "min_measurements must be at least 1", min_measurements=0)
    refused(inv, "max_outer must be at least 1", max_outer=0)
    refused(uns, "max_outer exceeds BSGPU_LOAM_MAX_OUTER", max_outer=capi.LOAM_MAX_OUTER + 1)
    refused(uns, "inner->max_num_iterations exceeds BSGPU_LOAM_MAX_INNER", inner=dict(max_num_iterations=capi.LOAM_MAX_INNER + 1))
    refused(uns, "Levenberg-Marquardt only", inner=dict(trust_region_strategy_type=1))
    for name in ("conv_translation_m", "conv_rotation_deg"):
        for bad in (-1e-3, np.nan):
            refused(inv, "must not be negative or NaN", **{name: bad})
    refused(inv, "conv_rotation_deg must be below 180", conv_rotation_deg=180.0)
    refused(inv, "unknown loss kind", loss_kind=3)
    refused(inv, "unknown loss kind", loss_kind=-1)
    refused(uns, "the Cauchy loss is not supported", loss_kind=capi.LOSS_CAUCHY)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(inv, "loss_a must be positive and finite", loss_a=bad)
    # the feature cap: one pair of 65 537 target features
    many = np.zeros((capi.LOAM_MAX_FEATURES + 1, 3))
    refused(uns, "more than BSGPU_LOAM_MAX_FEATURES target features", tgt_edge_start=[0, 1, len(many)], tgt_edges=many)
    # the cell cap: two points 100 m apart in every axis span 201^3 > 2^22 cells of 0.5 m; 50 m apart they are accepted
    wide = np.array([[0.0, 0.0, 0.0], [100.0, 100.0, 100.0]])
    refused(uns, "a reference cloud's grid exceeds BSGPU_ICP_MAX_CELLS cells", ref_surf_start=[0, len(RS), len(RS) + 2], ref_surfs=np.concatenate([RS, wide]))
    z = np.zeros((0, 3))
    ok = gpu.register_scans_loam([0, 2], wide * 0.5, [0, 0], z, [0, len(TE)], TE, [0, 0], z)
    assert ok["status"][0] == ref.TOO_FEW and ok["n_iters"][0] == 0
    # 17 reference grids of 161^3 cells: each below the cap, together above 16 x the cap
    n = 17
    refused(uns, "the call's grids exceed 16 x BSGPU_ICP_MAX_CELLS cells", ref_edge_start=np.arange(n + 1) * 2, ref_edges=np.tile(wide * 0.8, (n, 1)),
            ref_surf_start=[0] * (n + 1), ref_surfs=z, tgt_edge_start=[0] * (n + 1), tgt_edges=z, tgt_surf_start=[0] * (n + 1), tgt_surfs=z)
    # NULL where an array is needed, a negative count: through the raw entry point; the outputs stay untouched
    dp, ip = capi._dp, capi._ip
    T, st = np.full(12, 7.0), np.full(1, 7, np.int32)
    kw = dict(ref.DEFAULTS, max_corr=1.5)
    args, keep = _raw_args(capi, gpu, [RE, RS, TE, TS], kw, T, st)
    for i, message in ((2, "null argument"), (3, "null or non-finite reference edge points"), (4, "null argument"), (5, "null or non-finite reference surface points"),
                       (6, "null argument"), (7, "null or non-finite target edge points"), (8, "null argument"), (9, "null or non-finite target surface points"),
                       (16, "null argument"), (20, "null argument"), (28, "null argument")):
        bad = list(args)
        bad[i] = ctypes.cast(None, ctypes.POINTER(capi.Options)) if i == 16 else ctypes.cast(None, ip if i in (2, 4, 6, 8, 28) else dp)
        assert fn(*bad) == inv and "register_scans_loam: " + message in gpu.register_scans_error(), (i, gpu.register_scans_error())
    assert fn(0, -1, *args[2:]) == inv
    assert (T == 7.0).all() and st[0] == 7
    assert fn(*args) == 0 and st[0] == ref.TRANSFORM
