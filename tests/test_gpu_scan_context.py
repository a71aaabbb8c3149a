"""bsgpu_scan_context_describe / bsgpu_scan_context_match on the device (k_scan_context.hip) against the NumPy restatement
(tests/scan_context_ref.py) and, bit for bit, against the shared header on the CPU (beam_slam_amd/csrc/scan_context.h through
tests/plan/test_scan_context.cpp); the CPU side of the same checks is tests/test_scan_context.py.

Shapes, the smallest at which the kernels can still go wrong: aggregates of 0, 1, 255, 256, 257 and a chunk + 1 points (sc_bin_kernel:
256 lanes, chunks of kScChunk points), 1 and 3 members, a scan used by two aggregates, every point beyond the radius; sets of 0, 1, 4, 5
and 70 candidates (sc_match_kernel: 4 waves per workgroup; more than one wave of candidates in the selection), K of 0, 1, 10 and above
the set's size, R of 0, 3 and 30, a set without queries, n_sets == 0; one call of several unequal sets and aggregates against the lone
calls; cases without a revisit (-1 for finite distances); descriptors near the ends of the FP64 range; NULL optional outputs; every
refused argument.

Accuracy criterion as on the CPU.  Measured on an MI355X: see test_device_against_restatement.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import scan_context_ref as ref
from test_scan_context import (INC, MATCH_CASES, MOTIONS, _compile, aggregate_cases, check_match, comparable, describe_command, extreme_sets,
                               match_case, match_command, parse_describe, parse_match, run_program)

pytestmark = pytest.mark.gpu

CHUNK = int(re.search(r"constexpr int kScChunk = (\d+);", open(os.path.join(INC, "scan_context.h")).read()).group(1))


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"], "test_scan_context")


def _describe(scans, aggregates, lidar_height=ref.LIDAR_HEIGHT, max_radius=ref.MAX_RADIUS):
    """scans: list of (n, 3); aggregates: list of lists of (scan index, T or None) -> gpu.scan_context_describe's dict."""
    from beam_slam_amd import gpu
    members = [m for a in aggregates for m in a]
    has_T = any(T is not None for _, T in members)
    ss = np.cumsum([0] + [len(s) for s in scans])
    ms = np.cumsum([0] + [len(a) for a in aggregates])
    pts = np.concatenate([np.asarray(s, float).reshape(-1, 3) for s in scans]) if scans else np.zeros((0, 3))
    mT = np.stack([ref.EYE if T is None else np.asarray(T, float) for _, T in members]) if has_T else None
    return gpu.scan_context_describe(ss, pts, ms, np.array([k for k, _ in members], np.int32), mT, lidar_height, max_radius)


def _match(sets, n_tree_candidates=10, search_ratio=0.1, dist_thres=0.3):
    """sets: list of (query descriptors, candidate descriptors) -> gpu.scan_context_match's dict (flat arrays, as parse_match's)."""
    from beam_slam_amd import gpu
    qs = np.cumsum([0] + [len(q) for q, _ in sets])
    cs = np.cumsum([0] + [len(c) for _, c in sets])
    cat = lambda xs: np.concatenate([np.asarray(x, float).reshape(-1, ref.RINGS, ref.SECTORS) for x in xs]) if xs else np.zeros((0, ref.RINGS, ref.SECTORS))
    return gpu.scan_context_match(qs, cat([q for q, _ in sets]), cs, cat([c for _, c in sets]), n_tree_candidates, search_ratio, dist_thres)


def _same_describe(a, b, what, rows=None):
    rows = slice(None) if rows is None else rows
    for k in ("n_binned", "desc", "ring_key", "sector_key"):
        x, y = np.ascontiguousarray(a[k][rows]), np.ascontiguousarray(b[k])
        assert x.tobytes() == y.tobytes(), (what, k, np.abs(x.astype(float) - y.astype(float)).max())


def _same_match(a, b, what):
    for k in ("best_cand", "best_dist", "best_shift", "yaw", "dist_all", "shift_all"):
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (what, k, a[k], b[k])


def _shape_scans():
    """Scans of 0, 1, 255, 256, 257 and a chunk + 1 points, one whose every point lies beyond the radius, and a plain one."""
    long = np.concatenate([np.array(ref.scan("A")), np.array(ref.scan("A_far"))])
    assert len(long) > CHUNK + 1
    A = np.array(ref.scan("A"))
    return [A[:0], A[:1], A[:255], A[:256], A[:257], long[:CHUNK + 1], A * 100.0, np.array(ref.scan("B"))]


def _shape_aggregates():
    """One member each for the eight scans; three members (the chunk + 1 scan among them, scan 7 used by two aggregates); no member; a
    member with an empty scan beside a full one."""
    return [[(k, MOTIONS[k % 3])] for k in range(8)] + [[(7, MOTIONS[0]), (5, MOTIONS[1]), (4, MOTIONS[2])], [], [(0, MOTIONS[0]), (7, MOTIONS[2])]]


@pytest.fixture(scope="module")
def many():
    """70 descriptors (the five views through 14 planar motions each) from the restatement: inputs of the match tests."""
    rng = np.random.default_rng(5)
    scans = [ref.scan(n) for n in ref.VIEWS]
    aggs = [[(k % 5, np.hstack([ref.rotz(rng.uniform(0, 360)), [[rng.uniform(-1, 1)], [rng.uniform(-1, 1)], [0.0]]]))] for k in range(70)]
    return ref.describe(scans, aggs)["desc"]


# ---- against the restatement -------------------------------------------------------------------------------------------------------------
def test_device_against_restatement():
    """describe: the five views (identity members) and three aggregates of three members; match: A against (A revisited, A from afar,
    B, C) at the shipped parameters, without pre-selection, with K = 2 and with the full window, and the three cases without a revisit
    (test_scan_context.MATCH_CASES), whose every query must come back -1 with the restatement's finite best_dist and its best_shift.  Measured on an MI355X (2026-10-20),
    difference / bound — the header's figures (tests/test_scan_context.py), since the device returns the header's bits: ring_key 0.125
    at most, sector_key 0, dist_all 0.125 at most, best_dist 0, yaw 0.64 (its bound is the 2^-52 floor)."""
    names = list(ref.VIEWS)
    scans, aggs = aggregate_cases()
    agg_T = [[(k, ref.EYE if T is None else T) for k, T in a] for a in aggs]
    for want, got, who in ((comparable(ref.descriptors()), _describe(scans, [[(k, None)] for k in range(len(names))]), "identity"),
                           (comparable(ref.describe(scans, agg_T)), _describe(scans, agg_T), "three members")):
        assert (got["n_binned"] == want["n_binned"]).all(), who
        assert got["desc"].tobytes() == want["desc"].tobytes(), (who, np.abs(got["desc"] - want["desc"]).max())
        for a in range(len(want["desc"])):
            rk, sk = ref.keys(want["desc"][a][::-1, ::-1])
            ref.check(got["ring_key"][a], want["ring_key"][a], rk[::-1], f"kernel {who} ring_key {a}")
            ref.check(got["sector_key"][a], want["sector_key"][a], sk[::-1], f"kernel {who} sector_key {a}")
    for name in MATCH_CASES:
        q, c, kw, res, rev = match_case(name)
        got = _match([(q, c)], **kw)
        check_match(got, res, rev, f"kernel {name}")
        if name.startswith("none"):      # no revisit among the candidates: -1 for finite distances, best_dist and best_shift still the restatement's
            assert (got["best_cand"] == -1).all() and (got["best_shift"] == res["best_shift"]).all() and np.isfinite(got["best_dist"]).all()
        else:
            assert got["best_cand"][0] == 0 and got["best_shift"][0] in (15, 16)


# ---- bit for bit against the header ------------------------------------------------------------------------------------------------------
def test_describe_equals_header_bit_for_bit(core, tmp_path):
    """Every shape in one call: the device's descriptors, keys and n_binned are the header's bits, and every aggregate returns the bits
    of its lone call."""
    scans, aggs = _shape_scans(), _shape_aggregates()
    together = _describe(scans, aggs)
    want = parse_describe(run_program(core, [describe_command(scans, aggs)], tmp_path)[0], len(aggs))
    _same_describe(together, want, "whole call")
    assert list(together["n_binned"][:6]) == [0, 1, 255, 256, 257, CHUNK + 1] and together["n_binned"][6] == 0 and not together["desc"][6].any()
    assert together["n_binned"][8] == 4000 + CHUNK + 1 + 257 and together["n_binned"][9] == 0 and not together["desc"][9].any()
    for a, members in enumerate(aggs):
        used = sorted({k for k, _ in members})
        lone = _describe([scans[k] for k in used], [[(used.index(k), T) for k, T in members]])
        _same_describe(together, lone, f"aggregate {a}", rows=slice(a, a + 1))


def test_describe_identity_members_and_shared_scan(core, tmp_path):
    """member_T NULL: every member the identity; one scan used by two aggregates; no scans at all."""
    A = np.array(ref.scan("A"))
    scans, aggs = [A, A[:300]], [[(0, None)], [(0, None), (1, None)], [(1, None)]]
    got = _describe(scans, aggs)
    _same_describe(got, parse_describe(run_program(core, [describe_command(scans, aggs)], tmp_path)[0], 3), "identity")
    assert got["desc"][0].tobytes() == got["desc"][1].tobytes() == ref.descriptors()["desc"][0].tobytes() and got["n_binned"][1] == 4300
    none = _describe([], [[], []])
    assert none["desc"].shape == (2, 20, 60) and not none["desc"].any() and not none["n_binned"].any()
    assert _describe([A], [])["desc"].shape == (0, 20, 60)


@pytest.mark.parametrize("K,ratio", [(0, 0.1), (1, 0.1), (10, 0.0), (10, 1.0), (64, 0.1)], ids=["K0_R3", "K1_R3", "K10_R0", "K10_R30", "K64_R3"])
def test_match_equals_header_bit_for_bit(K, ratio, many, core, tmp_path):
    """Sets of 0, 1, 4, 5 and 70 candidates and a set without queries in one call: every dist_all / shift_all entry and every result
    is the header's bits, and every set returns the bits of its lone call."""
    D = ref.descriptors()["desc"]
    sets = [(D[[0, 3]], many[:0]), (D[[0]], many[[7]]), (D[[1, 4]], many[10:14]), (D[[2]], many[20:25]), (np.concatenate([D[[0, 3]], many[[33]]]), many),
            (D[:0], many[:3])]
    together = _match(sets, K, ratio, 0.3)
    _same_match(together, parse_match(run_program(core, [match_command(sets, K, ratio, 0.3)], tmp_path)[0]), "whole call")
    assert (together["best_cand"][:2] == -1).all() and np.isinf(together["best_dist"][:2]).all() and (together["best_shift"][:2] == 0).all()
    if 0 < K < 70:
        assert (np.isfinite(together["dist_all"][-3 * 70:]).reshape(3, 70).sum(axis=1) == K).all()
    assert together["best_cand"][-1] == 33
    q0 = p0 = 0
    for s, (q, c) in enumerate(sets):
        lone = _match([(q, c)], K, ratio, 0.3)
        part = dict({k: together[k][q0:q0 + len(q)] for k in ("best_cand", "best_dist", "best_shift", "yaw")},
                    **{k: together[k][p0:p0 + len(q) * len(c)] for k in ("dist_all", "shift_all")})
        _same_match(part, lone, f"set {s}")
        q0, p0 = q0 + len(q), p0 + len(q) * len(c)


@pytest.mark.parametrize("K", [0, 2, 3, 5])
def test_nan_counts_as_infinity(K, core, tmp_path):
    """Finite descriptors scaled to 1e306, 1e-162 and 1e-170 among plain ones (test_scan_context.extreme_sets), where ring-key distances,
    alignment norms and cosines overflow or lose their norms: device and header order them alike, so the pre-selection takes the same K
    candidates and every entry is the header's bits."""
    sets = extreme_sets()
    got = _match(sets, K, 0.1, 0.3)
    _same_match(got, parse_match(run_program(core, [match_command(sets, K, 0.1, 0.3)], tmp_path)[0]), K)
    assert not np.isnan(got["dist_all"]).any()


def test_no_sets_and_no_queries(many):
    out = _match([])
    assert out["best_cand"].shape == (0,) and out["dist_all"].shape == (0,)
    out = _match([(many[:0], many[:5])])
    assert out["best_cand"].shape == (0,) and out["dist_all"].shape == (0,)


# ---- the C-ABI's edges -------------------------------------------------------------------------------------------------------------------
def _raw():
    from beam_slam_amd import capi, gpu
    fd, fm = gpu.lib().bsgpu_scan_context_describe, gpu.lib().bsgpu_scan_context_match
    fd.argtypes, fm.argtypes = capi.SCAN_CONTEXT_DESCRIBE_ARGTYPES, capi.SCAN_CONTEXT_MATCH_ARGTYPES
    return fd, fm, capi, gpu


def test_optional_outputs_may_be_null():
    fd, fm, capi, gpu = _raw()
    dp, ip = capi._dp, capi._ip
    d = lambda x: x.ctypes.data_as(dp)
    i = lambda x: x.ctypes.data_as(ip)
    null_d, null_i = ctypes.cast(None, dp), ctypes.cast(None, ip)
    A = np.ascontiguousarray(ref.scan("A"))
    ss, ms, mscan = np.array([0, 4000], np.int32), np.array([0, 1], np.int32), np.array([0], np.int32)
    desc = np.zeros((1, 20, 60))
    assert fd(0, 1, i(ss), d(A), 1, i(ms), i(mscan), null_d, ref.LIDAR_HEIGHT, ref.MAX_RADIUS, d(desc), null_d, null_d, null_i) == 0
    assert desc.tobytes() == ref.descriptors()["desc"][[0]].tobytes()
    D = np.ascontiguousarray(ref.descriptors()["desc"])
    full = _match([(D[[0]], D[1:])])
    one = np.array([0, 1], np.int32)
    four = np.array([0, 4], np.int32)
    bc, bd, bs = np.zeros(1, np.int32), np.zeros(1), np.zeros(1, np.int32)
    assert fm(0, 1, i(one), d(D), i(four), d(D[1:]), 10, 0.1, 0.3, i(bc), d(bd), i(bs), null_d, null_d, null_i) == 0
    assert (bc[0], bd[0], bs[0]) == (full["best_cand"][0], full["best_dist"][0], full["best_shift"][0])


def test_argument_errors(many):
    """Every refused argument: its code and what bsgpu_scan_context_error then says; nothing is written."""
    fd, fm, capi, gpu = _raw()
    inv, uns = capi.ERR_INVALID, capi.ERR_UNSUPPORTED
    A = np.array(ref.scan("A"))
    two = np.concatenate([A, A])

    def refused(fn, base, code, message, **over):
        kw = dict(base, **over)
        with pytest.raises(capi.SolverError) as e:
            fn(**kw)
        assert e.value.code == code and message in str(e.value), (over.keys(), str(e.value))

    base = dict(scan_start=[0, 4000, 8000], points=two, member_start=[0, 1, 3], member_scan=[0, 1, 0], member_T=None, lidar_height=2.0, max_radius=40.0)
    dref = lambda code, message, **over: refused(gpu.scan_context_describe, base, code, message, **over)
    dref(inv, "scan_start[0] must be 0", scan_start=[1, 4000, 8000])
    dref(inv, "scan_start must be non-decreasing", scan_start=[0, 5000, 4000])
    dref(inv, "member_start[0] must be 0", member_start=[1, 1, 3])
    dref(inv, "member_start must be non-decreasing", member_start=[0, 3, 2])
    dref(inv, "name more entries than were passed", scan_start=[0, 4000, 8001])
    dref(inv, "a member index out of range", member_scan=[0, 2, 0])
    dref(inv, "a member index out of range", member_scan=[0, -1, 0])
    for bad in (np.nan, np.inf):
        pts = two.copy()
        pts[4100, 2] = bad
        dref(inv, "non-finite points", points=pts)
        T = np.stack([ref.EYE] * 3)
        T[2, 1, 3] = bad
        dref(inv, "non-finite member_T", member_T=T)
        dref(inv, "max_radius must be positive and finite", max_radius=bad)
        dref(inv, "lidar_height must be finite", lidar_height=bad)
    dref(inv, "max_radius must be positive and finite", max_radius=0.0)
    dref(inv, "max_radius must be positive and finite", max_radius=-1.0)
    dref(inv, "array sizes do not agree", member_T=ref.EYE[None])
    # a scan of more than BSGPU_SC_MAX_SCAN_POINTS points: refused from the start table, before a point is read (raw entry point below)

    D = np.ascontiguousarray(ref.descriptors()["desc"])
    mbase = dict(query_start=[0, 1, 2], query_desc=D[:2], cand_start=[0, 2, 3], cand_desc=D[2:], n_tree_candidates=10, search_ratio=0.1, dist_thres=0.3)
    mref = lambda code, message, **over: refused(gpu.scan_context_match, mbase, code, message, **over)
    mref(inv, "query_start[0] must be 0", query_start=[1, 1, 2])
    mref(inv, "query_start must be non-decreasing", query_start=[0, 2, 1])
    mref(inv, "cand_start[0] must be 0", cand_start=[1, 2, 3])
    mref(inv, "cand_start must be non-decreasing", cand_start=[0, 3, 2])
    mref(inv, "name more descriptors than were passed", cand_start=[0, 2, 4])
    mref(inv, "array sizes do not agree", cand_start=[0, 3])
    for bad in (np.nan, np.inf):
        q = D[:2].copy()
        q[1, 3, 5] = bad
        mref(inv, "non-finite query descriptors", query_desc=q)
        c = D[2:].copy()
        c[2, 19, 59] = bad
        mref(inv, "non-finite candidate descriptors", cand_desc=c)
    mref(inv, "search_ratio must not be negative or NaN", search_ratio=-0.1)
    mref(inv, "search_ratio must not be negative or NaN", search_ratio=np.nan)
    mref(inv, "dist_thres must not be negative or NaN", dist_thres=-1e-9)
    mref(inv, "dist_thres must not be negative or NaN", dist_thres=np.nan)
    mref(uns, "n_tree_candidates exceeds BSGPU_SC_MAX_TREE_CANDIDATES", n_tree_candidates=65)
    # more than 65 536 candidates in a set: refused from the start table, before a descriptor is read (through the raw entry point:
    # the Python side checks the sizes first)
    dp, ip = capi._dp, capi._ip
    d = lambda x: x.ctypes.data_as(dp)
    i = lambda x: x.ctypes.data_as(ip)
    null_d, null_i = ctypes.cast(None, dp), ctypes.cast(None, ip)
    bc, bd, bs = np.full(1, 7, np.int32), np.full(1, 7.0), np.full(1, 7, np.int32)
    one, big = np.array([0, 1], np.int32), np.array([0, capi.SC_MAX_CANDIDATES + 1], np.int32)
    margs = [0, 1, i(one), d(D), i(big), d(D), 10, 0.1, 0.3, i(bc), d(bd), i(bs), null_d, null_d, null_i]
    assert fm(*margs) == uns and "more than BSGPU_SC_MAX_CANDIDATES candidates" in gpu.scan_context_error()
    # NULL where an array is needed, a negative count; the outputs stay untouched
    four = np.array([0, 4], np.int32)
    margs[4], margs[5] = i(four), d(D[1:])
    for k, message in ((2, "null argument"), (3, "null or non-finite query descriptors"), (4, "null argument"), (5, "null or non-finite candidate descriptors"),
                       (9, "null argument"), (10, "null argument"), (11, "null argument")):
        bad = list(margs)
        bad[k] = null_i if k in (2, 4, 9, 11) else null_d
        assert fm(*bad) == inv and message in gpu.scan_context_error(), k
    assert fm(0, -1, *margs[2:]) == inv
    assert bc[0] == 7 and bd[0] == 7.0 and bs[0] == 7
    assert fm(*margs) == 0 and bc[0] == 0

    Ac = np.ascontiguousarray(A)
    ss, ms, mscan = np.array([0, 4000], np.int32), np.array([0, 1], np.int32), np.array([0], np.int32)
    desc, nb = np.full((1, 20, 60), 7.0), np.full(1, 7, np.int32)
    dargs = [0, 1, i(ss), d(Ac), 1, i(ms), i(mscan), null_d, 2.0, 40.0, d(desc), null_d, null_d, i(nb)]
    for k, message in ((2, "null argument"), (3, "null or non-finite points"), (5, "null argument"), (6, "null member_scan"), (10, "null argument")):
        bad = list(dargs)
        bad[k] = null_i if k in (2, 5, 6) else null_d
        assert fd(*bad) == inv and message in gpu.scan_context_error(), k
    assert fd(0, -1, *dargs[2:]) == inv and fd(0, 1, i(ss), d(Ac), -1, *dargs[5:]) == inv
    long = list(dargs)
    long[2] = i(np.array([0, capi.SC_MAX_SCAN_POINTS + 1], np.int32))
    assert fd(*long) == uns and "more than BSGPU_SC_MAX_SCAN_POINTS points" in gpu.scan_context_error()
    assert (desc == 7.0).all() and nb[0] == 7
    assert fd(*dargs) == 0 and nb[0] == 4000 and desc.tobytes() == ref.descriptors()["desc"][[0]].tobytes()
