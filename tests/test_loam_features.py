"""bsgpu_extract_loam_features on the CPU: beam_slam_amd/csrc/loam_features.h (through tests/plan/test_loam_features.cpp: the rules of
the contract and loam_extract_serial, one scan on one core) against the NumPy restatement (tests/loam_features_ref.py: Python loops per
ring, numpy.lexsort, numpy.arctan2 for the ring, other orders of the curvature's sum).

Cases (CASES): the reference's own VLP-16 test scan (tests/golden/vlp16_scan.cloud) with its ring field at the shipped parameters
(loam_vlp16.json) and at loam_vlp16_init.json's, and by elevation at fov_deg 20 (its beams sit at +-10 degrees: at the shipped 30 they
fall on ring boundaries); box scenes of 4 x 240, 16 x 360 and, along vertical_axis X, 8 x 300 returns, by elevation.  Before anything is
compared every case asserts that its input can be compared: all margins of loam_features_ref exceed 1e-9.

Exact fixtures (exact_fixtures): rings on a line at y = 32 with x in steps of 1/8 and z in eighths, so that every sum is exact and ties are
real; two of them carry one step whose squared gap is 0.05, or 0.1, to the bit.

Criterion: labels and all four index lists equal; curvature within 8 x the restatement's own spread between its two orders of summation,
and not below 2^-52 of the largest value (test_loam.py's criterion).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import loam_features_ref as ref
from test_icp import run_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plan", "test_loam_features.cpp")
INC = os.path.join(ROOT, "beam_slam_amd", "csrc")
LISTS = ("sharp", "less_sharp", "flat", "less_flat")
PARAM_ORDER = ("number_of_beams", "fov_deg", "vertical_axis", "n_feature_regions", "curvature_region", "max_corner_sharp", "max_corner_less_sharp",
               "max_surface_flat", "surface_curvature_threshold")


def feat_command(points, ring=None, **params):
    P = dict(ref.DEFAULTS, **params)
    points = np.asarray(points, float).reshape(-1, 3)
    head = [1, len(points), 0 if ring is None else 1] + [P[k] for k in PARAM_ORDER]
    return np.concatenate([np.array(head, float), points.ravel(), np.zeros(0) if ring is None else np.asarray(ring, float).ravel()])


def parse_feat(tok, n):
    """The driver's line -> dict(ok, the four lists, label, curvature); ok 0: a ring above the cap"""
    if tok[2] == "0":
        return dict(ok=0)
    counts = [int(t) for t in tok[3:7]]
    at, out = 7, dict(ok=1)
    for name, k in zip(LISTS, counts):
        out[name] = [int(t) for t in tok[at:at + k]]
        at += k
    out["label"] = np.array([int(t) for t in tok[at:at + n]], int)
    out["curvature"] = np.array([int(t, 16) for t in tok[at + n:at + 2 * n]], np.uint64).view(np.float64)
    assert len(tok) == at + 2 * n
    return out


def _compile(tmp_path_factory, flags, name):
    exe = str(tmp_path_factory.mktemp("loam_features") / name)
    # -ffp-contract=off: the header's pragma is clang's; GCC gets the same rule from the command line (loam_features.h, "Bits")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", INC, SRC, "-o", exe] + flags, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"], "test_loam_features")


def header(core, tmp_path, runs):
    """runs: [(points, ring, params)] -> the header's results"""
    rows = run_program(core, [feat_command(p, r, **kw) for p, r, kw in runs], tmp_path)
    return [parse_feat(tok, len(np.asarray(p).reshape(-1, 3))) for tok, (p, r, kw) in zip(rows, runs)]


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------
def case(name):
    """(points, ring or None, parameters)"""
    if name.startswith("fixture"):
        pts, ring = ref.fixture()
        return {"fixture_shipped": (pts, ring, {}), "fixture_init": (pts, ring, {k: ref.INIT[k] for k in ("n_feature_regions", "curvature_region", "max_corner_less_sharp")}),
                "fixture_elevation": (pts, None, dict(fov_deg=20.0))}[name]
    rings, azimuths, axis = {"box_4x240": (4, 240, 2), "box_16x360": (16, 360, 2), "box_axis_x": (8, 300, 0)}[name]
    pts, _ = ref.box_scene(rings, azimuths, axis=axis)
    return pts, None, dict(number_of_beams=rings, vertical_axis=axis)


CASES = ("fixture_shipped", "fixture_init", "fixture_elevation", "box_4x240", "box_16x360", "box_axis_x")


def line_ring(z_eighths, y=32.0):
    """A ring on a line: x in steps of 1/8 about 0, y constant, z in eighths.  Gaps of 1/64 + dz^2: no jump for |dz| <= 1/4, marks pass
    for |dz| <= 1/8; 0.0002 |p|^2 >= 0.2 is above every gap, so no point is unreliable."""
    z = np.asarray(z_eighths, float) / 8.0
    m = len(z)
    return np.stack([(np.arange(m) - m // 2) / 8.0, np.full(m, y), z], axis=1)


def spikes(m, at):
    z = np.zeros(m)
    z[list(at)] = 1.0
    return z


def _step(total):
    """d with (1/64 + 0) + d d == total to the bit, and the next double above it"""
    d = np.sqrt(total - 1.0 / 64.0)
    for _ in range(64):
        got = (1.0 / 64.0 + 0.0) + d * d
        if got == total:
            up = d
            while (1.0 / 64.0 + 0.0) + up * up == total:
                up = np.nextafter(up, 1.0)
            return float(d), float(up)
        d = np.nextafter(d, 0.0 if got > total else 1.0)
    raise AssertionError("no step gives %r exactly" % total)


def stepped_ring(m, at, d, spike=None):
    """A line ring whose z rises by d between positions at and at + 1 (and stays); spike: a position one eighth higher."""
    R = line_ring(np.zeros(m))
    R[at + 1:, 2] += d
    if spike is not None:
        R[spike, 2] += 1.0 / 8.0
    return R


SMALL = dict(number_of_beams=1, n_feature_regions=1, curvature_region=2, max_corner_sharp=1, max_corner_less_sharp=3, max_surface_flat=2)


def exact_fixtures():
    """{name: (points, ring, parameters)}"""
    out = {}
    zeros = lambda n: np.zeros(n, np.int32)
    two = line_ring(spikes(40, (10, 25)))
    out["ties"] = (two, zeros(40), SMALL)
    out["on_threshold"] = (two, zeros(40), dict(SMALL, surface_curvature_threshold=0.25))
    d05, d05_up = _step(0.05)
    d10, d10_up = _step(0.1)
    out["gap_0.05"] = (stepped_ring(40, 14, d05, spike=16), zeros(40), SMALL)
    out["gap_above_0.05"] = (stepped_ring(40, 14, d05_up, spike=16), zeros(40), SMALL)
    out["gap_0.1"] = (stepped_ring(40, 4, d10), zeros(40), SMALL)
    out["gap_above_0.1"] = (stepped_ring(40, 4, d10_up), zeros(40), SMALL)
    out["across_border"] = (line_ring(spikes(40, (18,))), zeros(40), dict(SMALL, n_feature_regions=2))
    # rings of 2 c + 1 (skipped) and 2 c + 2 points (its one region has one point), next to a ring that is processed, interleaved
    short = np.concatenate([line_ring(np.zeros(5)), line_ring(np.zeros(6)), line_ring(spikes(30, (12,)))])
    ring = np.concatenate([np.full(5, 0), np.full(6, 1), np.full(30, 2)]).astype(np.int32)
    mix = np.random.default_rng(5).permutation(len(short))
    mix = mix[np.argsort(np.arange(len(short))[mix] // 3, kind="stable")]     # (shuffled within triples: every ring keeps arriving throughout)
    out["short_rings"] = (short[mix], ring[mix], dict(SMALL, number_of_beams=3))
    # L = 5 over 4 regions: three regions of one point (skipped), one of exactly two
    out["tiny_regions"] = (line_ring(spikes(10, (6,))), zeros(10), dict(SMALL, n_feature_regions=4))
    bad = two.copy()
    bad[3] = [np.nan, 32.0, 0.0]; bad[11, 2] = np.inf; bad[20] = [0.0, 0.0, 0.0]; bad[30, 0] = -np.inf; bad[31] = [0.0, 0.009, 0.0]
    out["invalid_points"] = (bad, zeros(40), SMALL)
    r = zeros(40)
    r[[5, 17]] = -1; r[[6, 29]] = 2
    out["ring_out_of_range"] = (two, r, dict(SMALL, number_of_beams=2))
    out["sharp_above_less_sharp"] = (two, zeros(40), dict(SMALL, max_corner_sharp=5, max_corner_less_sharp=1))
    out["all_counts_zero"] = (two, zeros(40), dict(SMALL, max_corner_sharp=0, max_corner_less_sharp=0, max_surface_flat=0))
    return out


def same_selections(got, res, what):
    assert got["ok"] == 1, what
    for k in LISTS:
        assert got[k] == res[k], (what, k, got[k][:12], res[k][:12])
    assert (got["label"] == res["label"]).all(), (what, np.flatnonzero(got["label"] != res["label"])[:12])


# ---- the header against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_header_against_restatement(name, core, tmp_path):
    """Measured (CPU build, g++ -O2), per case: SHARP / LESS_SHARP / FLAT / LESS_FLAT, the smallest margin and its kind, the largest
    curvature difference over its bound:
        fixture_shipped    176 / 906 / 384 / 24118   1.2e-6 parallel   0.00
        fixture_init        92 / 538 / 192 / 24826   7.5e-8 curv_gap   0.00
        fixture_elevation  176 / 906 / 384 / 24118   1.2e-6 parallel   0.00
        box_4x240           11 /   0 /  95 /   810   1.8e-4 curv_gap   0.32
        box_16x360          27 /   1 / 384 /  5172   2.7e-7 curv_gap   0.11
        box_axis_x          14 /   0 / 192 /  2106   6.5e-6 curv_gap   0.15
    (the fixture's coordinates are float32 values, whose sums of 11 are exact in FP64: every order gives the same curvature)
    """
    pts, ring, kw = case(name)
    res = ref.extract(pts, ring, **kw)
    worst = min(ref.KINDS, key=lambda k: res["margins"][k])
    assert ref.comparable(res), (name, res["margins"])
    got = header(core, tmp_path, [(pts, ring, kw)])[0]
    same_selections(got, res, name)
    have = ~np.isnan(res["curvature"])
    assert (np.isnan(got["curvature"]) == ~have).all()
    diff, bound = float(np.abs(got["curvature"][have] - res["curvature"][have]).max()), ref.curvature_bound(res)
    print(f"{name}: {len(res['sharp'])} / {len(res['less_sharp'])} / {len(res['flat'])} / {len(res['less_flat'])}, smallest margin {res['margins'][worst]:.2e} "
          f"({worst}), curvature difference / bound {diff / bound:.2f}")
    assert diff <= bound, (name, diff, bound)
    assert len(res["sharp"]) > 0 and len(res["flat"]) > 0 and len(res["less_flat"]) > 0
    if name == "fixture_shipped":      # the figures of the prototype that the contract was written from
        assert (len(res["sharp"]), len(res["less_sharp"]), len(res["flat"])) == (176, 906, 384)
    if name == "fixture_elevation":    # the elevation rule gives the ring field on every point
        assert res["ring_sizes"] == list(np.bincount(ref.fixture()[1], minlength=16)) and res["margins"]["t_integer"] > 0.4


def test_exact_fixtures(core, tmp_path):
    """Ties, the strict comparisons and the edge shapes: the header's selections are the restatement's, and each fixture does what its
    name says."""
    fx = exact_fixtures()
    res = {k: ref.extract(p, r, **kw) for k, (p, r, kw) in fx.items()}
    got = dict(zip(fx, header(core, tmp_path, list(fx.values()))))
    for k in fx:
        same_selections(got[k], res[k], k)
        a, b = got[k]["curvature"], res[k]["curvature"]
        assert (np.isnan(a) == np.isnan(b)).all() and np.abs(a - b)[~np.isnan(a)].max(initial=0.0) <= 1e-14, k
    # equal curvatures: of two equal edges the higher position goes first, of equal surfaces the lower
    assert res["ties"]["margins"]["curv_gap"] == 0.0 and res["ties"]["curvature"][10] == res["ties"]["curvature"][25] == 0.25
    assert res["ties"]["sharp"] == [25] and res["ties"]["less_sharp"] == [10] and res["ties"]["flat"] == [2, 5]
    # a curvature exactly at the threshold is neither an edge nor a surface
    on = res["on_threshold"]
    assert on["margins"]["threshold"] == 0.0 and on["sharp"] == [] and on["less_sharp"] == [] and on["label"][10] == on["label"][25] == ref.LESS_FLAT
    # a squared gap of exactly 0.05 lets the marks pass, the next double stops them: position 14 is then free to be an edge
    assert res["gap_0.05"]["margins"]["mark"] == 0.0 and 0.0 < res["gap_above_0.05"]["margins"]["mark"] < 1e-15
    assert 14 not in res["gap_0.05"]["sharp"] + res["gap_0.05"]["less_sharp"] and 14 in res["gap_above_0.05"]["sharp"] + res["gap_above_0.05"]["less_sharp"]
    # a squared gap of exactly 0.1 is no jump, the next double is one (and marks the farther side, 5 .. 7, as picked)
    assert res["gap_0.1"]["margins"]["jump"] == 0.0 and 0.0 < res["gap_above_0.1"]["margins"]["jump"] < 1e-15
    assert res["gap_0.1"]["label"].tolist() != res["gap_above_0.1"]["label"].tolist()
    # the pick at the last position of region 0 marks the first two of region 1, which therefore are no surfaces
    ab = res["across_border"]
    assert ab["sharp"] == [18] and ab["label"][19] == ab["label"][20] == ref.LESS_FLAT and 21 in ab["flat"] and 2 in ab["flat"]
    sr = res["short_rings"]
    assert sr["ring_sizes"] == [5, 6, 30] and (sr["label"][fx["short_rings"][1] < 2] == ref.DROPPED).all() and len(sr["sharp"]) == 1
    tr = res["tiny_regions"]
    assert (tr["label"] != ref.DROPPED).sum() == 2 and tr["sharp"] == [6]
    iv = res["invalid_points"]
    assert iv["ring_sizes"] == [35] and (iv["label"][[3, 11, 20, 30, 31]] == ref.DROPPED).all() and iv["margins"]["valid"] < 1.0
    ro = res["ring_out_of_range"]
    assert ro["ring_sizes"] == [36, 0] and (ro["label"][[5, 17, 6, 29]] == ref.DROPPED).all()
    sl = res["sharp_above_less_sharp"]
    assert sl["sharp"] == [25] and sl["less_sharp"] == []
    z = res["all_counts_zero"]
    assert z["sharp"] == z["less_sharp"] == z["flat"] == [] and z["less_flat"] == list(range(2, 37))


def test_ring_cap(core, tmp_path):
    """A ring of kLoamMaxRingPoints points is extracted, one more is refused."""
    from beam_slam_amd import capi
    n = capi.LOAM_MAX_RING_POINTS
    ok, over = line_ring(np.arange(n) % 2), line_ring(np.arange(n + 1) % 2)
    a, b = header(core, tmp_path, [(ok, np.zeros(n, np.int32), SMALL), (over, np.zeros(n + 1, np.int32), SMALL)])
    assert a["ok"] == 1 and (a["label"][2:n - 3] != ref.DROPPED).all() and b["ok"] == 0


def test_header_under_sanitizers(tmp_path_factory, tmp_path):
    """The header as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, arrays of exact size: a box
    scene, the exact fixtures, an empty scan and the ring cap run clean."""
    exe = _compile(tmp_path_factory, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "test_loam_features_san")
    runs = [case("box_4x240"), case("box_axis_x")] + list(exact_fixtures().values()) + [(np.zeros((0, 3)), None, {}), (np.zeros((0, 3)), np.zeros(0, np.int32), {})]
    n = 4097
    runs.append((line_ring(np.arange(n) % 2), np.zeros(n, np.int32), SMALL))
    run_program(exe, [feat_command(p, r, **kw) for p, r, kw in runs], tmp_path)


# ---- the entry point's argument checks (they come before the device is touched) ------------------------------------------------------
def test_argument_errors():
    """Every refused argument: its code and what bsgpu_register_scans_error then says."""
    from beam_slam_amd import capi, gpu
    pts, ring = ref.box_scene(4, 240)

    def refused(code, message, **over):
        kw = dict(scan_start=[0, len(pts)], points=pts, ring=ring, number_of_beams=4)
        kw.update(over)
        with pytest.raises(capi.SolverError) as e:
            gpu.extract_loam_features(**kw)
        assert e.value.code == code and "extract_loam_features: " in str(e.value) and message in str(e.value), (over.keys(), str(e.value))

    inv, uns = capi.ERR_INVALID, capi.ERR_UNSUPPORTED
    refused(inv, "scan_start[0] must be 0", scan_start=[1, len(pts)])
    refused(inv, "scan_start must be non-decreasing", scan_start=[0, len(pts), len(pts) - 1])
    refused(inv, "names more points than were passed", scan_start=[0, len(pts) + 1])
    refused(inv, "array sizes do not agree", ring=ring[:-1])
    refused(inv, "number_of_beams must be at least 1", number_of_beams=0)
    refused(inv, "n_feature_regions must be at least 1", n_feature_regions=0)
    refused(inv, "curvature_region must be at least 1", curvature_region=0)
    for name in ("max_corner_sharp", "max_corner_less_sharp", "max_surface_flat"):
        refused(inv, "must not be negative", **{name: -1})
    for bad in (0.0, 180.0, -30.0, np.nan):
        refused(inv, "fov_deg must lie in (0, 180)", fov_deg=bad)
    for bad in (np.nan, np.inf, -np.inf):
        refused(inv, "surface_curvature_threshold must be finite", surface_curvature_threshold=bad)
    for bad in (-1, 3, "W"):
        refused(inv, "unknown vertical_axis", vertical_axis=bad)
    refused(uns, "number_of_beams exceeds BSGPU_LOAM_MAX_RINGS", number_of_beams=capi.LOAM_MAX_RINGS + 1)
    refused(uns, "curvature_region exceeds BSGPU_LOAM_MAX_CURVATURE_REGION", curvature_region=capi.LOAM_MAX_CURVATURE_REGION + 1)
    refused(uns, "n_feature_regions exceeds BSGPU_LOAM_MAX_REGIONS", n_feature_regions=capi.LOAM_MAX_REGIONS + 1)
    refused(uns, "downsample_less_flat_features is not supported", downsample_less_flat_features=1)
    # NULL where an array is needed, a weak group given in part, a negative count: through the raw entry point; nothing is written
    fn = gpu.lib().bsgpu_extract_loam_features
    fn.argtypes = capi.EXTRACT_LOAM_FEATURES_ARGTYPES
    dp, ip = capi._dp, capi._ip
    ss, P = np.array([0, len(pts)], np.int32), capi.LOAM_FEATURE_DEFAULTS
    outs = [np.full(8, 0x5A5A5A5A, np.int32) for _ in range(4)]
    null_d, null_i = ctypes.cast(None, dp), ctypes.cast(None, ip)
    args = [0, 1, ss.ctypes.data_as(ip), pts.ctypes.data_as(dp), null_i, 4, P["fov_deg"], P["vertical_axis"], P["n_feature_regions"], P["curvature_region"],
            P["max_corner_sharp"], P["max_corner_less_sharp"], P["max_surface_flat"], P["surface_curvature_threshold"], 0,
            outs[0].ctypes.data_as(ip), outs[1].ctypes.data_as(ip), null_d, outs[2].ctypes.data_as(ip), outs[3].ctypes.data_as(ip), null_d,
            null_i, null_i, null_d, null_i, null_i, null_d, null_i, null_d]
    for i in (2, 15, 16, 18, 19):
        bad = list(args)
        bad[i] = null_i
        assert fn(*bad) == inv and gpu.register_scans_error() == "extract_loam_features: null argument", i
    bad = list(args)
    bad[3] = null_d
    assert fn(*bad) == inv and gpu.register_scans_error() == "extract_loam_features: null points"
    for i in (21, 22, 24, 25):
        bad = list(args)
        bad[i] = outs[0].ctypes.data_as(ip)
        assert fn(*bad) == inv and "the weak clouds come as a group" in gpu.register_scans_error(), i
    assert fn(0, -1, *args[2:]) == inv
    assert all((o == 0x5A5A5A5A).all() for o in outs)


def test_declared_and_bound():
    """The C-ABI declares the entry point and the Python side binds it with the contract's constants."""
    from beam_slam_amd import capi, gpu
    text = open(os.path.join(ROOT, "include", "bsgpu.h")).read()
    assert "int bsgpu_extract_loam_features(int device, int32_t n_scans" in text and "extract_loam_features" in capi.SYMBOLS
    block = text[text.index("LOAM feature extraction for a batch of scans"):]
    assert "RECALLED" in block and "OUT OF SCOPE" in block and "the library's choice" in block
    head = open(os.path.join(INC, "loam_features.h")).read()
    for name, value, const in (("MAX_RINGS", 128, "kLoamMaxRings"), ("MAX_RING_POINTS", 4096, "kLoamMaxRingPoints"),
                               ("MAX_CURVATURE_REGION", 16, "kLoamMaxCurvatureRegion"), ("MAX_REGIONS", 64, "kLoamMaxRegions")):
        assert getattr(capi, "LOAM_" + name) == value and f"#define BSGPU_LOAM_{name} {value}" in text and f"constexpr int {const} = {value};" in head
    assert (capi.LOAM_DROPPED, capi.LOAM_LESS_FLAT, capi.LOAM_FLAT, capi.LOAM_LESS_SHARP, capi.LOAM_SHARP) == \
        (ref.DROPPED, ref.LESS_FLAT, ref.FLAT, ref.LESS_SHARP, ref.SHARP) == (-1, 0, 1, 2, 3)
    assert "BSGPU_LOAM_DROPPED = -1, BSGPU_LOAM_LESS_FLAT = 0, BSGPU_LOAM_FLAT = 1, BSGPU_LOAM_LESS_SHARP = 2, BSGPU_LOAM_SHARP = 3" in text
    assert capi.LOAM_FEATURE_DEFAULTS == ref.DEFAULTS and len(capi.EXTRACT_LOAM_FEATURES_ARGTYPES) == 29 and callable(gpu.extract_loam_features)
    import json
    shipped = os.path.join(ROOT, "tests", "golden", "loam_vlp16.json")
    keys = json.load(open(shipped))
    axis = {"X": capi.AXIS_X, "Y": capi.AXIS_Y, "Z": capi.AXIS_Z}[keys["vertical_axis"]]
    assert {k: (axis if k == "vertical_axis" else int(keys[k]) if isinstance(keys[k], bool) else keys[k]) for k in ref.DEFAULTS} == ref.DEFAULTS
