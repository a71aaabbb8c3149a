"""bsgpu_build_registration_maps on the device (k_registration_map.hip) against the shared header on the CPU (beam_slam_amd/csrc/
registration_map.h through tests/plan/test_registration_map.cpp).  The device must return the header's bytes: start tables, points,
counts.  The header against the NumPy restatement is tests/test_registration_map.py.

Shapes, with TILE = capi.MAP_SORT_TILE (the keys of one workgroup of the sort): maps of 0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1 and
3 TILE + 1 points whose voxels' runs — 16 points in the lowest voxel, 32 in every other — lie across every wave boundary and every tile
boundary of the sorted order, coordinates not exact, so that a sum taken in another order than the input's gives other bits; one voxel
with a run of 2 TILE; every point its own voxel with mixed signs; five unequal maps in one call against each alone; NaN and infinite
points; the merge; NULL map_count and NULL T_map_scan; the range refusal with pre-filled outputs; the golden-scan cases and exact
fixtures of test_registration_map.py; and extraction, map and registration chained.
"""
import numpy as np
import pytest

import registration_map_ref as ref
from test_registration_map import CASES, PERM, _compile, case, chain_scans, exact_fixtures, header, header_chain, poses, stack_scans

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return _compile(tmp_path_factory, ["-O2"], "test_registration_map")


def _device(run, counts=True):
    from beam_slam_amd import gpu
    ms, ss, pts, T, v = run
    out = gpu.build_registration_maps(ms, ss, pts, T, v, counts=counts)
    return dict(ok=1, start=out["map_start"], points=out["map_points"], count=out.get("map_count"))


def _same(dev, hdr, what):
    """Every output of a call on the device is the header's, byte for byte (NaNs, which only the merge passes on, by position)."""
    assert hdr["ok"] == 1, what
    assert dev["start"].tolist() == hdr["start"].tolist(), (what, dev["start"], hdr["start"])
    if dev["count"] is not None:
        assert dev["count"].tobytes() == hdr["count"].tobytes(), (what, np.flatnonzero(dev["count"] != hdr["count"])[:10])
    a, b = dev["points"], hdr["points"]
    assert (np.isnan(a) == np.isnan(b)).all(), what
    assert np.where(np.isnan(a), 0.0, a).tobytes() == np.where(np.isnan(b), 0.0, b).tobytes(), (what, np.flatnonzero((a != b).any(axis=1))[:10])


def runs_cloud(n, seed, v=0.1):
    """n points in voxels of leaf v, shuffled: 16 in the voxel with the lowest key, 32 in each of the others (the one with the highest key takes the
    rest), at scattered cells of both signs; inside a voxel the coordinates are uniform, so sums are not exact.  In sorted order a run then
    starts at 16 + 32 j: every multiple of 64, and so every wave and tile boundary of the sort, lies inside a run."""
    rng = np.random.default_rng(seed)
    sizes = [min(16, n)] + [32] * ((max(n - 16, 0) + 31) // 32)
    sizes[-1] -= sum(sizes) - n
    J = len(sizes)
    cells = np.stack([(np.arange(J) * 37) % 1001 - 500, (np.arange(J) * 11) % 301 - 150, np.arange(J) % 7 - 3], axis=1).astype(float)
    cells[0], cells[-1] = [0.0, 0.0, -100.0], [0.0, 0.0, 100.0 if J > 1 else -100.0]      # the lowest key; the rest has the highest
    pts = np.concatenate([(c + rng.uniform(0.1, 0.9, (k, 3))) * v for c, k in zip(cells, sizes)]) if n else np.zeros((0, 3))
    return pts[rng.permutation(n)], sizes


def _tile():
    from beam_slam_amd import capi
    return capi.MAP_SORT_TILE


@pytest.mark.parametrize("shape", ["0", "1", "63", "64", "65", "TILE-1", "TILE", "TILE+1", "3*TILE+1"])
def test_tile_and_wave_boundaries(shape, core, tmp_path):
    TILE = _tile()
    n = eval(shape, dict(TILE=TILE))
    pts, sizes = runs_cloud(n, 100 + n)
    # two scans under two transforms, so that the input order is (scan, point)
    run = stack_scans([[pts[:n // 3], pts[n // 3:]]]) + (np.stack([poses(1)[0], poses(2)[1]]), 0.1)
    hdr = header(core, tmp_path, [run])[0]
    _same(_device(run), hdr, shape)
    # and untransformed, where the runs are the generator's: across every multiple of 64 of the sorted order
    run = stack_scans([[pts]]) + (None, 0.1)
    hdr = header(core, tmp_path, [run])[0]
    assert sorted(hdr["count"].tolist()) == sorted(k for k in sizes if k) and hdr["count"].tolist()[:1] == sizes[:1] * (n > 0)
    ends = np.cumsum(hdr["count"])
    assert not set(ends[:-1].tolist()) & set(range(64, n, 64))      # (TILE is a multiple of 64)
    _same(_device(run), hdr, (shape, "untransformed"))


def test_one_voxel_and_own_voxels(core, tmp_path):
    TILE = _tile()
    rng = np.random.default_rng(21)
    one = stack_scans([[(np.array([-3.0, 7.0, -1.0]) + rng.uniform(0.1, 0.9, (2 * TILE, 3))) * 0.1]]) + (None, 0.1)
    n = TILE + 7
    cells = np.stack([np.arange(n) % 29 - 14, (np.arange(n) // 29) % 13 - 6, np.arange(n) // (29 * 13) - 1], axis=1).astype(float)
    own = stack_scans([[((cells + rng.uniform(0.1, 0.9, (n, 3))) * 0.1)[rng.permutation(n)]]]) + (None, 0.1)
    hdrs = header(core, tmp_path, [one, own])
    assert hdrs[0]["count"].tolist() == [2 * TILE] and (hdrs[1]["count"] == 1).all() and len(hdrs[1]["count"]) == n
    assert (hdrs[1]["points"] < 0).any() and (hdrs[1]["points"] > 0).any()
    _same(_device(one), hdrs[0], "one voxel")
    _same(_device(own), hdrs[1], "own voxels")


def _split(run, m):
    """map m of a run as a call of its own"""
    ms, ss, pts, T, v = run
    a, b = int(ms[m]), int(ms[m + 1])
    return (np.array([0, b - a], np.int32), (ss[a:b + 1] - ss[a]).astype(np.int32), pts[ss[a]:ss[b]], None if T is None else T[a:b], v)


def test_batch_equals_lone_calls(core, tmp_path):
    """Five unequal maps in one call, an empty one among them: each has the bytes of its lone call, which are the header's."""
    TILE = _tile()
    sizes = [700, 1, 0, 2 * TILE + 452, TILE + 300]
    clouds = [runs_cloud(n, 40 + k)[0] for k, n in enumerate(sizes)]
    T = np.stack([poses(5)[k] for k in (0, 3, 1, 4, 2, 0)])
    run = stack_scans([[clouds[0][:300], clouds[0][300:]], [clouds[1]], [clouds[2]], [clouds[3]], [clouds[4]]]) + (T, 0.1)
    together, hdr = _device(run), header(core, tmp_path, [run])[0]
    _same(together, hdr, "batch")
    lone = header(core, tmp_path, [_split(run, m) for m in range(5)])
    for m in range(5):
        alone = _device(_split(run, m))
        _same(alone, lone[m], (m, "alone"))
        a, b = together["start"][m], together["start"][m + 1]
        assert together["points"][a:b].tobytes() == alone["points"].tobytes() and together["count"][a:b].tobytes() == alone["count"].tobytes(), m


def test_dropped_points_merge_and_optional_arguments(core, tmp_path):
    TILE = _tile()
    pts, _ = runs_cloud(TILE + 100, 7)
    pts = pts.copy()
    pts[[0, 63, 64, 500, TILE - 1, TILE, TILE + 99], [0, 1, 2, 0, 1, 2, 0]] = [np.nan, np.inf, -np.inf, np.nan, np.nan, np.inf, np.nan]
    T = np.stack([poses(2)[1], PERM])
    with_T, without = stack_scans([[pts[:400], pts[400:]]]) + (T, 0.1), stack_scans([[pts[:400], pts[400:]]]) + (None, 0.1)
    merged, merged_plain = with_T[:4] + (ref.MERGE_ONLY,), without[:4] + (ref.MERGE_ONLY,)
    hdrs = header(core, tmp_path, [with_T, without, merged, merged_plain])
    assert hdrs[0]["count"].sum() == hdrs[1]["count"].sum() == TILE + 100 - 7 and hdrs[2]["start"].tolist() == [0, TILE + 100]
    for run, hdr, what in zip((with_T, without, merged, merged_plain), hdrs, ("dropped", "dropped, no T", "merge", "merge, no T")):
        _same(_device(run), hdr, what)
        _same(_device(run, counts=False), hdr, (what, "no counts"))


def test_range_refusal_leaves_outputs_alone():
    """A finite coordinate with |q / v| = 2^20 is UNSUPPORTED — the device's flag —, and nothing is written; one cell below is accepted."""
    from beam_slam_amd import capi, gpu
    fn = gpu.lib().bsgpu_build_registration_maps
    fn.argtypes = capi.BUILD_REGISTRATION_MAPS_ARGTYPES
    pts, _ = runs_cloud(300, 9)
    pts = pts.copy()
    pts[123, 1] = -(2.0 ** 20) * 0.1
    ms, ss = np.array([0, 1], np.int32), np.array([0, 300], np.int32)
    outs = [np.full(2, 0x5A5A5A5A, np.int32), np.frombuffer(b"\x5a" * 8 * 900, np.float64).copy(), np.full(300, 0x5A5A5A5A, np.int32)]
    i, d = (lambda a: a.ctypes.data_as(capi._ip)), (lambda a: a.ctypes.data_as(capi._dp))
    rc = fn(0, 1, i(ms), i(ss), d(pts), None, 0.1, i(outs[0]), d(outs[1]), i(outs[2]))
    assert rc == capi.ERR_UNSUPPORTED and gpu.register_scans_error() == "build_registration_maps: a transformed coordinate has |q / voxel_size| >= 2^20"
    assert all((np.frombuffer(o.tobytes(), np.uint8) == 0x5A).all() for o in outs)
    pts[123, 1] = -(2.0 ** 20 - 1.0) * 0.125
    out = gpu.build_registration_maps(ms, ss, pts, None, 0.125)
    assert out["map_points"][:, 1].min() == pts[123, 1] and out["map_count"].sum() == 300


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("golden")])
def test_device_equals_header_on_golden_cases(name, core, tmp_path, tmp_path_factory):
    run = case(name, tmp_path_factory)
    hdr = header(core, tmp_path, [run])[0]
    assert len(hdr["count"]) > 500
    _same(_device(run), hdr, name)


def test_device_equals_header_on_exact_fixtures(core, tmp_path):
    fx = exact_fixtures()
    for (name, run), hdr in zip(fx.items(), header(core, tmp_path, list(fx.values()))):
        _same(_device(run), hdr, name)


def test_extract_map_register(tmp_path, tmp_path_factory):
    """raw scan -> features -> map -> pose: bsgpu_extract_loam_features on the golden scan seen from five poses, this call on the edge
    and surface features at leaf 0.1, bsgpu_register_scans_loam of the sixth scan against the map.  Every step returns the bits of
    loam_extract_serial + registration_map_serial + loam_register_serial; the recovered translation is within half a voxel edge
    (0.05 m) of the true pose's on both sides — a sanity condition (reached: 0.0020 m)."""
    import loam_ref
    from beam_slam_amd import gpu
    from test_gpu_register_scans_loam import _same_bits
    scans, ring, P = chain_scans()
    feats, maps, want = header_chain(tmp_path_factory, tmp_path)
    assert want["ok"] == 1 and want["status"] in (loam_ref.TRANSFORM, loam_ref.MAX_ITERATIONS)
    assert np.linalg.norm(want["T_ref_tgt"][:, 3] - P[5][:, 3]) < 0.05
    start = np.arange(7) * len(scans[0])
    f = gpu.extract_loam_features(start, np.concatenate(scans), np.tile(ring, 6), weak=False, labels=False, curvature=False)
    for k in range(6):
        assert f["edge_index"][f["edge_start"][k]:f["edge_start"][k + 1]].tolist() == feats[k]["sharp"], k
        assert f["surf_index"][f["surf_start"][k]:f["surf_start"][k + 1]].tolist() == feats[k]["flat"], k
    # ONE call, two maps: the first five scans' edges, then their surfaces
    e5, s5 = int(f["edge_start"][5]), int(f["surf_start"][5])
    scan_start = np.concatenate([f["edge_start"][:6], e5 + f["surf_start"][1:6]]).astype(np.int32)
    m = gpu.build_registration_maps([0, 5, 10], scan_start, np.concatenate([f["edge_points"][:e5], f["surf_points"][:s5]]), np.concatenate([P[:5], P[:5]]), 0.1)
    _same(dict(start=m["map_start"], points=m["map_points"], count=m["map_count"]), maps, "chained maps")
    a, b = int(m["map_start"][1]), int(m["map_start"][2])
    tgt_e, tgt_s = f["edge_points"][e5:], f["surf_points"][s5:]
    out = gpu.register_scans_loam([0, a], m["map_points"][:a], [0, b - a], m["map_points"][a:b], [0, len(tgt_e)], tgt_e, [0, len(tgt_s)], tgt_s, **loam_ref.DEFAULTS)
    got = dict({k: out[k][0] for k in ("T_refest_ref", "T_ref_tgt", "cov")}, cost=float(out["cost"][0]), **{k: int(out[k][0]) for k in loam_ref.COUNTS})
    _same_bits(got, want, "chained")
    error = float(np.linalg.norm(got["T_ref_tgt"][:, 3] - P[5][:, 3]))
    print(f"chained: map {np.diff(m['map_start']).tolist()}, translation error {error:.4f} m")
    assert error < 0.05
