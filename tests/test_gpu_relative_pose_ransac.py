"""bsgpu_relative_pose_ransac (the two-view bootstrap of ComputePathWithVision for a batch of match sets, k_relpose.hip) on the device
against tests/seven_point_ref.py, the independent NumPy restatement of the contract's serial loop (not against seven_point.h).

Gap data (seven_point_ref.make_pair): noise-free inliers, every outlier at least 40 px off the true epipolar line; under the true
model the outliers then have at least 24 px of reprojection error and the inliers at most 4e-13 px, so at 5 px and at 10 px the mask is
the labels and the ratio the inlier share exactly."""

import numpy as np
import pytest

import p3p_ref
import seven_point_ref as ref
from beam_slam_amd import capi

pytestmark = pytest.mark.gpu
SEED = 2026
ROUND = 16   # samples per round of relpose_kernel
_REF = {}

# three cameras: intrinsics and T_cam_baselink all different
_R0 = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
CAMS = [(ref.K_DEFAULT, ref.rodrigues([0.012, 0.04, -0.008]) @ _R0, np.array([0.05, -0.02, 0.1])),
        ((440.0, 452.5, 380.25, 236.0), ref.rodrigues([-0.03, 0.01, 0.02]) @ _R0, np.array([-0.04, 0.03, 0.12])),
        ((471.5, 463.0, 359.5, 251.75), ref.rodrigues([0.02, -0.05, 0.015]) @ _R0, np.array([0.0, 0.06, -0.05]))]


def _camera(K, R_cb, t_cb):
    c = capi.Camera()
    c.fx, c.fy, c.cx, c.cy = K
    c.R_cam_baselink[:] = list(np.ravel(R_cb))
    c.t_cam_baselink[:] = list(t_cb)
    return c


@pytest.fixture(scope="module")
def g(gpu_solver_cls):
    s = gpu_solver_cls(0)
    s.set_cameras([_camera(*c) for c in CAMS])
    return s


def _call(g, pairs, lead=0, **kw):
    """One call for `pairs` behind `lead` empty sets (so that a set keeps the position, hence the sampler stream, it has elsewhere)."""
    sizes = [0] * lead + [len(p["px_first"]) for p in pairs]
    ms = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    p0 = np.concatenate([np.zeros((0, 2))] + [p["px_first"] for p in pairs])
    p1 = np.concatenate([np.zeros((0, 2))] + [p["px_last"] for p in pairs])
    cam = np.array([0] * lead + [p.get("cam", 0) for p in pairs], np.int32)
    out = g.relative_pose_ransac(ms, p0, p1, cam, seed=SEED, **kw)
    for name in ("mask", "valid_mask", "points"):
        out[name + "s"] = [out[name][ms[k]:ms[k + 1]] for k in range(len(sizes))]
    return out


def _ref(key, pr, set_index=0, **kw):
    """The reference's serial loop, computed once per case and shared."""
    if key not in _REF:
        _REF[key] = ref.ransac_serial(pr["px_first"], pr["px_last"], pr["K"], seed=SEED, set_index=set_index, **kw)
    return _REF[key]


def _quat_dist(q, p, R, t):
    return max(np.abs(ref.quat_to_rot(q) - R).max(), np.abs(np.asarray(p) - t).max())


def _pose_errors(out, k, r, pr):
    """(device, reference) distance of T_last_first to the truth; the device's q / p against its own T_last_first."""
    T = out["T_last_first"][k]
    dev = ref.pose_dist((T[:, :3], T[:, 3]), pr["R"], pr["t"])
    own = ref.pose_dist((r["R"], r["t"]), pr["R"], pr["t"])
    _, R_cb, t_cb = CAMS[pr.get("cam", 0)]
    (Ra, pa), (Rb, pb) = ref.baselink_poses(T[:, :3], T[:, 3], R_cb, t_cb)
    assert _quat_dist(out["q"][k][0], out["p"][k][0], Ra, pa) <= 1e-12 and _quat_dist(out["q"][k][1], out["p"][k][1], Rb, pb) <= 1e-12
    for q in out["q"][k]:
        assert abs(np.linalg.norm(q) - 1.0) <= 1e-14 and q[0] >= 0.0
    assert abs(np.linalg.norm(T[:, 3]) - 1.0) <= 1e-14
    return dev, own


_BITS = ("q", "p", "T_last_first", "inlier_ratio")


def _same_bits(a, b, ka, kb):
    assert a["status"][ka] == b["status"][kb] and a["pair_valid"][ka] == b["pair_valid"][kb]
    assert np.array_equal(a["masks"][ka], b["masks"][kb]) and np.array_equal(a["valid_masks"][ka], b["valid_masks"][kb])
    assert a["pointss"][ka].tobytes() == b["pointss"][kb].tobytes()
    assert a["n_iters"][ka] == b["n_iters"][kb] and a["n_inliers"][ka] == b["n_inliers"][kb]
    assert np.array_equal(a["best_sample"][ka], b["best_sample"][kb])
    for name in _BITS:
        assert a[name][ka].tobytes() == b[name][kb].tobytes(), name


def _assert_no_model(out, k):
    assert np.all(out["masks"][k] == 0) and np.all(out["valid_masks"][k] == 0) and np.all(np.isnan(out["pointss"][k]))
    assert out["n_inliers"][k] == 0 and np.all(out["best_sample"][k] == -1) and out["pair_valid"][k] == 0
    for name in _BITS:
        assert np.all(np.isnan(out[name][k])), name


def test_eight_noise_free_matches(g):
    """n = 8: the true pose has 8 inliers, ep = 0 ends the loop after one sample.  Tolerance: 100 x the reference's own distance to
    the truth, floor 1e-12.  Measured: device 3.5e-15, reference 8.2e-14."""
    pr = ref.make_pair(31, 8, 0)
    r = _ref(("eight",), pr, prob=0.99)
    assert r["status"] == ref.STATUS_OK and r["n_iters"] == 1
    out = _call(g, [pr], prob=0.99)
    assert out["status"][0] == capi.RANSAC_OK and out["n_inliers"][0] == 8 and out["n_iters"][0] == 1 and out["pair_valid"][0] == 1
    assert np.all(out["mask"] == 1) and np.array_equal(out["best_sample"][0], r["best_sample"])
    dev, own = _pose_errors(out, 0, r, pr)
    print(f"n = 8: device distance to the truth {dev:.3e}, reference {own:.3e}")
    assert dev <= max(100.0 * own, 1e-12)


def test_small_sets_in_a_batch(g):
    pairs = [ref.make_pair(40, 0, 0), ref.make_pair(41, 7, 0), ref.make_pair(42, 8, 0), ref.make_pair(43, 40, 12)]
    out = _call(g, pairs, prob=0.99)
    assert list(out["status"]) == [capi.RANSAC_TOO_FEW, capi.RANSAC_TOO_FEW, capi.RANSAC_OK, capi.RANSAC_OK]
    assert len(out["masks"][0]) == 0 and len(out["masks"][1]) == 7
    for k in (0, 1):
        _assert_no_model(out, k)
        assert out["n_iters"][k] == 0
    for name in _BITS:
        assert np.all(np.isfinite(out[name][2:]))
    for k in (2, 3):   # unaffected by their neighbours: the same bits as alone at the same position
        _same_bits(out, _call(g, [pairs[k]], lead=k, prob=0.99), k, k)
    assert np.array_equal(out["masks"][3], pairs[3]["labels"]) and np.array_equal(out["valid_masks"][3], pairs[3]["labels"])


GAP_SEEDS = {40: 541, 257: 757, 300: 800}


@pytest.mark.parametrize("n,n_out", [(40, 12), (257, 77), (300, 120)])
def test_gap_data_matches_the_serial_loop(g, n, n_out):
    """The mask is the labels; n_iters and best_sample are the restatement's.  40 % outliers need about 160 samples, more than two
    rounds of 16 and not a multiple of the round size, so the in-order updates of a round and the dropping of samples past niters
    decide n_iters and best_sample.  Measured: n_iters 54, 53 and 162; distance of T_last_first to the truth: device 2.6e-15,
    1.3e-13 and 4.8e-15, reference 5.2e-15, 1.5e-13 and 4.1e-15."""
    pr = ref.make_pair(GAP_SEEDS[n], n, n_out)
    r = _ref(("gap", n), pr, prob=0.99, max_iters=2000)
    out = _call(g, [pr], prob=0.99, max_iters=2000)
    assert out["status"][0] == r["status"] == capi.RANSAC_OK
    assert np.array_equal(out["mask"], pr["labels"]) and np.array_equal(r["mask"], pr["labels"])
    assert out["n_inliers"][0] == r["n_inliers"] == n - n_out
    assert out["n_iters"][0] == r["n_iters"]
    assert np.array_equal(out["best_sample"][0], r["best_sample"])
    if n == 300:
        assert r["n_iters"] > 2 * ROUND and r["n_iters"] % ROUND != 0
    dev, own = _pose_errors(out, 0, r, pr)
    print(f"n = {n}: n_iters {r['n_iters']}, device distance to the truth {dev:.3e}, reference {own:.3e}")
    assert dev <= max(100.0 * own, 1e-12)


def test_fixed_loop_of_the_reference_call(g):
    """prob = 0, max_iters = 100, 5 px — RANSACEstimator(cam, cam, first, last, SEVENPOINT, 100): all 100 samples are consumed."""
    pr = ref.make_pair(640, 120, 36)
    r = _ref(("fixed",), pr)
    out = _call(g, [pr])
    assert out["status"][0] == r["status"] == capi.RANSAC_OK
    assert out["n_iters"][0] == r["n_iters"] == 100
    assert np.array_equal(out["best_sample"][0], r["best_sample"]) and out["n_inliers"][0] == r["n_inliers"]
    assert np.array_equal(out["mask"], pr["labels"])


def test_batch_of_33_sets_equals_lone_calls(g):
    pairs = []
    for k in range(33):
        n = 8 + (122 * k) // 32
        pr = ref.make_pair(700 + k, n, int(0.3 * n) if n >= 30 else 0, K=CAMS[k % 3][0])
        pr["cam"] = k % 3
        pairs.append(pr)
    assert len(pairs[0]["px_first"]) == 8 and len(pairs[-1]["px_first"]) == 130
    out = _call(g, pairs, prob=0.99)
    for k, pr in enumerate(pairs):
        _same_bits(out, _call(g, [pr], lead=k, prob=0.99), k, k)
    assert np.all(out["status"] == capi.RANSAC_OK) and np.all(out["n_iters"] >= 1)
    for k in (5, 18, 31):   # one set per camera: its own K and T_cam_baselink went into the result
        pr = pairs[k]
        T = out["T_last_first"][k]
        assert ref.pose_dist((T[:, :3], T[:, 3]), pr["R"], pr["t"]) <= 1e-6
        (Ra, pa), (Rb, pb) = ref.baselink_poses(pr["R"], pr["t"], CAMS[pr["cam"]][1], CAMS[pr["cam"]][2])
        assert _quat_dist(out["q"][k][0], out["p"][k][0], Ra, pa) <= 1e-12 and _quat_dist(out["q"][k][1], out["p"][k][1], Rb, pb) <= 1e-6


@pytest.mark.parametrize("n_out,ratio,pair_valid", [(20, 0.9, 1), (60, 0.7, 0)])
def test_validity_gate(g, n_out, ratio, pair_valid):
    """200 matches: the 10 px gate keeps exactly the labelled inliers, the ratio is their share, 0.8 decides.  The points of the
    inliers are the true ones within 100 x the restatement's own distance (floor 1e-12).  Measured: device 1.7e-12 and 1.0e-12,
    reference 1.1e-12 and 1.3e-12."""
    pr = ref.make_pair(900 + n_out, 200, n_out)
    r = _ref(("gate", n_out), pr)
    out = _call(g, [pr])
    assert out["status"][0] == r["status"] == capi.RANSAC_OK
    assert np.array_equal(out["valid_mask"], pr["labels"]) and np.array_equal(r["valid_mask"], pr["labels"])
    assert out["inlier_ratio"][0] == r["inlier_ratio"] == ratio
    assert out["pair_valid"][0] == r["pair_valid"] == pair_valid
    inl = pr["labels"] == 1
    own = np.abs(r["points"][inl] - pr["points"][inl]).max()
    dev = np.abs(out["points"][inl] - pr["points"][inl]).max()
    print(f"{n_out} outliers: distance of the inliers' points to the truth: device {dev:.3e}, reference {own:.3e}")
    assert dev <= max(100.0 * own, 1e-12)


def test_truncated_pixels(g):
    """300 matches truncated to integers (the reference's cast<int>), 20 % gross outliers, 5 px: every gross outlier is rejected and
    the mask is the reference loop's, apart from matches whose reference error lies within a relative 1e-6 of thr^2 (at most 1 %)."""
    pr = ref.make_pair(905, 300, 60)
    r = _ref(("truncated",), pr, prob=0.99, max_iters=2000, truncate=True)
    out = _call(g, [pr], prob=0.99, max_iters=2000, truncate_pixels=True)
    assert out["status"][0] == r["status"] == capi.RANSAC_OK
    assert np.all(out["mask"][pr["labels"] == 0] == 0)
    edge = np.abs(r["err"] - r["thr2"]) <= 1e-6 * r["thr2"]
    assert edge.sum() <= 3
    assert out["n_iters"][0] == r["n_iters"]
    assert np.array_equal(out["mask"][~edge], r["mask"][~edge])


def test_iteration_cap_on_random_matches(g):
    pr = ref.make_random_pair(41, 64)
    r = _ref(("cap",), pr, prob=0.99, max_iters=64)
    out = _call(g, [pr], prob=0.99, max_iters=64)
    assert out["n_iters"][0] == r["n_iters"] <= 64
    assert out["status"][0] == r["status"] and out["status"][0] in (capi.RANSAC_OK, capi.RANSAC_NO_MODEL)
    assert set(np.unique(out["mask"])) <= {0, 1} and set(np.unique(out["valid_mask"])) <= {0, 1}
    if out["status"][0] == capi.RANSAC_OK:
        assert out["n_inliers"][0] == int(out["mask"].sum()) >= 8
        assert all(np.all(np.isfinite(out[name])) for name in _BITS)
        assert np.all(np.isfinite(out["points"][out["mask"] == 1]))
        assert out["inlier_ratio"][0] == out["valid_mask"].sum() / 64
    else:
        assert out["n_iters"][0] == 64
        _assert_no_model(out, 0)


def test_invalid_arguments(g):
    from beam_slam_amd import gpu
    fn = gpu.lib().bsgpu_relative_pose_ransac
    fn.argtypes = capi.RELATIVE_POSE_RANSAC_ARGTYPES
    pr = ref.make_pair(43, 40, 12)
    n = 40
    a0, b0 = np.ascontiguousarray(pr["px_first"]), np.ascontiguousarray(pr["px_last"])
    dp, ip, bp = capi._dp, capi._ip, capi._bp

    def call(ms=(0, n), p0=a0, p1=b0, cam=(0,), prob=0.99, thr=5.0, iters=100, val=10.0, ratio=0.8, mask=True, q=True, p=True, pv=True,
             status=True, ctx=True, n_sets=None, start=True):
        ms = np.array(ms, np.int32)
        cam = None if cam is None else np.array(cam, np.int32)
        S, m_n = ms.size, max(int(ms.max()), 1)
        m, vm = np.full(m_n, 7, np.uint8), np.full(m_n, 7, np.uint8)
        stt, pvo = np.full(S, 9, np.int32), np.full(S, 9, np.int32)
        dbl = {k: np.full(sz, 5.0) for k, sz in dict(T=12 * S, q=8 * S, p=6 * S, pts=3 * m_n, ratio=S).items()}
        ints = np.full(9 * S, 9, np.int32)
        rc = fn(g._ctx if ctx else None, S - 1 if n_sets is None else n_sets, ms.ctypes.data_as(ip) if start else None,
                None if p0 is None else p0.ctypes.data_as(dp), None if p1 is None else p1.ctypes.data_as(dp),
                None if cam is None else cam.ctypes.data_as(ip), prob, thr, iters, 1, 0, val, ratio, m.ctypes.data_as(bp) if mask else None,
                dbl["T"].ctypes.data_as(dp), dbl["q"].ctypes.data_as(dp) if q else None, dbl["p"].ctypes.data_as(dp) if p else None,
                dbl["pts"].ctypes.data_as(dp), vm.ctypes.data_as(bp), dbl["ratio"].ctypes.data_as(dp), pvo.ctypes.data_as(ip) if pv else None,
                ints[:S].ctypes.data_as(ip), ints[S:2 * S].ctypes.data_as(ip), ints[2 * S:].ctypes.data_as(ip),
                stt.ctypes.data_as(ip) if status else None)
        assert rc != capi.OK     # nothing was written
        assert np.all(m == 7) and np.all(vm == 7) and np.all(stt == 9) and np.all(pvo == 9) and np.all(ints == 9)
        assert all(np.all(v == 5.0) for v in dbl.values())
        return rc

    q1, p1 = np.zeros(8), np.zeros(6)
    assert fn(g._ctx, 1, np.array([0, n], np.int32).ctypes.data_as(ip), a0.ctypes.data_as(dp), b0.ctypes.data_as(dp),
              np.zeros(1, np.int32).ctypes.data_as(ip), 0.0, 5.0, 100, 1, 0, 10.0, 0.8, np.zeros(n, np.uint8).ctypes.data_as(bp), None,
              q1.ctypes.data_as(dp), p1.ctypes.data_as(dp), None, None, None, np.zeros(1, np.int32).ctypes.data_as(ip), None, None, None,
              np.zeros(1, np.int32).ctypes.data_as(ip)) == capi.OK   # every optional output NULL
    assert np.all(np.isfinite(q1)) and np.all(np.isfinite(p1))
    for kw in (dict(start=False), dict(p0=None), dict(p1=None), dict(cam=None), dict(mask=False), dict(q=False), dict(p=False), dict(pv=False),
               dict(status=False), dict(ctx=False), dict(n_sets=-1), dict(ms=(0, 30, 20), cam=(0, 0)), dict(ms=(1, n)), dict(prob=-0.1),
               dict(prob=1.0), dict(prob=float("nan")), dict(thr=0.0), dict(thr=-1.0), dict(val=0.0), dict(val=-2.0), dict(iters=0),
               dict(ratio=-0.1), dict(ratio=1.5), dict(ratio=float("nan")), dict(cam=(3,)), dict(cam=(-1,))):
        assert call(**kw) == capi.ERR_INVALID, kw
    big = capi.RANSAC_MAX_MATCHES + 1
    assert call(ms=(0, big), p0=np.zeros((big, 2)), p1=np.zeros((big, 2))) == capi.ERR_UNSUPPORTED


def test_points_feed_absolute_pose_ransac(g):
    """The chain of the bootstrap: points[valid_mask] and a third view's pixels of the same landmarks go into
    bsgpu_absolute_pose_ransac and reproduce that view's true pose (world = first camera) within 100 x the distance the same call
    reaches from the TRUE points, floor 1e-9.  Measured: 1.9e-13 against 4.6e-14."""
    pr = ref.make_pair(810, 100, 10)
    rng = np.random.default_rng(811)
    R3, t3 = ref.rodrigues(rng.normal(0.0, 0.08, 3)), rng.normal(0.0, 0.4, 3)
    pix3 = ref.project(pr["points"] @ R3.T + t3, pr["K"])
    out = _call(g, [pr])
    assert out["status"][0] == capi.RANSAC_OK and out["pair_valid"][0] == 1 and np.array_equal(out["valid_mask"], pr["labels"])
    keep = out["valid_mask"] == 1
    os_ = [0, int(keep.sum())]
    a = g.absolute_pose_ransac(os_, pix3[keep], out["points"][keep], 0, seed=SEED)
    b = g.absolute_pose_ransac(os_, pix3[keep], pr["points"][keep], 0, seed=SEED)
    assert a["status"][0] == capi.RANSAC_OK and b["status"][0] == capi.RANSAC_OK and np.all(a["mask"] == 1)
    Ta, Tb = a["T_cam_world"][0], b["T_cam_world"][0]
    got, own = p3p_ref.pose_dist((Ta[:, :3], Ta[:, 3]), R3, t3), p3p_ref.pose_dist((Tb[:, :3], Tb[:, 3]), R3, t3)
    print(f"chained: distance of the third view's pose to the truth {got:.3e}; from the true points {own:.3e}")
    assert got <= max(100.0 * own, 1e-9)
