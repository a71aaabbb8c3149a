"""bsgpu_essential_ransac (cv::findEssentialMat's RANSAC for a batch of match sets, k_ransac.hip) on the device against
tests/essential_ref.py, the independent NumPy restatement of the contract's serial loop (not against five_point.h)."""

import numpy as np
import pytest

import essential_ref as ref
from beam_slam_amd import capi

pytestmark = pytest.mark.gpu
SEED = 2024
_REF = {}


@pytest.fixture(scope="module")
def g(gpu_solver_cls):
    return gpu_solver_cls(0)


def _call(g, sets, lead=0, **kw):
    """One call for `sets` behind `lead` empty sets (so that a set keeps the position, hence the sampler stream, it has elsewhere)."""
    sizes = [0] * lead + [len(s["px_prev"]) for s in sets]
    ms = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    p1 = np.concatenate([np.zeros((0, 2))] + [s["px_prev"] for s in sets])
    p2 = np.concatenate([np.zeros((0, 2))] + [s["px_cur"] for s in sets])
    K = np.array([ref.K_DEFAULT] * lead + [s["K"] for s in sets])
    out = g.essential_ransac(ms, p1, p2, K, seed=SEED, **kw)
    out["masks"] = [out["mask"][ms[k]:ms[k + 1]] for k in range(len(sizes))]
    return out


def _ref(key, st, set_index=0, **kw):
    """The reference's serial loop, computed once per case and shared."""
    if key not in _REF:
        _REF[key] = ref.ransac_serial(st["px_prev"], st["px_cur"], st["K"], seed=SEED, set_index=set_index, **kw)
    return _REF[key]


def test_five_noise_free_matches(g):
    """n = 5: every solution has 5 inliers and the first one (ascending E[0]) wins, ep = 0 ends the loop after one sample.  The seed
    is one whose true E is that first solution.  Tolerance: 100 x the reference's own distance to the truth, floor 1e-12."""
    st = ref.make_set(20, 5, 0.0)
    x1, x2 = ref.normalize_pixels(st["px_prev"], st["K"]), ref.normalize_pixels(st["px_cur"], st["K"])
    sols = ref.five_point(x1, x2)
    ref_err = ref.dist_E(sols[0], st["E_true"])
    assert ref_err == min(ref.dist_E(S, st["E_true"]) for S in sols) and ref_err < 1e-6
    out = _call(g, [st])
    assert out["status"][0] == capi.RANSAC_OK and out["n_inliers"][0] == 5 and out["n_iters"][0] == 1
    assert np.all(out["mask"] == 1) and sorted(out["best_sample"][0]) == [0, 1, 2, 3, 4]
    err = ref.dist_E(out["E"][0], st["E_true"])
    print(f"n = 5: device distance to the truth {err:.3e}, reference {ref_err:.3e}")
    assert err <= max(100.0 * ref_err, 1e-12)


def test_small_sets_in_a_batch(g):
    sets = [ref.make_set(20, 0, 0.0), ref.make_set(21, 4, 0.0), ref.make_set(22, 5, 0.0), ref.make_set(23, 40, 0.3)]
    out = _call(g, sets)
    assert list(out["status"][:2]) == [capi.RANSAC_TOO_FEW] * 2
    assert np.all(out["masks"][1] == 1) and len(out["masks"][0]) == 0
    assert np.all(out["E"][:2] == 0) and np.all(out["n_iters"][:2] == 0) and np.all(out["best_sample"][:2] == -1)
    assert np.all(out["n_inliers"][:2] == 0)
    for k in (2, 3):   # unaffected by their neighbours: the same bits as alone at the same position
        lone = _call(g, [sets[k]], lead=k)
        assert out["status"][k] == lone["status"][k] == capi.RANSAC_OK
        assert np.array_equal(out["masks"][k], lone["masks"][k]) and out["n_iters"][k] == lone["n_iters"][k]
        assert out["E"][k].tobytes() == lone["E"][k].tobytes()
    assert np.array_equal(out["masks"][3], sets[3]["labels"])


@pytest.mark.parametrize("n,n_out", [(40, 12), (257, 128), (300, 150)])
def test_gap_data_matches_the_serial_loop(g, n, n_out):
    """Noise-free inliers, outliers at least 10 px off: the mask is the labels; 50 % outliers need about 145 samples, nine rounds of
    16, so the in-order updates of a round and the dropping of samples past niters decide n_iters and best_sample."""
    st = ref.make_set(500 + n, n, n_out / n)
    r = _ref(("gap", n), st)
    out = _call(g, [st])
    assert out["status"][0] == r["status"] == capi.RANSAC_OK
    assert np.array_equal(out["mask"], st["labels"]) and np.array_equal(r["mask"], st["labels"])
    assert out["n_inliers"][0] == r["n_inliers"] == n - n_out
    assert out["n_iters"][0] == r["n_iters"]
    assert np.array_equal(out["best_sample"][0], r["best_sample"])
    if n_out * 2 >= n:
        assert r["n_iters"] > 16


def test_batch_of_33_sets_equals_lone_calls(g):
    sets = []
    for k in range(33):
        n = 5 + (125 * k) // 32
        K = (380.0 + 3.0 * k, 395.0 + 2.0 * k, 310.0 + k, 235.0 + 0.5 * k)
        sets.append(ref.make_set(700 + k, n, 0.3 if n >= 20 else 0.0, K=K))
    assert len(sets[0]["px_prev"]) == 5 and len(sets[-1]["px_prev"]) == 130
    out = _call(g, sets)
    for k, st in enumerate(sets):
        lone = _call(g, [st], lead=k)
        assert out["status"][k] == lone["status"][k]
        assert np.array_equal(out["masks"][k], lone["masks"][k]), k
        assert out["n_iters"][k] == lone["n_iters"][k] and out["n_inliers"][k] == lone["n_inliers"][k]
        assert out["E"][k].tobytes() == lone["E"][k].tobytes(), k
        assert np.array_equal(out["best_sample"][k], lone["best_sample"][k])
    assert np.all(out["status"] == capi.RANSAC_OK) and np.all(out["n_iters"] >= 1)


def test_iteration_cap_on_random_matches(g):
    st = ref.make_random_set(41, 64)
    r = _ref(("cap",), st, max_iters=64)
    out = _call(g, [st], max_iters=64)
    assert out["n_iters"][0] == r["n_iters"] == 64
    assert out["status"][0] == r["status"] and out["status"][0] in (capi.RANSAC_OK, capi.RANSAC_NO_MODEL)
    assert np.all(np.isfinite(out["E"])) and set(np.unique(out["mask"])) <= {0, 1}
    if out["status"][0] == capi.RANSAC_OK:
        assert out["n_inliers"][0] == int(out["mask"].sum()) >= 5
    else:
        assert np.all(out["mask"] == 1) and np.all(out["E"] == 0)


def test_rounded_pixels(g):
    """300 matches truncated to integers (the reference's cast<int>), 20 % gross outliers, 1 px: every gross outlier is rejected and
    the mask is the reference loop's, apart from matches whose reference error lies within a relative 1e-6 of thr^2 (none here)."""
    st = ref.make_set(903, 300, 0.2, truncate=True)
    r = _ref(("rounded",), st)
    out = _call(g, [st])
    assert out["status"][0] == r["status"] == capi.RANSAC_OK
    assert np.all(out["mask"][st["labels"] == 0] == 0)
    edge = np.abs(r["err"] - r["thr2"]) <= 1e-6 * r["thr2"]
    assert edge.sum() <= 3
    assert np.array_equal(out["mask"][~edge], r["mask"][~edge])
    assert out["n_iters"][0] == r["n_iters"] and np.array_equal(out["best_sample"][0], r["best_sample"])


def test_invalid_arguments(g):
    from beam_slam_amd import gpu
    fn = gpu.lib().bsgpu_essential_ransac
    fn.argtypes = capi.ESSENTIAL_RANSAC_ARGTYPES
    st = ref.make_set(23, 40, 0.3)
    n = 40
    p1, p2 = np.ascontiguousarray(st["px_prev"]), np.ascontiguousarray(st["px_cur"])
    K = np.array(st["K"])
    dp, ip, bp = capi._dp, capi._ip, capi._bp

    def call(ms=(0, n), prev=p1, cur=p2, Kv=K, prob=0.99, thr=1.0, iters=100, mask=True, status=True, ctx=True, n_sets=None):
        ms = np.array(ms, np.int32)
        m = np.full(max(int(ms.max()), 1), 7, np.uint8)
        stt = np.full(ms.size, 9, np.int32)
        rc = fn(g._ctx if ctx else None, ms.size - 1 if n_sets is None else n_sets, ms.ctypes.data_as(ip),
                None if prev is None else prev.ctypes.data_as(dp), None if cur is None else cur.ctypes.data_as(dp),
                None if Kv is None else np.ascontiguousarray(Kv, np.float64).ctypes.data_as(dp), prob, thr, iters, 1,
                m.ctypes.data_as(bp) if mask else None, None, None, None, None, stt.ctypes.data_as(ip) if status else None)
        assert rc != capi.OK and np.all(m == 7) and np.all(stt == 9)     # nothing was written
        return rc

    assert fn(g._ctx, 1, np.array([0, n], np.int32).ctypes.data_as(ip), p1.ctypes.data_as(dp), p2.ctypes.data_as(dp), K.ctypes.data_as(dp),
              0.99, 1.0, 100, 1, np.zeros(n, np.uint8).ctypes.data_as(bp), None, None, None, None,
              np.zeros(1, np.int32).ctypes.data_as(ip)) == capi.OK       # every optional output NULL
    for kw in (dict(prev=None), dict(cur=None), dict(Kv=None), dict(mask=False), dict(status=False), dict(ctx=False), dict(n_sets=-1),
               dict(ms=(0, 30, 20), Kv=np.tile(K, 2)), dict(ms=(1, n)), dict(prob=0.0), dict(prob=1.0), dict(prob=float("nan")),
               dict(thr=0.0), dict(thr=-1.0), dict(iters=0), dict(Kv=np.array([0.0, 400, 320, 240])),
               dict(Kv=np.array([400, -1.0, 320, 240]))):
        assert call(**kw) == capi.ERR_INVALID, kw
    big = capi.RANSAC_MAX_MATCHES + 1
    z = np.zeros((big, 2))
    assert call(ms=(0, big), prev=z, cur=z) == capi.ERR_UNSUPPORTED
