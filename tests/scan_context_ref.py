"""NumPy restatement of the Scan Context contract that include/bsgpu.h pins for bsgpu_scan_context_describe and bsgpu_scan_context_match:
numpy.arctan2 for the sector, numpy.maximum.at for the bins, plain mean / norm, brute force over shifts and candidates.  Deliberately not
the code of beam_slam_amd/csrc/scan_context.h.  Also the scenes of the tests and the margins of their decisions (how far a point is from
a bin boundary, the gaps between best and second best), which must be far above rounding for two implementations to be comparable at all.
"""
import functools

import numpy as np

RINGS, SECTORS = 20, 60
DEFAULTS = dict(n_tree_candidates=10, search_ratio=0.1, dist_thres=0.3)
LIDAR_HEIGHT, MAX_RADIUS = 2.0, 40.0            # what the tests pass to describe
EYE = np.hstack([np.eye(3), np.zeros((3, 1))])


def rotz(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def transform(T, P):
    """T p as ((T0 x + T1 y) + T2 z) + T3 per row: the contract's order, every product and sum rounded."""
    T, P = np.asarray(T, float).reshape(3, 4), np.asarray(P, float).reshape(-1, 3)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def bins(P, max_radius):
    """Per point: ring, sector (-1, -1: dropped) and its distance from the nearest ring or sector boundary in bins (for a dropped point:
    from the radius)."""
    P = np.asarray(P, float).reshape(-1, 3)
    r = np.sqrt(P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1])
    theta = np.degrees(np.arctan2(P[:, 1], P[:, 0])) % 360.0
    fr, fs = r / max_radius * RINGS, theta / (360.0 / SECTORS)
    ring = np.clip(np.ceil(fr), 1, RINGS).astype(int) - 1
    sector = np.clip(np.ceil(fs), 1, SECTORS).astype(int) - 1
    keep = r <= max_radius
    ring_margin = np.where(fr < 0.5, np.inf, np.abs(fr - np.round(fr)))            # (no ring boundary at r = 0)
    margin = np.where(keep, np.minimum(ring_margin, np.abs(fs - np.round(fs))), np.abs(fr - RINGS))
    return np.where(keep, ring, -1), np.where(keep, sector, -1), margin


def keys(desc):
    """(ring key: the mean of each row, sector key: the mean of each column)"""
    return desc.mean(axis=1), desc.mean(axis=0)


def describe(scans, aggregates, lidar_height=LIDAR_HEIGHT, max_radius=MAX_RADIUS):
    """scans: list of (n, 3) arrays; aggregates: list of lists of (scan index, T or None).  Returns dict(desc (A, 20, 60), ring_key,
    sector_key, n_binned, margin: the smallest bin margin over every point of the call)."""
    A = len(aggregates)
    out = dict(desc=np.zeros((A, RINGS, SECTORS)), ring_key=np.zeros((A, RINGS)), sector_key=np.zeros((A, SECTORS)), n_binned=np.zeros(A, np.int32),
               margin=np.inf)
    for a, members in enumerate(aggregates):
        d = np.full((RINGS, SECTORS), -np.inf)
        for k, T in members:
            P = transform(EYE if T is None else T, scans[k])
            if len(P) == 0:
                continue
            ring, sector, margin = bins(P, max_radius)
            out["margin"] = min(out["margin"], float(margin.min()))
            keep = ring >= 0
            np.maximum.at(d, (ring[keep], sector[keep]), P[keep, 2] + lidar_height)
            out["n_binned"][a] += int(keep.sum())
        d[np.isneginf(d)] = 0.0
        out["desc"][a] = d
        out["ring_key"][a], out["sector_key"][a] = keys(d)
    return out


def search_radius(search_ratio):
    return int(min(np.floor(0.5 * search_ratio * SECTORS + 0.5), 30))


def window(shift0, R):
    return list(range(SECTORS)) if R >= 30 else sorted({(shift0 + k) % SECTORS for k in range(-R, R + 1)})


def _sum(x, rev):
    x = np.asarray(x, float)
    return float(np.sum(x[::-1] if rev else x))


def compare(q, c, R, rev=False):
    """One query against one candidate.  Returns (distance, shift, alignment gap, distance gap, the distances of the window's shifts)."""
    if rev:
        q, c = q[::-1], c[::-1]                    # the rings in the other order: every 20-term sum changes its order
    qk, ck = np.array([_sum(q[:, j], False) for j in range(SECTORS)]) / RINGS, np.array([_sum(c[:, j], False) for j in range(SECTORS)]) / RINGS
    norms = np.array([np.sqrt(_sum((qk - np.roll(ck, s)) ** 2, rev)) for s in range(SECTORS)])
    shift0 = int(np.argmin(norms))
    align_gap = float(np.partition(norms, 1)[1] - norms[shift0])
    nq = np.sqrt((q * q).sum(axis=0))
    dist = {}
    for s in window(shift0, R):
        cs = np.roll(c, s, axis=1)
        nc = np.sqrt((cs * cs).sum(axis=0))
        both = (nq != 0) & (nc != 0)
        if not both.any():
            dist[s] = np.inf
            continue
        cos = (q[:, both] * cs[:, both]).sum(axis=0) / (nq[both] * nc[both])
        dist[s] = 1.0 - _sum(cos, rev) / int(both.sum())
    shifts = list(dist)
    vals = np.array([dist[s] for s in shifts])
    k = int(np.argmin(vals))
    with np.errstate(invalid="ignore"):
        dist_gap = float(np.partition(vals, 1)[1] - vals[k]) if len(vals) > 1 else np.inf
    return float(vals[k]), shifts[k], align_gap, (np.inf if np.isnan(dist_gap) else dist_gap), dist


def match(query_desc, cand_desc, n_tree_candidates=10, search_ratio=0.1, dist_thres=0.3, rev=False):
    """One set.  Returns dict(best_cand, best_dist, best_shift, yaw (Q), dist_all, shift_all (Q x C, inf / 0: left out), taken (Q x C
    bool) and the gaps: align_gap, shift_gap (smallest over compared pairs), cand_gap (best against second-best compared candidate),
    tree_gap (K-th against (K+1)-th ring-key distance), thres_gap (|best_dist - dist_thres|))."""
    Q, C = len(query_desc), len(cand_desc)
    R, K = search_radius(search_ratio), n_tree_candidates
    out = dict(best_cand=np.full(Q, -1, np.int32), best_dist=np.full(Q, np.inf), best_shift=np.zeros(Q, np.int32), yaw=np.zeros(Q),
               dist_all=np.full((Q, C), np.inf), shift_all=np.zeros((Q, C), np.int32), taken=np.ones((Q, C), bool), align_gap=np.inf,
               shift_gap=np.inf, cand_gap=np.inf, tree_gap=np.inf, thres_gap=np.inf)
    for i, q in enumerate(query_desc):
        if 0 < K < C:
            qr = keys(q)[0]
            d2 = np.array([_sum((qr - keys(c)[0]) ** 2, rev) for c in cand_desc])
            order = np.argsort(d2, kind="stable")
            out["taken"][i] = False
            out["taken"][i, order[:K]] = True
            out["tree_gap"] = min(out["tree_gap"], float(d2[order[K]] - d2[order[K - 1]]))
        for j, c in enumerate(cand_desc):
            if out["taken"][i, j]:
                d, s, ag, sg, _ = compare(q, c, R, rev)
                out["dist_all"][i, j], out["shift_all"][i, j] = d, s
                out["align_gap"], out["shift_gap"] = min(out["align_gap"], ag), min(out["shift_gap"], sg)
        if C:
            row = np.where(out["taken"][i], out["dist_all"][i], np.inf)
            j = int(np.argmin(row))
            if not out["taken"][i, j]:
                j = int(np.argmax(out["taken"][i]))
            out["best_dist"][i], out["best_shift"][i] = row[j], out["shift_all"][i, j]
            out["best_cand"][i] = j if row[j] < dist_thres else -1
            if np.isfinite(row[j]):
                out["thres_gap"] = min(out["thres_gap"], abs(float(row[j]) - dist_thres))
                if out["taken"][i].sum() > 1:
                    out["cand_gap"] = min(out["cand_gap"], float(np.partition(row, 1)[1] - row[j]))
        out["yaw"][i] = out["best_shift"][i] * 2.0 * np.pi / SECTORS
    return out


def bound(a, b):
    """The allowed difference from `a`: 8 x the restatement's own difference under another summation order (`b`), and not below one
    unit of FP64 precision of the quantity's largest magnitude.  Entries that are infinite on both sides count as equal."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    fin = np.isfinite(a) & np.isfinite(b)
    assert (fin | (a == b)).all()
    own = float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0
    mag = float(np.abs(a[fin]).max()) if fin.any() else 0.0
    return max(8.0 * own, 2.0 ** -52 * mag), own


def check(got, want, other, who):
    """Asserts |got - want| <= bound(want, other); returns difference / bound (printed by the callers, recorded in their docstrings)."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    bd, own = bound(want, other)
    fin = np.isfinite(want)
    assert (got[~fin] == want[~fin]).all(), who
    diff = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    ratio = diff / bd if bd > 0 else (0.0 if diff == 0 else np.inf)
    print(f"{who}: difference {diff:.3e}, bound {bd:.3e} (own difference {own:.3e}), ratio {ratio:.3f}")
    assert diff <= bd, (who, diff, bd)
    return ratio


# ---- the commands of tests/plan/test_scan_context.cpp (and of scripts/time_scan_context_cpu.cpp): arrays of doubles -------------------------
def describe_command(scans, aggregates, lidar_height=LIDAR_HEIGHT, max_radius=MAX_RADIUS):
    """scans: list of (n, 3); aggregates: list of lists of (scan index, T or None) — all None or all given."""
    members = [m for a in aggregates for m in a]
    has_T = any(T is not None for _, T in members)
    ss = np.cumsum([0] + [len(s) for s in scans])
    ms = np.cumsum([0] + [len(a) for a in aggregates])
    pts = np.concatenate([np.asarray(s, float).reshape(-1) for s in scans]) if scans else np.zeros(0)
    T = np.concatenate([np.asarray(EYE if T is None else T, float).reshape(-1) for _, T in members]) if has_T else np.zeros(0)
    return np.concatenate([np.array([1, len(scans), len(aggregates), len(members), 1 if has_T else 0, lidar_height, max_radius], float), ss, pts, ms,
                           np.array([k for k, _ in members], float), T])


def match_command(sets, n_tree_candidates=10, search_ratio=0.1, dist_thres=0.3):
    """sets: list of (query descriptors (Q, 20, 60), candidate descriptors (C, 20, 60))."""
    qs = np.cumsum([0] + [len(q) for q, _ in sets])
    cs = np.cumsum([0] + [len(c) for _, c in sets])
    return np.concatenate([np.array([2, len(sets), n_tree_candidates, search_ratio, dist_thres], float), qs, cs] +
                          [np.asarray(q, float).reshape(-1) for q, _ in sets] + [np.asarray(c, float).reshape(-1) for _, c in sets])


def bin_command(xy, max_radius):
    xy = np.asarray(xy, float).reshape(-1, 2)
    return np.concatenate([np.array([3, len(xy), max_radius], float), xy.ravel()])


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
# a box room (centred at the origin, floor at z = 0) with vertical round pillars (x, y, radius) from floor to ceiling
PLACES = {
    "A": (np.array([20.0, 14.0, 5.0]), [(4.0, 3.0, 0.5), (-5.0, -2.5, 0.6), (-2.0, 4.0, 0.4)]),
    "B": (np.array([34.0, 8.0, 3.0]), [(9.0, -1.5, 0.5), (-11.0, 1.0, 0.5)]),
    "C": (np.array([60.0, 50.0, 9.0]), []),
}
SENSOR_Z = 1.5
# name -> (place, sensor x, y, yaw in degrees)
VIEWS = {"A": ("A", 1.0, 0.5, 0.0), "A_revisit": ("A", 1.3, 0.3, 93.0), "A_far": ("A", -6.0, 3.0, 200.0), "B": ("B", 3.0, -1.0, 40.0),
         "C": ("C", 7.0, -4.0, 10.0)}


def cast(place, sx, sy, yaw_deg, n=4000, seed=0):
    """n points in the sensor's frame: rays of a 16-beam revolution (elevations -15 .. 15 degrees, azimuths jittered) from (sx, sy,
    SENSOR_Z) at yaw_deg against the room's walls, floor, ceiling and pillars."""
    size, pillars = PLACES[place]
    rng = np.random.default_rng(seed)
    per = n // 16
    az = (np.arange(per)[None, :] + rng.random((16, per))) * (2 * np.pi / per)
    el = np.radians(np.linspace(-15.0, 15.0, 16))[:, None] + 0.0 * az
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1).reshape(-1, 3)      # sensor frame
    dw = d @ rotz(yaw_deg).T
    o = np.array([sx, sy, SENSOR_Z])
    t = np.full(len(d), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis, lo, hi in ((0, -size[0] / 2, size[0] / 2), (1, -size[1] / 2, size[1] / 2), (2, 0.0, size[2])):
            for plane in (lo, hi):
                tt = (plane - o[axis]) / dw[:, axis]
                t = np.where((tt > 1e-9) & (tt < t), tt, t)
        for cx, cy, rad in pillars:
            a = dw[:, 0] ** 2 + dw[:, 1] ** 2
            b = 2 * (dw[:, 0] * (o[0] - cx) + dw[:, 1] * (o[1] - cy))
            c = (o[0] - cx) ** 2 + (o[1] - cy) ** 2 - rad * rad
            disc = b * b - 4 * a * c
            tt = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / (2 * a)
            t = np.where((tt > 1e-9) & (tt < t), tt, t)
    P = d * t[:, None]
    assert np.isfinite(P).all() and len(P) == n
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def scan(name):
    place, sx, sy, yaw = VIEWS[name]
    return cast(place, sx, sy, yaw, seed=sorted(VIEWS).index(name))


@functools.lru_cache(maxsize=None)
def descriptors(names=tuple(VIEWS)):
    """The restatement's descriptors of the named views, one scan per aggregate, identity members — computed once per process."""
    return describe([scan(n) for n in names], [[(k, None)] for k in range(len(names))])


@functools.lru_cache(maxsize=None)
def matched(query=("A",), cands=("A_revisit", "A_far", "B", "C"), rev=False, **kw):
    D = descriptors()["desc"]
    idx = {n: k for k, n in enumerate(VIEWS)}
    return match(D[[idx[n] for n in query]], D[[idx[n] for n in cands]], rev=rev, **dict(DEFAULTS, **kw))
