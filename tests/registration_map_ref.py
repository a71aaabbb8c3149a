"""bsgpu_build_registration_maps restated in NumPy, independently of beam_slam_amd/csrc/registration_map.h: the transform as three
products and three additions per coordinate (no fused multiply-add), numpy.floor for the voxel, numpy.lexsort for the order, and every
centroid from math.fsum — the exactly rounded sum — divided by the count.  Besides the maps it returns what a comparison needs: the
smallest distance of any transformed coordinate to a voxel boundary (below it the two sides may put a point into different voxels),
and per output coordinate the magnitude M of the error bound (k + 8) 2^-52 M, M the largest sum_j |T_aj p_j| + |t_a| over the voxel's
points: k - 1 sequential additions and the division on the header's side, one rounding on this side, and the transform's own rounding
(three products and additions here, three fused steps there) on both."""
import math

import numpy as np

MERGE_ONLY = -1.0
CELL_RANGE = 2.0 ** 20
EPS = 2.0 ** -52


def transform(T, p):
    """q = T p for n points, T 3 x 4: ((T_a0 p_0 + T_a1 p_1) + T_a2 p_2) + t_a, and sum_j |T_aj p_j| + |t_a|"""
    T = np.asarray(T, float).reshape(3, 4)
    q, mag = np.empty_like(p), np.empty_like(p)
    with np.errstate(all="ignore"):
        for a in range(3):
            x, y, z = T[a, 0] * p[:, 0], T[a, 1] * p[:, 1], T[a, 2] * p[:, 2]
            q[:, a] = ((x + y) + z) + T[a, 3]
            mag[:, a] = np.abs(x) + np.abs(y) + np.abs(z) + abs(T[a, 3])
    return q, mag


def build(map_scan_start, scan_start, points, T=None, v=0.1):
    """-> dict(ok, start, points, count, mag, margin); ok False: a finite coordinate with |q / v| >= 2^20"""
    points = np.asarray(points, float).reshape(-1, 3)
    n_maps = len(map_scan_start) - 1
    start, out_p, out_c, out_m, margin = [0], [], [], [], np.inf
    for m in range(n_maps):
        qs, mags = [np.zeros((0, 3))], [np.zeros((0, 3))]
        for s in range(map_scan_start[m], map_scan_start[m + 1]):
            p = points[scan_start[s]:scan_start[s + 1]]
            if T is None:
                q, mag = p.copy(), np.abs(p)
            else:
                q, mag = transform(np.asarray(T, float).reshape(-1, 12)[s], p)
            qs.append(q); mags.append(mag)
        q, mag = np.concatenate(qs), np.concatenate(mags)
        if v == MERGE_ONLY:
            out_p.append(q); out_c.append(np.ones(len(q), np.int32)); out_m.append(mag)
            start.append(start[-1] + len(q))
            continue
        keep = np.isfinite(q).all(axis=1)
        q, mag = q[keep], mag[keep]
        d = q / v
        if (np.abs(d) >= CELL_RANGE).any():
            return dict(ok=False)
        cell = np.floor(d)
        if len(q):
            frac = d - cell
            margin = min(margin, float(np.minimum(frac, 1.0 - frac).min()) * v)
        order = np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))      # stable: equal cells keep their input order
        cs = cell[order]
        heads = np.flatnonzero(np.r_[True, (cs[1:] != cs[:-1]).any(axis=1)]) if len(q) else np.zeros(0, int)
        ends = np.r_[heads[1:], len(q)]
        P, M = np.zeros((len(heads), 3)), np.zeros((len(heads), 3))
        for k, (a, b) in enumerate(zip(heads, ends)):
            rows = q[order[a:b]]
            P[k] = [math.fsum(rows[:, c]) / (b - a) for c in range(3)]
            M[k] = mag[order[a:b]].max(axis=0)
        out_p.append(P); out_c.append((ends - heads).astype(np.int32)); out_m.append(M)
        start.append(start[-1] + len(heads))
    cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape)
    return dict(ok=True, start=np.array(start, np.int32), points=cat(out_p, (0, 3)), count=cat(out_c, 0).astype(np.int32), mag=cat(out_m, (0, 3)),
                margin=margin)


def bound(res):
    """per output coordinate: (k + 8) 2^-52 M"""
    return (res["count"][:, None] + 8.0) * EPS * res["mag"]


def pose(rx, ry, rz, t):
    """a 3 x 4 transform from three small angles (radians, applied x then y then z) and a translation"""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.concatenate([Rz @ Ry @ Rx, np.asarray(t, float).reshape(3, 1)], axis=1)
