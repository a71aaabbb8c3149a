"""50-digit reference of landmark triangulation (mpmath) and the seeded track generator of tests/test_triangulation_hp.py —
TEST INFRASTRUCTURE.  The same definition as oracle/triangulation.py: T_camera_world from the un-normalised quaternion, unit bearings,
the 2V x 4 DLT matrix A, the right singular vector of its smallest singular value (mp.svd_r), de-homogenised; then, per view, the
camera-frame depth, the range and the re-projection distance the three rejection tests look at.

mpmath is needed only where the reference is evaluated (tests/golden/make_hp_golden.py and the regeneration test); the expected values
travel as tests/golden/triangulation_hp.npz.  Every input is built from the seeded generator with +, -, *, / and sqrt alone, so it is
the same float64 number on every IEEE machine.
"""
import numpy as np

OFFSET_DIR = np.array([0.6, -0.64, 0.48])                     # a generic direction of unit length (0.36 + 0.4096 + 0.2304 = 1)
OFFSETS = (0.0, 1e2, 1e3, 1e4, 1e5)                           # metres, of the whole scene along OFFSET_DIR
PARALLAX = ((0.5, 6.0), (0.05, 30.0), (0.01, 30.0))           # (baseline, depth) in metres
VIEWS = (2, 3, 12, 40)
SEEDS = 8
MAX_DIST, MAX_REPROJ = 80.0, 3.0                              # of every call of the grid
N_CALL = 257                                                  # tracks per call: one lane in a second workgroup of 256
MARGIN = 1e-6                                                 # every decision at least this far (relative) from its threshold


def camera_row():
    from beam_slam_amd import synthetic
    R, t = synthetic._t_cam_baselink()
    return np.array([synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY, *R.ravel(), *t])


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _project(q, p, cam, P):
    K, R_cb, t_cb = cam[:4], cam[4:13].reshape(3, 3), cam[13:16]
    R = R_cb @ _rot(q).T
    pc = R @ (P - p) + t_cb
    return np.array([K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]])


def _keyframes(rng, n, centre, baseline, cam):
    """n keyframes (q, p): rotations of up to ~0.3 rad, camera centres spread over `baseline` across the viewing direction."""
    R_cb, t_cb = cam[4:13].reshape(3, 3), cam[13:16]
    out = []
    for i in range(n):
        v = rng.uniform(-1.0, 1.0, 3)
        v *= rng.uniform(0.0, 0.15) / np.sqrt(v @ v)           # q = (1, tan(angle / 2) axis) normalised: angle <= 0.3 rad
        q = np.array([1.0, *v])
        q /= np.sqrt(q @ q)
        lat = np.array([(i / (n - 1) - 0.5), 0.3 * rng.uniform(-0.5, 0.5), 0.2 * rng.uniform(-0.5, 0.5)]) * baseline
        c = centre + R_cb.T @ lat                               # camera centre: lateral (x), a little vertical and along the axis
        p = c + _rot(q) @ (R_cb.T @ t_cb)                       # body position that puts the camera centre at c
        out.append((q, p))
    return out


def _point(rng, centre, depth, cam):
    R_cb = cam[4:13].reshape(3, 3)
    return centre + R_cb.T @ (np.array([rng.uniform(-0.25, 0.25), rng.uniform(-0.15, 0.15), 1.0]) * depth)


def build_inputs():
    """All tracks of the suite.  Returns a dict of arrays:
    camera (16); values (keyframe blocks q[4] p[3]); q_off / p_off / pixels per observation; track_start; per track: offset_id, cell
    (index into the offset x parallax x views grid, -1 for the deliberate status tracks) and kind (0 grid, 2 / 3 / 4 the status the
    track was built for)."""
    cam = camera_row()
    values, q_off, p_off, pixels, start, off_id, cell, kind = [], [], [], [], [0], [], [], []

    def add_kf(kfs):
        offs = []
        for q, p in kfs:
            offs.append(len(values))
            values.extend([*q, *p])
        return offs

    def add_track(offs, px, oi, ce, ki):
        for o, z in zip(offs, px):
            q_off.append(o); p_off.append(o + 4); pixels.append(z)
        start.append(len(q_off)); off_id.append(oi); cell.append(ce); kind.append(ki)

    for oi, off in enumerate(OFFSETS):
        centre = off * OFFSET_DIR
        for pi, (b, d) in enumerate(PARALLAX):
            for vi, nv in enumerate(VIEWS):
                rng = np.random.default_rng([2024, oi, pi, vi])
                kfs = _keyframes(rng, nv, centre, b, cam)
                offs = add_kf(kfs)
                for _ in range(SEEDS):
                    P = _point(rng, centre, d, cam)
                    add_track(offs, [_project(q, p, cam, P) for q, p in kfs], oi, (oi * len(PARALLAX) + pi) * len(VIEWS) + vi, 0)
        # deliberate rejections: 3 of each kind
        rng = np.random.default_rng([2025, oi])
        for k in range(3):
            kfs = _keyframes(rng, 2, centre, 1.0, cam)          # the lines of sight meet 6 m behind the cameras
            P = _point(rng, centre, -6.0, cam)
            add_track(add_kf(kfs), [_project(q, p, cam, P) for q, p in kfs], oi, -1, 2)
            kfs = _keyframes(rng, 3, centre, 5.0, cam)          # 200 m away, MAX_DIST is 80
            P = _point(rng, centre, 200.0, cam)
            add_track(add_kf(kfs), [_project(q, p, cam, P) for q, p in kfs], oi, -1, 3)
            kfs = _keyframes(rng, 3, centre, 1.0, cam)          # the last view looks at a point 0.5 m aside: tens of pixels
            P = _point(rng, centre, 6.0, cam)
            px = [_project(q, p, cam, P) for q, p in kfs[:2]] + [_project(*kfs[2], cam, P + 0.5 * OFFSET_DIR[[1, 0, 2]])]
            add_track(add_kf(kfs), px, oi, -1, 4)
    return dict(camera=cam, values=np.array(values), q_off=np.array(q_off, np.int32), p_off=np.array(p_off, np.int32),
                pixels=np.array(pixels), track_start=np.array(start, np.int32), offset_id=np.array(off_id, np.int32),
                cell=np.array(cell, np.int32), kind=np.array(kind, np.int32))


def call_layout(inp, oi):
    """The N_CALL tracks of offset oi's call: an empty track, a single-view track, every track of the offset, then the offset's grid
    tracks again until the call is full.  Returns (track_start, obs) — obs indexes the observations of `inp` — and src, the track of
    `inp` behind each track of the call (-1 for the two in front)."""
    tr = np.flatnonzero(inp["offset_id"] == oi)
    grid = tr[inp["cell"][tr] >= 0]
    src = [-1, -1] + list(tr)
    while len(src) < N_CALL:
        src.append(int(grid[(len(src) * 7) % len(grid)]))
    ts = inp["track_start"]
    first = int(ts[tr[0]])
    obs, start = [first], [0, 0, 1]
    for s in src[2:]:
        obs.extend(range(int(ts[s]), int(ts[s + 1])))
        start.append(len(obs))
    return np.array(start, np.int32), np.array(obs), np.array(src)


# ---- 50 digits ---------------------------------------------------------------------------------------------------------------------
def triangulate_hp(cam, views, truncate, max_dist, max_reproj):
    """views: [(q[4], p[3], pixel[2])] in float64.  Returns (P (3 mpf, None at infinity), status, margin): status as
    oracle/triangulation.py decides it but in 50 digits, margin the smallest relative distance of a quantity that took part in the
    decision from its threshold (depth against 0, relative to the range)."""
    import mpmath as mp
    mp.mp.dps = 50
    f = lambda v: mp.mpf(float(v))
    fx, fy, cx, cy = (f(v) for v in cam[:4])
    R_cb = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            R_cb[i, j] = f(cam[4 + 3 * i + j])
    t_cb = mp.matrix([f(v) for v in cam[13:16]])
    if len(views) < 2:
        return None, 1, 1.0
    Ts, zs = [], []
    A = mp.matrix(2 * len(views), 4)
    for k, (q, p, z) in enumerate(views):
        w, x, y, zq = (f(v) for v in q)
        Rwb = mp.matrix([[1 - 2 * (y * y + zq * zq), 2 * (x * y - w * zq), 2 * (x * zq + w * y)],
                         [2 * (x * y + w * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - w * x)],
                         [2 * (x * zq - w * y), 2 * (y * zq + w * x), 1 - 2 * (x * x + y * y)]])
        R = R_cb * Rwb.T
        t = t_cb - R * mp.matrix([f(v) for v in p])
        T = mp.matrix(3, 4)
        for i in range(3):
            for j in range(3):
                T[i, j] = R[i, j]
            T[i, 3] = t[i]
        u, v = (f(np.trunc(z[0])), f(np.trunc(z[1]))) if truncate else (f(z[0]), f(z[1]))
        m = [(u - cx) / fx, (v - cy) / fy, mp.mpf(1)]
        n = mp.sqrt(m[0] ** 2 + m[1] ** 2 + 1)
        m = [e / n for e in m]
        for j in range(4):
            A[2 * k, j] = m[0] * T[2, j] - m[2] * T[0, j]
            A[2 * k + 1, j] = m[1] * T[2, j] - m[2] * T[1, j]
        Ts.append(T); zs.append((u, v))
    _, S, V = mp.svd_r(A, full_matrices=False, compute_uv=True)
    assert all(S[i] >= S[i + 1] for i in range(3))
    h = [V[3, j] for j in range(4)]
    if h[3] == 0:
        return None, 5, 1.0
    P = [h[j] / h[3] for j in range(3)]
    status, margin = 0, mp.inf
    for T, (u, v) in zip(Ts, zs):
        pc = [T[i, 0] * P[0] + T[i, 1] * P[1] + T[i, 2] * P[2] + T[i, 3] for i in range(3)]
        rng_ = mp.sqrt(pc[0] ** 2 + pc[1] ** 2 + pc[2] ** 2)
        margin = min(margin, abs(pc[2]) / rng_)
        if pc[2] < 0:
            status = 2
            break
        if max_dist > 0:
            margin = min(margin, abs(rng_ - max_dist) / max_dist)
            if rng_ > max_dist:
                status = 3
                break
        if max_reproj > 0:
            e = mp.sqrt((u - (fx * pc[0] / pc[2] + cx)) ** 2 + (v - (fy * pc[1] / pc[2] + cy)) ** 2)
            margin = min(margin, abs(e - max_reproj) / max_reproj)
            if not e <= max_reproj:
                status = 4
                break
    return P, status, float(margin)


def split(x):
    """An mpf as the float64 pair (hi, lo), hi the rounded value: hi + lo holds 100 bits of it."""
    import mpmath as mp
    hi = float(x)
    return hi, float(x - mp.mpf(hi))


def views_of(inp, track):
    ts, v = inp["track_start"], inp["values"]
    return [(v[inp["q_off"][o]:inp["q_off"][o] + 4], v[inp["p_off"][o]:inp["p_off"][o] + 3], inp["pixels"][o])
            for o in range(int(ts[track]), int(ts[track + 1]))]


def evaluate(inp):
    """The 50-digit results and the float64 yardstick (oracle/triangulation.py) of every track, exact and truncated pixels.
    Arrays indexed [truncate, track]: hp_hi / hp_lo (3), hp_status, hp_margin, ref (3), ref_status, e_ref (largest coordinate error of
    the yardstick against the 50-digit point, evaluated in 50 digits)."""
    import mpmath as mp
    import triangulation as tri
    cam = inp["camera"]
    K, R_cb, t_cb = cam[:4], cam[4:13].reshape(3, 3), cam[13:16]
    n = len(inp["track_start"]) - 1
    out = dict(hp_hi=np.zeros((2, n, 3)), hp_lo=np.zeros((2, n, 3)), hp_status=np.zeros((2, n), np.int32), hp_margin=np.zeros((2, n)),
               ref=np.zeros((2, n, 3)), ref_status=np.zeros((2, n), np.int32), e_ref=np.zeros((2, n)))
    for t in range(n):
        views = views_of(inp, t)
        Ts = [tri.camera_from_world(q, p, R_cb, t_cb) for q, p, _ in views]
        for tr in (0, 1):
            P, st, margin = triangulate_hp(cam, views, bool(tr), MAX_DIST, MAX_REPROJ)
            px = [np.trunc(z) if tr else z for _, _, z in views]
            ref, ref_st = tri.triangulate_point(Ts, px, K, MAX_DIST, MAX_REPROJ)
            out["hp_status"][tr, t], out["hp_margin"][tr, t] = st, margin
            out["ref"][tr, t], out["ref_status"][tr, t] = ref, ref_st
            if P is not None:
                for j in range(3):
                    out["hp_hi"][tr, t, j], out["hp_lo"][tr, t, j] = split(P[j])
                out["e_ref"][tr, t] = float(max(abs(mp.mpf(float(ref[j])) - P[j]) for j in range(3)))
    return out


def error(got, hi, lo):
    """Largest coordinate error of float64 points against the 50-digit ones kept as (hi, lo): (got - hi) is exact wherever it matters
    (Sterbenz), so the rounding of the reference to float64 does not enter."""
    return np.abs((np.asarray(got) - hi) - lo).max(axis=-1)
