"""50-digit reference of IMU pre-integration (mpmath) and the case list of tests/test_preint_hp.py — TEST INFRASTRUCTURE.

The recursion of bs_common/src/bs_common/preintegrator.cpp:26-143 as beam_slam_amd/csrc/preint_core.h states it — error-state order
(q, p, v, bg, ba), Q / max(dt, 1e-7), the order of the bias-Jacobian updates, mid-point state update and renormalisation, the
Integrate loop with its `> t_end + 1e-12` break and `dt > 1e-12` remainder, the two norm guards, U upper with U^T U = cov^-1 and a
positive diagonal, times info_weight — evaluated in 50 digits on the float64 inputs.  The coefficients sin th / th,
(1 - cos th) / th^2, (th - sin th) / th^3 and the quaternion of a rotation vector are the closed forms, with no small-angle branch
but the exact limit at th == 0: at 50 digits they are good to 20 digits for every float64 th.

mpmath is needed only where the reference is evaluated (tests/golden/make_hp_golden.py and the regeneration test); the expected values
travel as tests/golden/preint_hp.npz.  Inputs are built with +, -, *, / and sqrt from literals and a seeded generator.
"""
import numpy as np

INFO_WEIGHT = 0.7
N_OUT = 287
ANGLES = (0.0, 1e-13, 5e-13, 2e-12, 5e-11, 2e-10, 5e-9, 1.0001e-8, 3e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 0.1, 3.0)
AXIS = np.array([0.48, -0.6, 0.64])                          # generic, unit length (0.2304 + 0.36 + 0.4096 = 1)
DEFAULT_COV = (5.7e-4, 9.4e-4, 3.7e-6, 2.4e-6)               # gyro / accelerometer noise, gyro / accelerometer bias walk
# Scalar covariances of the guard cases, for their 0.1 s interval of 20 samples: (cov_w = cov_a, cov_bg = cov_ba) put the Frobenius
# norm of the 9 x 9 block at about 0.5e-5 (the 1e-5 guard fires) / 2e-5 (it does not) and that of the 6 x 6 block at about 0.5e-9 /
# 2e-9 (guard at 1e-9); calibrated once against the 50-digit norms, which test_guards_have_margin checks.
GUARD_NOISE = {True: 1.742e-5, False: 6.968e-5}
GUARD_WALK = {True: 2.04e-9, False: 8.16e-9}
GROUPS = (("state", 0, 11), ("dq_dbg", 11, 20), ("dp_dbg", 20, 29), ("dp_dba", 29, 38), ("dv_dbg", 38, 47), ("dv_dba", 47, 56),
          ("A", 62, 287))


def _spd(rng, scale):
    M = rng.uniform(-1.0, 1.0, (3, 3))
    return scale * (M @ M.T + 0.3 * np.eye(3))


def cov_sets():
    """(n_sets, 4, 3, 3): 0 the default scalars, 1-2 full random SPD matrices, 3-6 the guard scalars (9 x 9 fires?, 6 x 6 fires?)."""
    eye = np.eye(3)
    sets = [[c * eye for c in DEFAULT_COV]]
    for seed in (1, 2):
        rng = np.random.default_rng([77, seed])
        sets.append([_spd(rng, s) for s in DEFAULT_COV])
    for f9 in (True, False):
        for f6 in (True, False):
            sets.append([GUARD_NOISE[f9] * eye, GUARD_NOISE[f9] * eye, GUARD_WALK[f6] * eye, GUARD_WALK[f6] * eye])
    return np.array(sets)


def _motion(rng, n, rate=0.3):
    """n samples of a slowly varying rotation rate of about `rate` rad/s and a specific force near gravity."""
    w = rate * (AXIS + 0.3 * rng.uniform(-1.0, 1.0, (n, 3)))
    a = np.array([0.3, -0.2, 9.8]) + 0.5 * rng.uniform(-1.0, 1.0, (n, 3))
    return w, a


def build_inputs():
    """The cases, each one interval.  Returns a dict of arrays: t / w / a (all samples), sample_start (n + 1), t_end, bg, ba, cov_id per
    case, covs (cov_sets()), name per case."""
    t_all, w_all, a_all, start, t_end, bgs, bas, cov_id, names = [], [], [], [0], [], [], [], [], []
    bg0, ba0 = np.array([1.5e-3, -0.7e-3, 2.1e-3]), np.array([0.02, -0.013, 0.008])

    def add(name, t, w, a, te, cov=0, bg=bg0, ba=ba0):
        t_all.extend(np.asarray(t, float)); w_all.extend(np.asarray(w, float).reshape(-1, 3)); a_all.extend(np.asarray(a, float).reshape(-1, 3))
        start.append(len(t_all)); t_end.append(float(te)); bgs.append(bg); bas.append(ba); cov_id.append(cov); names.append(name)

    # 1. angle sweep: |w - bg| dt = angle along AXIS, one increment and 20 equal ones
    dt = 0.005
    for ang in ANGLES:
        for n_inc in (1, 20):
            t = dt * np.arange(n_inc + 1)
            w = np.tile(bg0 + AXIS * (ang / dt), (n_inc + 1, 1))
            a = np.tile(ba0 + np.array([0.3, -0.2, 9.8]), (n_inc + 1, 1))
            add(f"angle {ang:g} x{n_inc}", t, w, a, t[-1])
    # 2. noise covariances on one 0.1 s interval of ordinary motion
    rng = np.random.default_rng(31)
    t = dt * np.arange(21)
    w, a = _motion(rng, 21)
    for cs in (1, 2):
        add(f"full covariances {cs}", t, w + bg0, a + ba0, t[-1], cov=cs)
    for k, (f9, f6) in enumerate([(True, True), (True, False), (False, True), (False, False)]):
        add(f"guards 9x9 {'fires' if f9 else 'quiet'} 6x6 {'fires' if f6 else 'quiet'}", t, w + bg0, a + ba0, t[-1], cov=3 + k)
    # 3. sample layouts
    add("no samples", [], [], [], 0.1)
    # (a lone increment leaves the 9 x 9 block at rank 6 — B Q B^T — so it is kept short enough for the norm guard to replace it:
    # above the guard cov^-1 is the inverse of a singular matrix, which no arithmetic pins)
    add("one sample, t_end after it", t[:1], w[:1] + bg0, a[:1] + ba0, 0.004)
    add("t_end on the last sample", t[:9], w[:9] + bg0, a[:9] + ba0, t[8])
    add("t_end between interior samples", t, w + bg0, a + ba0, 0.5 * (t[7] + t[8]))
    add("t_end before the first sample", t[3:], w[3:] + bg0, a[3:] + ba0, t[1])
    t_eq = np.concatenate([t[:6], t[5:10]])
    add("two equal timestamps", t_eq, w[:11] + bg0, a[:11] + ba0, t_eq[-1] + 0.002)
    steps = np.array([1e-4, 5e-2, 3e-4, 2e-2, 1e-4, 1e-3, 4e-2, 5e-4, 7e-3, 2e-4, 5e-2, 1e-4])
    t_nu = np.concatenate([[0.0], np.cumsum(steps)])
    add("non-uniform dt", t_nu, w[:13] + bg0, a[:13] + ba0, t_nu[-1] + 0.011)
    return dict(t=np.array(t_all), w=np.array(w_all).reshape(-1, 3), a=np.array(a_all).reshape(-1, 3),
                sample_start=np.array(start, np.int32), t_end=np.array(t_end), bg=np.array(bgs), ba=np.array(bas),
                cov_id=np.array(cov_id, np.int32), covs=cov_sets(), name=np.array(names))


def case(inp, k):
    """(t, w, a, t_end, bg, ba, covs[4, 3, 3]) of case k."""
    s0, s1 = int(inp["sample_start"][k]), int(inp["sample_start"][k + 1])
    return inp["t"][s0:s1], inp["w"][s0:s1], inp["a"][s0:s1], inp["t_end"][k], inp["bg"][k], inp["ba"][k], inp["covs"][inp["cov_id"][k]]


# ---- 50 digits ---------------------------------------------------------------------------------------------------------------------
def preintegrate_hp(t, w, a, t_end, bg, ba, covs, info_weight):
    """One interval in 50 digits: (out: 287 mpf in the layout of BSGPU_F_IMU_DELTA's consts, n9, n6: the Frobenius norms the two
    guards compare with 1e-5 and 1e-9)."""
    import mpmath as mp
    mp.mp.dps = 50
    f = lambda v: mp.mpf(float(v))
    M = lambda A: mp.matrix([[f(v) for v in row] for row in np.asarray(A, float)])
    vec = lambda v: mp.matrix([f(e) for e in v])
    skew = lambda v: mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    I3 = mp.eye(3)

    def rot(q):
        w_, x, y, z = q
        return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y)],
                          [2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w_ * x)],
                          [2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)]])

    def qmul(p, q):
        return [p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]]

    def quat_of(v):
        th = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
        s = mp.mpf(1) / 2 if th == 0 else mp.sin(th / 2) / th
        return [mp.cos(th / 2), s * v[0], s * v[1], s * v[2]]

    def coeffs(th):
        if th == 0:
            return mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1) / 6
        return mp.sin(th) / th, (1 - mp.cos(th)) / th ** 2, (th - mp.sin(th)) / th ** 3

    Cw, Ca, Cbg, Cba = (M(c) for c in covs)
    bgm, bam = vec(bg), vec(ba)
    st = dict(t=mp.mpf(0), q=[mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)], p=mp.zeros(3, 1), v=mp.zeros(3, 1), cov=mp.zeros(15, 15),
              dq_dbg=mp.zeros(3, 3), dp_dbg=mp.zeros(3, 3), dp_dba=mp.zeros(3, 3), dv_dbg=mp.zeros(3, 3), dv_dba=mp.zeros(3, 3))

    def increment(dt, w_raw, a_raw):
        wv, av = vec(w_raw) - bgm, vec(a_raw) - bam
        wdt = wv * dt
        th = mp.sqrt(wdt[0] ** 2 + wdt[1] ** 2 + wdt[2] ** 2)
        cA, cB, cC = coeffs(th)
        K = skew(wdt)
        K2 = K * K
        R_full = I3 + cA * K + cB * K2
        Jr = I3 - cB * K + cC * K2
        Rdq, Sa = rot(st["q"]), skew(av)
        RS = Rdq * Sa
        A = mp.eye(9)
        B = mp.zeros(9, 6)
        Rt = R_full.T
        for i in range(3):
            for j in range(3):
                A[i, j] = Rt[i, j]
                A[6 + i, j] = -dt * RS[i, j]
                A[3 + i, j] = -dt * dt * RS[i, j] / 2
                A[3 + i, 6 + j] = dt if i == j else 0
                B[i, j] = dt * Jr[i, j]
                B[6 + i, 3 + j] = dt * Rdq[i, j]
                B[3 + i, 3 + j] = dt * dt * Rdq[i, j] / 2
        inv_dt = 1 / max(dt, f(1e-7))
        Q = mp.zeros(6, 6)
        for i in range(3):
            for j in range(3):
                Q[i, j] = Cw[i, j] * inv_dt
                Q[3 + i, 3 + j] = Ca[i, j] * inv_dt
        P9 = A * st["cov"][0:9, 0:9] * A.T + B * Q * B.T
        cov = st["cov"]
        for i in range(9):
            for j in range(9):
                cov[i, j] = P9[i, j]
        for i in range(3):
            for j in range(3):
                cov[9 + i, 9 + j] += dt * Cbg[i, j]
                cov[12 + i, 12 + j] += dt * Cba[i, j]
        RSdq = RS * st["dq_dbg"]
        st["dp_dbg"] = st["dp_dbg"] + dt * st["dv_dbg"] - dt * dt * RSdq / 2
        st["dp_dba"] = st["dp_dba"] + dt * st["dv_dba"] - dt * dt * Rdq / 2
        st["dv_dbg"] = st["dv_dbg"] - dt * RSdq
        st["dv_dba"] = st["dv_dba"] - dt * Rdq
        st["dq_dbg"] = Rt * st["dq_dbg"] - dt * Jr
        amid = rot(qmul(st["q"], quat_of(wdt / 2))) * av
        st["t"] += dt
        st["p"] = st["p"] + dt * st["v"] + dt * dt * amid / 2
        st["v"] = st["v"] + dt * amid
        qn = qmul(st["q"], quat_of(wdt))
        nn = mp.sqrt(sum(e * e for e in qn))
        st["q"] = [e / nn for e in qn]

    te, ts = f(t_end), [f(x) for x in t]
    tiny = f(1e-12)
    for s in range(len(ts) - 1):
        if ts[s + 1] > te + tiny:
            break
        increment(ts[s + 1] - ts[s], w[s], a[s])
    if len(ts) > 0:
        dt = te - ts[-1]
        if dt > tiny:
            increment(dt, w[-1], a[-1])
    cov = st["cov"]
    n9 = mp.sqrt(sum(cov[i, j] ** 2 for i in range(9) for j in range(9)))
    n6 = mp.sqrt(sum(cov[i, j] ** 2 for i in range(9, 15) for j in range(9, 15)))
    if n9 < f(1e-5):
        for i in range(9):
            for j in range(9):
                cov[i, j] = f(1e-5) if i == j else 0
    if n6 < f(1e-9):
        for i in range(9, 15):
            for j in range(9, 15):
                cov[i, j] = f(1e-9) if i == j else 0
    U = mp.cholesky(mp.inverse(cov)).T
    out = [st["t"], *st["q"], *st["p"], *st["v"]]
    for name in ("dq_dbg", "dp_dbg", "dp_dba", "dv_dbg", "dv_dba"):
        out += [st[name][i, j] for i in range(3) for j in range(3)]
    out += [f(e) for e in bg] + [f(e) for e in ba]
    out += [f(info_weight) * U[i, j] for i in range(15) for j in range(15)]
    assert len(out) == N_OUT
    return out, n9, n6


def evaluate(inp):
    """hp_hi / hp_lo (n x 287: the 50-digit value as a float64 pair, hi the rounded value) and hp_n9 / hp_n6, the guards' norms."""
    import mpmath as mp
    n = len(inp["t_end"])
    out = dict(hp_hi=np.zeros((n, N_OUT)), hp_lo=np.zeros((n, N_OUT)), hp_n9=np.zeros(n), hp_n6=np.zeros(n))
    for k in range(n):
        o, n9, n6 = preintegrate_hp(*case(inp, k), INFO_WEIGHT)
        for i, x in enumerate(o):
            hi = float(x)
            out["hp_hi"][k, i], out["hp_lo"][k, i] = hi, float(x - mp.mpf(hi))
        out["hp_n9"][k], out["hp_n6"][k] = float(n9), float(n6)
    return out


def error(got, hi, lo):
    """|got - (hi + lo)| entrywise: (got - hi) is exact wherever it matters, so the reference's rounding to float64 does not enter."""
    return np.abs((np.asarray(got) - hi) - lo)
