"""IMU pre-integration against a 50-digit reference (tests/preint_hp.py), on the CPU through beam_slam_amd/csrc/preint_core.h
(tests/plan/test_preint.cpp) and on the device through bsgpu_preintegrate.  info_weight = 0.7, single intervals:

* angle sweep: |w - b_g| dt in {0, 1e-13, 5e-13, 2e-12, 5e-11, 2e-10, 5e-9, 1.0001e-8, 3e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 0.1, 3} along a
  generic axis, as one increment and as 20 equal ones — across the reference's small-angle thresholds 1e-12, 1e-10 and 1e-8;
* full random SPD 3 x 3 noise covariances; scalar ones that put either norm guard of ComputeSqrtInvCov on either side of its threshold
  (never within a relative 1e-3 of it, checked on the 50-digit norms);
* sample layouts: no samples, one sample, t_end on a sample, t_end between interior samples (the early break, remainder skipped), t_end
  before the first sample, two equal timestamps (dt == 0), dt from 1e-4 to 5e-2;
* batches of 1, 64 and 65 intervals (the launch boundary of 64 lanes), each row the bits of its lone call; n = 0.

Tolerance, per case and per output group (dt dq dp dv; each of the five bias Jacobians; A): 16 x the error of `yardstick` below — the
same recursion in float64 numpy with cancellation-free coefficients, 1 - cos th = 2 sin^2(th / 2) and series for sin th / th and
(th - sin th) / th^3 below th^2 < 1e-4 — against the 50-digit values, floor 4e-16 x the group's largest entry.  For A the yardstick's
error carries the condition number of the covariance.

Measured.  Largest error / bound over all cases: core (CPU) 0.21 (group A), kernel (MI355X) 0.33 (group state); the yardstick sits
at 1 / 16 = 0.0625 by construction.  Entrywise error of the right Jacobian (error of dq_dbg / dt after one increment), parent
commit's coefficients through the same driver against the header and the kernel:
    |w - b_g| dt   parent (CPU)   core (CPU)   kernel (MI355X)
    5e-9           3.2e-18        3.2e-18      3.2e-18
    1.0001e-8      3.2e-09        1.3e-17      1.3e-17
    3e-8           1.3e-10        8.5e-17      8.5e-17
    1e-7           2.6e-11        1.1e-16      1.1e-16
    1e-6           2.8e-11        7.1e-17      7.1e-17
    1e-5           2.6e-13        1.2e-16      1.2e-16
    1e-4           1.7e-13        5.4e-17      5.4e-17
    1e-3           5.0e-15        6.6e-17      6.6e-17
    0.1            3.6e-16        2.9e-17      2.9e-17
    3              8.3e-17        9.7e-17      9.7e-17
With the parent's coefficients test_core_against_50_digits fails from 1.0001e-8 (8e6 x the bound) to 1e-3 (4.8 x) and in four of the
sample-layout cases (their angles are about 1.5e-3); below 1e-8 and from 0.1 on it passes.
"""
import os
import subprocess

import numpy as np
import pytest

import preint_hp as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the float64 yardstick -----------------------------------------------------------------------------------------------------
def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _coeffs(th):
    """sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3 without cancellation."""
    if th == 0.0:
        return 1.0, 0.5, 1.0 / 6.0
    u = th * th
    sh = np.sin(0.5 * th) / th
    if u < 1e-4:
        return (1.0 - u / 6.0 * (1.0 - u / 20.0 * (1.0 - u / 42.0 * (1.0 - u / 72.0))), 2.0 * sh * sh,
                1.0 / 6.0 * (1.0 - u / 20.0 * (1.0 - u / 42.0 * (1.0 - u / 72.0 * (1.0 - u / 110.0)))))
    return np.sin(th) / th, 2.0 * sh * sh, (th - np.sin(th)) / (u * th)


def _quat_of(v):
    th = np.sqrt(v @ v)
    s = 0.5 if th == 0.0 else np.sin(0.5 * th) / th
    return np.array([np.cos(0.5 * th), *(s * v)])


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def yardstick(t, w, a, t_end, bg, ba, covs, info_weight):
    """preintegrator.cpp:26-143 for one interval in float64 -> the 287 consts of BSGPU_F_IMU_DELTA."""
    Cw, Ca, Cbg, Cba = covs
    tt, q, p, v, cov = 0.0, np.array([1.0, 0, 0, 0]), np.zeros(3), np.zeros(3), np.zeros((15, 15))
    dq_dbg, dp_dbg, dp_dba, dv_dbg, dv_dba = (np.zeros((3, 3)) for _ in range(5))

    def increment(dt, w_raw, a_raw):
        nonlocal tt, q, p, v, dq_dbg, dp_dbg, dp_dba, dv_dbg, dv_dba
        wv, av = w_raw - bg, a_raw - ba
        wdt = wv * dt
        cA, cB, cC = _coeffs(np.sqrt(wdt @ wdt))
        K = _skew(wdt)
        R_full, Jr = np.eye(3) + cA * K + cB * K @ K, np.eye(3) - cB * K + cC * K @ K
        Rdq = _rot(q)
        RS = Rdq @ _skew(av)
        A, B = np.eye(9), np.zeros((9, 6))
        A[0:3, 0:3], A[6:9, 0:3], A[3:6, 0:3], A[3:6, 6:9] = R_full.T, -dt * RS, -0.5 * dt * dt * RS, dt * np.eye(3)
        B[0:3, 0:3], B[6:9, 3:6], B[3:6, 3:6] = dt * Jr, dt * Rdq, 0.5 * dt * dt * Rdq
        Q = np.zeros((6, 6))
        Q[0:3, 0:3], Q[3:6, 3:6] = Cw / max(dt, 1e-7), Ca / max(dt, 1e-7)
        cov[0:9, 0:9] = A @ cov[0:9, 0:9] @ A.T + B @ Q @ B.T
        cov[9:12, 9:12] += dt * Cbg
        cov[12:15, 12:15] += dt * Cba
        RSdq = RS @ dq_dbg
        dp_dbg = dp_dbg + dt * dv_dbg - 0.5 * dt * dt * RSdq
        dp_dba = dp_dba + dt * dv_dba - 0.5 * dt * dt * Rdq
        dv_dbg = dv_dbg - dt * RSdq
        dv_dba = dv_dba - dt * Rdq
        dq_dbg = R_full.T @ dq_dbg - dt * Jr
        amid = _rot(_qmul(q, _quat_of(0.5 * wdt))) @ av
        tt += dt
        p = p + dt * v + 0.5 * dt * dt * amid
        v = v + dt * amid
        qn = _qmul(q, _quat_of(wdt))
        q = qn / np.sqrt(qn @ qn)

    for s in range(len(t) - 1):
        if t[s + 1] > t_end + 1e-12:
            break
        increment(t[s + 1] - t[s], w[s], a[s])
    if len(t) > 0 and t_end - t[-1] > 1e-12:
        increment(t_end - t[-1], w[-1], a[-1])
    if np.linalg.norm(cov[0:9, 0:9]) < 1e-5:
        cov[0:9, 0:9] = 1e-5 * np.eye(9)
    if np.linalg.norm(cov[9:15, 9:15]) < 1e-9:
        cov[9:15, 9:15] = 1e-9 * np.eye(6)
    try:
        U = np.linalg.cholesky(np.linalg.inv(cov)).T
        if not np.isfinite(U).all():
            raise np.linalg.LinAlgError
    except np.linalg.LinAlgError:
        U = 1e-4 * np.eye(15)
    return np.concatenate([[tt], q, p, v, dq_dbg.ravel(), dp_dbg.ravel(), dp_dba.ravel(), dv_dbg.ravel(), dv_dba.ravel(), bg, ba,
                           (info_weight * U).ravel()])


def yardstick_all(inp):
    return np.stack([yardstick(*hp.case(inp, k), hp.INFO_WEIGHT) for k in range(len(inp["t_end"]))])


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(ROOT, "tests", "golden", "preint_hp.npz")) as z:
        return {k: z[k] for k in z.files}


def _call_arrays(fx, cases):
    """The arguments of one bsgpu_preintegrate call on the cases (all of one covariance set): sample_start, t, w, a, t_end, bg, ba."""
    parts = [hp.case(fx, k) for k in cases]
    ss = np.concatenate([[0], np.cumsum([len(c[0]) for c in parts])]).astype(np.int32)
    cat = lambda i, shape: np.concatenate([np.asarray(c[i], float).reshape(shape) for c in parts] + [np.zeros((0,) + shape[1:])])
    return ss, cat(0, (-1,)), cat(1, (-1, 3)), cat(2, (-1, 3)), np.array([c[3] for c in parts]), cat(4, (-1, 3)), cat(5, (-1, 3))


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("preint") / "test_preint")
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                          os.path.join(ROOT, "tests", "plan", "test_preint.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]

    def run(fx, calls, tmp_path):
        """calls: [(covariance set, [cases])] -> [n x 287 per call]"""
        f = lambda v: " ".join(repr(float(x)) for x in np.ravel(v))
        lines = []
        for cs, cases in calls:
            ss, t, w, a, te, bg, ba = _call_arrays(fx, cases)
            lines += [f"PREINT {len(cases)} {len(t)} {hp.INFO_WEIGHT!r}", f(fx["covs"][cs]), " ".join(str(int(s)) for s in ss)]
            lines += [f([t[i], *w[i], *a[i]]) for i in range(len(t))]
            lines += [f([te[i], *bg[i], *ba[i]]) for i in range(len(cases))]
        path = tmp_path / "commands.txt"
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and f"DONE {len(calls)}" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        res = [[] for _ in calls]
        for ln in r.stdout.splitlines():
            tok = ln.split()
            if tok[0] == "OUT":
                assert int(tok[2]) == len(res[int(tok[1])])
                res[int(tok[1])].append([float(v) for v in tok[3:]])
        return [np.array(rows).reshape(-1, hp.N_OUT) for rows in res]
    return run


def _device(fx, cs, cases):
    from beam_slam_amd import gpu
    ss, t, w, a, te, bg, ba = _call_arrays(fx, cases)
    return gpu.preintegrate(ss, t, w, a, te, bg, ba, *fx["covs"][cs], info_weight=hp.INFO_WEIGHT)


def _check(fx, cases, out, who):
    """Every row of out against the 50-digit values of its case; returns {group: largest error / bound}."""
    worst = {}
    assert out.shape == (len(cases), hp.N_OUT)
    for row, k in zip(out, cases):
        assert np.array_equal(row[56:62], np.concatenate([fx["bg"][k], fx["ba"][k]]))
        A = row[62:].reshape(15, 15)
        assert np.array_equal(A, np.triu(A)) and (np.diag(A) > 0).all()
        err, e_y = hp.error(row, fx["hp_hi"][k], fx["hp_lo"][k]), hp.error(fx["yard"][k], fx["hp_hi"][k], fx["hp_lo"][k])
        for name, lo, hi in hp.GROUPS:
            bound = max(16.0 * e_y[lo:hi].max(), 4e-16 * np.abs(fx["hp_hi"][k][lo:hi]).max())
            e = err[lo:hi].max()
            print(f"{who}: {fx['name'][k]:<40s} {name:<7s} yardstick {e_y[lo:hi].max():.3e} error {e:.3e} bound {bound:.3e}")
            assert e <= bound, (who, str(fx["name"][k]), name, e, bound)
            if bound > 0:
                worst[name] = max(worst.get(name, 0.0), e / bound)
    return worst


def _by_cov(fx):
    return [(cs, [int(k) for k in np.flatnonzero(fx["cov_id"] == cs)]) for cs in range(len(fx["covs"]))]


# ---- tests -----------------------------------------------------------------------------------------------------------------------
def test_case_list(fx):
    """The sweep straddles the three thresholds with single and 20-fold increments, every layout is present, and the covariance sets
    are what their names say: symmetric positive definite, sets 1 and 2 full."""
    names = [str(n) for n in fx["name"]]
    assert len(names) == len(set(names)) == 2 * len(hp.ANGLES) + 6 + 7
    for lo, hi in ((0.0, 1e-12), (1e-12, 1e-10), (1e-10, 1e-8), (1e-8, 1e-5), (1e-5, 4.0)):
        assert sum(lo < a < hi for a in hp.ANGLES) >= 2, (lo, hi)
    assert sum(0.0 < 0.5 * a < 1e-12 for a in hp.ANGLES) >= 2 and hp.ANGLES[0] == 0.0
    for cs, cases in _by_cov(fx):
        assert cases
        for C in fx["covs"][cs]:
            assert np.array_equal(C, C.T) and np.linalg.eigvalsh(C).min() > 0
            assert (np.count_nonzero(C) == 9) == (cs in (1, 2))
    n_samples = np.diff(fx["sample_start"])
    assert n_samples.min() == 0 and (n_samples == 1).sum() == 1
    k = names.index("two equal timestamps")
    assert (np.diff(hp.case(fx, k)[0]) == 0.0).sum() == 1
    k = names.index("non-uniform dt")
    d = np.diff(hp.case(fx, k)[0])
    assert abs(d.min() - 1e-4) < 1e-12 and abs(d.max() - 5e-2) < 1e-12


def test_guards_have_margin(fx):
    """No case within a relative 1e-3 of a guard threshold (50-digit norms); each guard fires and stays quiet in the cases named so."""
    assert (np.abs(fx["hp_n9"] - 1e-5) >= 1e-3 * 1e-5).all() and (np.abs(fx["hp_n6"] - 1e-9) >= 1e-3 * 1e-9).all()
    for k, name in enumerate(str(n) for n in fx["name"]):
        if name.startswith("guards"):
            assert (fx["hp_n9"][k] < 1e-5) == ("9x9 fires" in name) and (fx["hp_n6"][k] < 1e-9) == ("6x6 fires" in name), name
            assert 0.4e-5 < fx["hp_n9"][k] < 2.5e-5 and 0.4e-9 < fx["hp_n6"][k] < 2.5e-9, name
        elif name.startswith(("no samples", "t_end before")):              # nothing integrated: both fire
            assert fx["hp_n9"][k] == 0.0 and fx["hp_n6"][k] == 0.0, name
        elif name.endswith("x1") or name.startswith("one sample"):          # one increment of 5 ms or less: the 9 x 9 guard fires
            assert fx["hp_n9"][k] < 1e-5 and fx["hp_n6"][k] > 1e-9, name
        else:
            assert fx["hp_n9"][k] > 1e-5 and fx["hp_n6"][k] > 1e-9, name


def test_fixture_matches_its_generator(fx):
    """The inputs and every 50-digit entry of tests/golden/preint_hp.npz, regenerated: the same bits.  The yardstick goes through
    LAPACK (inverse, Cholesky), whose last bits belong to the library build: it must reproduce within the bound it sets."""
    pytest.importorskip("mpmath")
    inp = hp.build_inputs()
    for k, v in inp.items():
        assert v.dtype == fx[k].dtype and v.tobytes() == fx[k].tobytes(), k
    out = hp.evaluate(inp)
    for k, v in out.items():
        assert v.dtype == fx[k].dtype and v.tobytes() == fx[k].tobytes(), k
    _check(fx, list(range(len(inp["t_end"]))), yardstick_all(inp), "yardstick")


def test_core_against_50_digits(fx, core, tmp_path):
    """Every case through the header on the CPU, one command per covariance set.  Measured: see the module docstring."""
    calls = _by_cov(fx)
    worst = {}
    for (cs, cases), out in zip(calls, core(fx, calls, tmp_path)):
        for g, r in _check(fx, cases, out, "core").items():
            worst[g] = max(worst.get(g, 0.0), r)
    print("core: largest error / bound per group:", {g: round(r, 3) for g, r in worst.items()})


def _batches(fx):
    base = [int(k) for k in np.flatnonzero(fx["cov_id"] == 0)]
    return base, [[base[(7 * i) % len(base)] for i in range(n)] for n in (64, 65)]


def test_core_batches_equal_lone_calls(fx, core, tmp_path):
    base, batches = _batches(fx)
    res = core(fx, [(0, [k]) for k in base] + [(0, b) for b in batches] + [(0, [])], tmp_path)
    lone = {k: res[i][0] for i, k in enumerate(base)}
    for b, out in zip(batches, res[len(base):]):
        assert out.shape[0] == len(b)
        assert all(out[i].tobytes() == lone[k].tobytes() for i, k in enumerate(b))
    assert res[-1].shape == (0, hp.N_OUT)


@pytest.mark.gpu
@pytest.mark.parametrize("cs", range(7))
def test_device_against_50_digits(fx, cs):
    """One bsgpu_preintegrate call per covariance set.  Measured: see the module docstring."""
    cases = _by_cov(fx)[cs][1]
    worst = _check(fx, cases, _device(fx, cs, cases), "kernel")
    print("kernel: covariance set", cs, "largest error / bound per group:", {g: round(r, 3) for g, r in worst.items()})


@pytest.mark.gpu
def test_device_batches_equal_lone_calls(fx):
    """1, 64 and 65 intervals (one lane in a second workgroup of 64): every row is the bits of its lone call; n = 0 returns cleanly."""
    base, batches = _batches(fx)
    lone = {k: _device(fx, 0, [k])[0] for k in base}
    for b in batches:
        out = _device(fx, 0, b)
        assert out.shape == (len(b), hp.N_OUT)
        assert all(out[i].tobytes() == lone[k].tobytes() for i, k in enumerate(b))
    assert _device(fx, 0, []).shape == (0, hp.N_OUT)
