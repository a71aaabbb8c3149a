"""Independent restatement of the Unicycle3D kinematic constraint (BSGPU_F_UNICYCLE) for the tests.

Forward-mode dual numbers over the 32 ambient parameters of one factor (p1, q1, v1, w1, a1, p2, q2, v2, w2, a2), written from
bs_constraints motion/unicycle_3d_state_cost_functor.h:65-125 and unicycle_3d_predict.h:49-196 — what ceres::AutoDiffCostFunction
computes — times the PlusJacobian of each orientation block; [EXT] fuse_core getRoll/getPitch/getYaw and wrapAngle2D.  Also a dense
Gauss-Newton reference that stacks these rows with the oracle's evaluate(jacobian=True) of every other factor."""
import ctypes
import math
import os
import subprocess

import numpy as np

from beam_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMB = [3, 4, 3, 3, 3, 3, 4, 3, 3, 3]
AOFF = np.concatenate([[0], np.cumsum(AMB)])


class D:
    """a + b eps, b over the 32 ambient parameters"""
    __slots__ = ("a", "b")

    def __init__(self, a, b=None):
        self.a = float(a)
        self.b = np.zeros(32) if b is None else b

    @staticmethod
    def _c(o):
        return o if isinstance(o, D) else D(o)

    def __add__(self, o):
        o = D._c(o)
        return D(self.a + o.a, self.b + o.b)
    __radd__ = __add__

    def __sub__(self, o):
        o = D._c(o)
        return D(self.a - o.a, self.b - o.b)

    def __rsub__(self, o):
        return D._c(o) - self

    def __neg__(self):
        return D(-self.a, -self.b)

    def __mul__(self, o):
        o = D._c(o)
        return D(self.a * o.a, self.a * o.b + o.a * self.b)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = D._c(o)
        return D(self.a / o.a, (self.b * o.a - self.a * o.b) / (o.a * o.a))

    def __rtruediv__(self, o):
        return D._c(o) / self


def dsin(x): return D(math.sin(x.a), math.cos(x.a) * x.b)
def dcos(x): return D(math.cos(x.a), -math.sin(x.a) * x.b)
def dasin(x): return D(math.asin(x.a), x.b / math.sqrt(1.0 - x.a * x.a))


def datan2(y, x):   # ceres Jet atan2(g, f): (f dg - g df) / (f^2 + g^2)
    return D(math.atan2(y.a, x.a), (x.a * y.b - y.a * x.b) / (x.a * x.a + y.a * y.a))


def wrap(x):        # [EXT] fuse_core::wrapAngle2D, [-pi, pi); derivative 1
    return D(x.a - 2.0 * math.pi * math.floor((x.a + math.pi) / (2.0 * math.pi)), x.b)


def rpy(w, x, y, z):
    roll = datan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y))
    s = 2.0 * (w * y - z * x)
    pitch = D(math.copysign(math.pi / 2.0, s.a) if s.a != 0 else 0.0) if abs(s.a) >= 1.0 else dasin(s)
    yaw = datan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))
    return roll, pitch, yaw


def error_dual(x32, dt):
    """the 15 unweighted errors as duals over the ambient parameters"""
    v = [D(x32[i], np.eye(32)[i]) for i in range(32)]
    p1, q1, v1, w1, a1, p2, q2, v2, w2, a2 = [v[AOFF[k]:AOFF[k + 1]] for k in range(10)]
    r1, pt1, y1 = rpy(*q1)
    sp, cp = dsin(pt1), dcos(pt1)
    cpi = 1.0 / cp
    tp = sp * cpi
    sr, cr, sy, cy = dsin(r1), dcos(r1), dsin(y1), dcos(y1)
    R = [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
         [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
         [-1.0 * sp, cp * sr, cp * cr]]
    pp = [p1[i] + sum((v1[j] * (R[i][j] * dt) for j in range(3)), D(0.0)) + sum((a1[j] * (0.5 * (R[i][j] * dt) * dt) for j in range(3)), D(0.0))
          for i in range(3)]
    VR, VP, VY = w1
    roll = wrap(r1 + VR * dt + VP * (sr * tp * dt) + VY * (cr * tp * dt))
    pitch = wrap(pt1 + VP * (cr * dt) + VY * (-1.0 * sr * dt))
    yaw = wrap(y1 + VP * (sr * cpi * dt) + VY * (cr * cpi * dt))
    r2, pt2, y2 = rpy(*q2)
    e = [p2[i] - pp[i] for i in range(3)]
    e += [wrap(r2 - roll), wrap(pt2 - pitch), wrap(y2 - yaw)]
    e += [v2[i] - (v1[i] + a1[i] * dt) for i in range(3)]
    e += [w2[i] - w1[i] for i in range(3)]
    e += [a2[i] - a1[i] for i in range(3)]
    return e


def plus_jacobian(q):
    w, x, y, z = q
    return 0.5 * np.array([[-x, -y, -z], [w, -z, y], [z, w, -x], [-y, x, w]])


def tangent_map(x32):
    """32 x 30: the ambient-to-tangent chain (identity on Euclidean blocks, the PlusJacobian on q1 and q2)"""
    M = np.zeros((32, 30))
    for k in range(10):
        if AMB[k] == 4:
            M[AOFF[k]:AOFF[k + 1], 3 * k:3 * k + 3] = plus_jacobian(x32[AOFF[k]:AOFF[k + 1]])
        else:
            M[AOFF[k]:AOFF[k + 1], 3 * k:3 * k + 3] = np.eye(3)
    return M


def error_and_jacobian(x32, dt):
    """unweighted e (15) and its tangent Jacobian (15 x 30)"""
    e = error_dual(np.asarray(x32, float), dt)
    return np.array([d.a for d in e]), np.stack([d.b for d in e]) @ tangent_map(x32)


def quat_plus(q, d):
    th = np.linalg.norm(d)
    dq = np.array([1.0, 0, 0, 0]) if th == 0 else np.concatenate([[math.cos(th / 2)], math.sin(th / 2) / th * d])
    w, x, y, z = q
    a, b, c, e = dq
    return np.array([w * a - x * b - y * c - z * e, w * b + x * a + y * e - z * c, w * c - x * e + y * a + z * b, w * e + x * c - y * b + z * a])


def manifold_plus32(x32, d30):
    out = np.array(x32, float)
    for k in range(10):
        s = slice(AOFF[k], AOFF[k + 1])
        out[s] = quat_plus(out[s], d30[3 * k:3 * k + 3]) if AMB[k] == 4 else out[s] + d30[3 * k:3 * k + 3]
    return out


def fd_jacobian(x32, dt, h=1e-6):
    """central differences of e on the manifold"""
    J = np.zeros((15, 30))
    for k in range(30):
        d = np.zeros(30)
        d[k] = h
        diff = np.array([v.a for v in error_dual(manifold_plus32(x32, d), dt)]) - np.array([v.a for v in error_dual(manifold_plus32(x32, -d), dt)])
        diff[3:6] -= 2.0 * np.pi * np.floor((diff[3:6] + np.pi) / (2.0 * np.pi))   # (a wrapped residual may cross +-pi between the two points)
        J[:, k] = diff / (2 * h)
    return J


def body_lib(tmp_dir):
    """tests/plan/unicycle_body_capi.cpp (the shared header unicycle_body.h) built with g++ and loaded"""
    so = os.path.join(str(tmp_dir), "unicycle_body.so")
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                          os.path.join(ROOT, "tests", "plan", "unicycle_body_capi.cpp"), "-o", so], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    lib = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.uni_eval.argtypes = [dp, ctypes.c_double, dp, dp]

    def ev(x32, dt):
        x = np.ascontiguousarray(x32, float)
        e, J = np.zeros(15), np.zeros((15, 30))
        lib.uni_eval(x.ctypes.data_as(dp), dt, e.ctypes.data_as(dp), J.ctypes.data_as(dp))
        return e, J
    return ev


# ---- whole problems --------------------------------------------------------------------------------------------------------------
def factor_x32(pr, values, idx_row):
    return np.concatenate([pr.block(int(b), values) for b in idx_row[:10]])


def unicycle_rows(pr, values, toff, n_tan):
    """(r, J) of every BSGPU_F_UNICYCLE factor of pr in table order: r = A e, J = A de/dtangent placed at the tangent offsets toff[b]
    (-1: constant block, its columns dropped); the per-factor loss is trivial here"""
    rs, Js = [], []
    for idx, consts, lk, _ in pr.factors.get(capi.F_UNICYCLE, []):
        assert np.all(lk == capi.LOSS_TRIVIAL)
        for f in range(idx.shape[0]):
            A = consts[f, 1:].reshape(15, 15)
            e, Jt = error_and_jacobian(factor_x32(pr, values, idx[f]), consts[f, 0])
            J = np.zeros((15, n_tan))
            for k in range(10):
                t = toff[int(idx[f, k])]
                if t >= 0:
                    J[:, t:t + 3] += A @ Jt[:, 3 * k:3 * k + 3]
            rs.append(A @ e)
            Js.append(J)
    return np.concatenate(rs), np.vstack(Js)


def without_unicycle(pr):
    from beam_slam_amd.problem import Problem
    q = Problem.from_arrays(pr.to_arrays())
    q.factors.pop(capi.F_UNICYCLE, None)
    q.meta = pr.meta
    return q


def canonical_toff(pr):
    """tangent offsets in block order over the non-constant blocks (-1: constant), and the tangent size"""
    toff, n = [], 0
    for b in range(pr.n_blocks):
        if pr.is_const[b]:
            toff.append(-1)
            continue
        toff.append(n)
        n += 3 if pr.manifold[b] == capi.MANIFOLD_QUAT_RIGHT else pr.size[b]
    return toff, n


def stacked(pr, rest, oracle, values):
    """r, J (canonical columns) of the whole problem: the oracle's evaluation of every non-unicycle factor of `rest`, then the restated
    unicycle rows"""
    oracle.set_values(values)
    c0, r0, _, J0o = oracle.evaluate(jacobian=True)
    toff, n = canonical_toff(pr)
    J0 = np.zeros((J0o.shape[0], n))
    for b in range(pr.n_blocks):
        ob = oracle.tangent_offset(b)
        if ob >= 0 and toff[b] >= 0:
            w = 3 if pr.manifold[b] == capi.MANIFOLD_QUAT_RIGHT else pr.size[b]
            J0[:, toff[b]:toff[b] + w] = J0o[:, ob:ob + w]
    r1, J1 = unicycle_rows(pr, values, toff, n)
    return np.concatenate([r0, r1]), np.vstack([J0, J1]), toff, c0 + 0.5 * float(r1 @ r1)


def plus_all(pr, values, delta, toff):
    out = values.copy()
    for b in range(pr.n_blocks):
        t = toff[b]
        if t < 0:
            continue
        o, s = pr.offset[b], pr.size[b]
        out[o:o + s] = quat_plus(values[o:o + 4], delta[t:t + 3]) if pr.manifold[b] == capi.MANIFOLD_QUAT_RIGHT else values[o:o + s] + delta[t:t + s]
    return out


def gauss_newton(pr, oracle_cls, max_it=50, tol=1e-13):
    """dense manifold Gauss-Newton to convergence: (values, cost); the oracle evaluates every factor but the unicycle ones"""
    rest = without_unicycle(pr)
    o = oracle_cls()
    rest.load(o)
    x = pr.values.copy()
    for _ in range(max_it):
        r, J, toff, c = stacked(pr, rest, o, x)
        dx = np.linalg.solve(J.T @ J, -J.T @ r)
        t = 1.0
        while t > 1e-6:   # (a step that raises the cost is halved: far from the optimum the full step can overshoot)
            xn = plus_all(pr, x, t * dx, toff)
            if stacked(pr, rest, o, xn)[3] <= c:
                break
            t *= 0.5
        x = xn
        if np.linalg.norm(t * dx) <= tol * (1.0 + np.linalg.norm(x)):
            break
    return x, stacked(pr, rest, o, x)[3]


def reference_system(pr, oracle_cls, values=None):
    """(J, r, toff) of the whole problem at `values` (default: its own), oracle rows then restated unicycle rows"""
    rest = without_unicycle(pr)
    o = oracle_cls()
    rest.load(o)
    r, J, toff, _ = stacked(pr, rest, o, pr.values.copy() if values is None else values)
    return J, r, toff
