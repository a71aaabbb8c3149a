"""50-digit reference of bsgpu_inertial_alignment (mpmath) and its stored results, tests/golden/align_hp.npz — TEST INFRASTRUCTURE.

The steps are those of tests/align_ref.py (`align`, written over an arithmetic back-end) evaluated on the float64 inputs with the
back-end below: closed-form sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3 with the exact limit at th == 0, the pseudo-inverse
through mpmath.eigsy, and the least squares through the normal equations and a Cholesky factorisation that skips structural zeros.  At
50 digits the normal equations cost 2 log10 cond(A), about 10 digits, of 50; the Cholesky factor of A^T A with the columns ordered
v_0 .. v_{N-1}, g, s is the triangular factor of A's QR up to signs, so its diagonal is the one the rank decision reads, and a zero
column gives an exactly zero pivot.

mpmath is needed only where the reference is evaluated (`python tests/align_hp.py` writes the file, one test regenerates it); tests
read the stored inputs and values.  Every value is stored as a float64 pair (hi the rounded value, lo the rest).
"""
import os

import numpy as np

import align_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_hp.npz")
INPUT_KEYS = ("tf", "qf", "pf", "t", "w", "a", "bg_true", "s_true", "g_true")
#: unit cases of FromTwoVectors (a, b): generic, nearly parallel, antiparallel along coordinate axes (both choices of the smallest
#: component the contract's rule can make there), antiparallel but for 3e-9 rad (1 + cos = 4.7e-18 against 2^-52), and parallel
FTV = np.array([[[0.3, -1.2, 9.7], [0.0, 0.0, -9.80665]], [[1e-9, -2e-9, -9.80665], [0.0, 0.0, -9.80665]],
                [[0.0, 0.0, 9.80665], [0.0, 0.0, -9.80665]], [[5.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], [[0.0, 7.0, 0.0], [0.0, -2.0, 0.0]],
                [[3e-8, 0.0, 9.80665], [0.0, 0.0, -9.80665]], [[0.0, 0.0, -9.80665], [0.0, 0.0, -9.80665]]])


def backend():
    import mpmath as mp
    mp.mp.dps = 50

    class Mp:
        zero, one = mp.mpf(0), mp.mpf(1)
        sqrt, sin, cos, atan2 = mp.sqrt, mp.sin, mp.cos, mp.atan2

        @staticmethod
        def num(x):
            return mp.mpf(float(x))

        @staticmethod
        def coeffs(th):
            if th == 0:
                return mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1) / 6
            return mp.sin(th) / th, (1 - mp.cos(th)) / th ** 2, (th - mp.sin(th)) / th ** 3

        @staticmethod
        def pinv_solve(A, b):
            E, Q = mp.eigsy(mp.matrix(A))
            lmax = max(E)
            x, rank = [mp.mpf(0)] * 3, 0
            for k in range(3):
                if E[k] > 3 * mp.mpf(2) ** -52 * lmax:
                    rank += 1
                    f = sum(Q[i, k] * b[i] for i in range(3)) / E[k]
                    x = [x[i] + f * Q[i, k] for i in range(3)]
            return x, rank

        @staticmethod
        def lstsq(A, b):
            n = len(A[0])
            H = [dict() for _ in range(n)]                      # A^T A, rows as {column: value}
            g = [mp.mpf(0)] * n
            for row, bi in zip(A, b):
                nz = [(j, v) for j, v in enumerate(row) if v != 0]
                for i, vi in nz:
                    g[i] += vi * bi
                    for j, vj in nz:
                        H[i][j] = H[i].get(j, 0) + vi * vj
            L = [dict() for _ in range(n)]                      # lower factor, rows as {column: value}
            diag = []
            for j in range(n):
                d = H[j].get(j, mp.mpf(0)) - sum(v * v for v in L[j].values())
                d = mp.sqrt(d) if d > 0 else mp.mpf(0)
                diag.append(d)
                if d == 0:
                    continue
                L[j][j] = d
                for i in range(j + 1, n):
                    s = H[i].get(j, 0) - sum(L[i].get(k, 0) * v for k, v in L[j].items() if k != j)
                    if s != 0:
                        L[i][j] = s / d
            if min(diag) == 0:
                return [mp.mpf(0)] * n, diag
            y = [mp.mpf(0)] * n
            for i in range(n):
                y[i] = (g[i] - sum(v * y[k] for k, v in L[i].items() if k != i)) / L[i][i]
            x = [mp.mpf(0)] * n
            for i in reversed(range(n)):
                x[i] = (y[i] - sum(L[k][i] * x[k] for k in range(i + 1, n) if i in L[k])) / L[i][i]
            return x, diag
    return Mp


def _pair(values):
    import mpmath as mp
    hi = np.array([float(v) for v in values])
    lo = np.array([float(mp.mpf(v) - mp.mpf(float(v))) for v in values])
    return hi, lo


def evaluate(paths):
    """The arrays of tests/golden/align_hp.npz from the path dicts: inputs, and per case the 50-digit outputs and decisions."""
    B = backend()
    out = {}
    for pk, p in paths.items():
        for k in INPUT_KEYS:
            out[f"in__{pk}__{k}"] = np.asarray(p[k], float)
    for name, (pk, kw) in ref.CASES.items():
        r = ref.run(paths[pk], kw, B=B)
        for grp in ref.GROUPS:
            v = r[grp]
            v = [v] if not isinstance(v, list) else [e for row in v for e in (row if isinstance(row, list) else [row])]
            out[f"hp__{name}__{grp}__hi"], out[f"hp__{name}__{grp}__lo"] = _pair(v)
        out[f"hp__{name}__status"] = np.array([r["status"], r["gyro_rank"]], np.int32)
        out[f"hp__{name}__qr_ratio"] = np.array([-1.0 if r["qr_ratio"] is None else float(r["qr_ratio"])])
    q = [ref.from_two_vectors(B, [B.num(e) for e in a], [B.num(e) for e in b]) for a, b in FTV]
    out["ftv__in"] = FTV
    out["ftv__hi"], out["ftv__lo"] = _pair([e for row in q for e in row])
    return out


def load():
    """-> (paths: name -> dict of inputs, hp: case -> dict(group -> (hi, lo), status, gyro_rank, qr_ratio), ftv: (inputs, hi, lo))."""
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    paths, hp = {}, {}
    for k, v in d.items():
        tok = k.split("__")
        if tok[0] == "in":
            paths.setdefault(tok[1], {})[tok[2]] = v
        elif tok[0] == "hp" and len(tok) == 4:
            e = hp.setdefault(tok[1], {})
            e.setdefault(tok[2], [None, None])[0 if tok[3] == "hi" else 1] = v
        elif tok[0] == "hp" and tok[2] == "status":
            hp.setdefault(tok[1], {}).update(status=int(v[0]), gyro_rank=int(v[1]))
        elif tok[0] == "hp":
            hp.setdefault(tok[1], {})["qr_ratio"] = float(v[0])
    return paths, hp, (d["ftv__in"], d["ftv__hi"].reshape(-1, 4), d["ftv__lo"].reshape(-1, 4))


def error(got, hi_lo):
    """max |got - (hi + lo)|: (got - hi) is exact wherever it matters, so the reference's rounding to float64 does not enter."""
    hi, lo = hi_lo
    got = np.asarray(got, float).reshape(-1)
    return float(np.abs((got - hi) - lo).max()) if got.size else 0.0


def check(got, yard, hp_case, who, name):
    """The accuracy criterion, per quantity: |got - 50 digits| <= max(8 x |NumPy restatement - 50 digits|, 1e-15 x the quantity's
    largest magnitude).  got / yard: {group: flat array, status, gyro_rank}.  Returns {group: error / bound}."""
    assert got["status"] == hp_case["status"] == yard["status"], (who, name, got["status"], hp_case["status"], yard["status"])
    assert got["gyro_rank"] == hp_case["gyro_rank"] == yard["gyro_rank"], (who, name)
    ratios = {}
    for g in ref.GROUPS:
        e, e_y = error(got[g], hp_case[g]), error(yard[g], hp_case[g])
        bound = max(8.0 * e_y, 1e-15 * float(np.abs(hp_case[g][0]).max()))
        print(f"{who}: {name:<16s} {g:<10s} restatement {e_y:.3e} error {e:.3e} bound {bound:.3e}")
        assert e <= bound, (who, name, g, e, bound)
        ratios[g] = e / bound if bound > 0 else 0.0
    return ratios


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **evaluate(ref.paths()))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
