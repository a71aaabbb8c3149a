"""Numpy restatement of Ceres' trust-region minimiser with the DOGLEG strategy (TRADITIONAL_DOGLEG) and Jacobi scaling, for the tests.

Written from the Ceres 1.14 TrustRegionMinimizer / DoglegStrategy semantics as beam_slam_amd/csrc/dogleg.h states them ([EXT], recalled), in
Ceres' own scaled form: J~ = J S, D = sqrt(clamp(diag(J~^T J~))), g' = J~^T r / D, the Gauss-Newton step from (J~^T J~ + mu D^2) y = J~^T r by
a dense Cholesky.  Residuals and Jacobians come from a solver's evaluate(jacobian=True) (the CPU oracle), x (+) delta from
tests/helpers.manifold_plus.  The acceptance tests and tolerances are those of beam_slam_amd/csrc/lm_state.h.

The core, `DoglegModel` / `traditional_step`, works on a given J and r so that the CPU tests can drive it on linear problems."""
import math

import numpy as np

from helpers import manifold_plus

MIN_MU, MAX_MU, MU_INCREASE = 1e-8, 1.0, 10.0


class DoglegModel:
    """The strategy's state at one linearisation: Cauchy point and Gauss-Newton step, kept for reuse after a rejection."""

    def __init__(self, J, r, scale, lo, hi, mu):
        Jt = J * scale[None, :]
        self.diag = np.sqrt(np.clip(np.sum(Jt * Jt, axis=0), lo, hi))
        self.scale = scale
        self.gradient = (Jt.T @ r) / self.diag
        Jg = Jt @ (self.gradient / self.diag)
        self.alpha = float(self.gradient @ self.gradient) / float(Jg @ Jg)
        self.mu = mu
        self.factorizations = 0
        self.gn = None
        A0 = Jt.T @ Jt
        b = Jt.T @ r
        while self.mu < MAX_MU:
            self.factorizations += 1
            try:
                L = np.linalg.cholesky(A0 + self.mu * np.diag(self.diag * self.diag))
                y = np.linalg.solve(L.T, np.linalg.solve(L, b))
            except np.linalg.LinAlgError:
                y = None
            if y is None or not np.all(np.isfinite(y)):
                self.mu *= MU_INCREASE
                continue
            self.gn = -self.diag * y
            break

    @property
    def valid(self):
        return self.gn is not None

    def step(self, radius):
        """(delta in unscaled tangent coordinates, |step'|, case)"""
        s, norm, case = traditional_step(self.gradient, self.gn, self.alpha, radius)
        return self.scale * s / self.diag, norm, case


def traditional_step(g, gn, alpha, radius):
    """ComputeTraditionalDoglegStep in the scaled space: (step', |step'|, case)"""
    gradient_norm = math.sqrt(float(g @ g))
    gauss_newton_norm = math.sqrt(float(gn @ gn))
    if gauss_newton_norm <= radius:
        return gn.copy(), gauss_newton_norm, 1
    if gradient_norm * alpha >= radius:
        return -(radius / gradient_norm) * g, radius, 2
    b_dot_a = -alpha * float(g @ gn)
    a_squared_norm = (alpha * gradient_norm) ** 2
    b_minus_a_squared_norm = a_squared_norm - 2 * b_dot_a + gauss_newton_norm ** 2
    c = b_dot_a - a_squared_norm
    d = math.sqrt(c * c + b_minus_a_squared_norm * (radius ** 2 - a_squared_norm))
    beta = (d - c) / b_minus_a_squared_norm if c <= 0 else (radius * radius - a_squared_norm) / (d + c)
    s = (-alpha * (1.0 - beta)) * g + beta * gn
    return s, math.sqrt(float(s @ s)), 3


def step_accepted(rho, step_norm, radius, mu):
    if rho < 0.25:
        radius *= 0.5
    if rho > 0.75:
        radius = max(radius, 3.0 * step_norm)
    return radius, max(MIN_MU, 2.0 * mu / MU_INCREASE)


def solve(pr, solver, options, fixed_cost=0.0):
    """Runs the minimiser on problem `pr` loaded into `solver` (an oracle).  Returns dict(records, x, factorizations, reused, steps).
    records: per iteration (iteration, valid, successful, cost, radius, mcc, relative_decrease) as bsgpu_iteration holds them."""
    o = options
    pr.load(solver)
    solver.finalize()
    nb = pr.n_blocks
    toff = [solver.tangent_offset(b) for b in range(nb)]
    toff_of = toff.__getitem__
    free = np.zeros(len(pr.values), bool)
    for b in range(nb):
        if toff[b] >= 0:
            free[pr.offset[b]:pr.offset[b] + pr.size[b]] = True

    def evaluate(x, jacobian=True):
        solver.set_values(x)
        c, r, _, J = solver.evaluate(jacobian=jacobian)
        return c, r, J

    x = np.array(pr.values, np.float64)
    cost, r, J = evaluate(x)
    scale = 1.0 / (1.0 + np.linalg.norm(J, axis=0)) if o.jacobi_scaling else np.ones(J.shape[1])

    def gmax_of(x, r, J):
        g = J.T @ r
        return float(np.abs(x - manifold_plus(pr, x, -g, toff_of)).max()) if g.size else 0.0

    x_cost = cost - fixed_cost
    radius, mu = o.initial_trust_region_radius, MIN_MU
    rec = dict(iteration=0, valid=1, successful=1, cost=cost, mcc=0.0, relative_decrease=0.0, gmax=gmax_of(x, r, J))
    records = []
    model = None
    factorizations = reused = steps = invalid = 0
    n_invalid = 0
    while True:
        rec["radius"] = radius
        records.append(dict(rec))
        if rec["iteration"] >= o.max_num_iterations:
            break
        if rec["successful"] and rec["gmax"] <= o.gradient_tolerance:
            break
        if radius <= o.min_trust_region_radius:
            break
        prev = rec
        rec = dict(iteration=prev["iteration"] + 1, valid=0, successful=0, cost=0.0, mcc=0.0, relative_decrease=0.0, gmax=prev["gmax"])
        steps += 1
        if model is None:
            model = DoglegModel(J, r, scale, o.min_lm_diagonal, o.max_lm_diagonal, mu)
            mu = model.mu
            factorizations += model.factorizations
        else:
            reused += 1
        if model.valid:
            delta, step_norm, _ = model.step(radius)
            Jd = J @ delta
            mcc = -float(Jd @ (r + 0.5 * Jd))
        else:
            mcc = 0.0
        rec["mcc"] = mcc
        if not (model.valid and mcc > 0.0):
            invalid += 1
            n_invalid += 1
            if n_invalid >= o.max_num_consecutive_invalid_steps:
                break
            mu *= MU_INCREASE
            model = None
            rec["cost"] = x_cost + fixed_cost
            continue
        rec["valid"] = 1
        n_invalid = 0
        x_new = manifold_plus(pr, x, delta, toff_of)
        cand, _, _ = evaluate(x_new, jacobian=False)
        cand -= fixed_cost
        step2 = float(np.sum((x - x_new)[free] ** 2))
        x_norm = math.sqrt(float(np.sum(x[free] ** 2)))
        if math.sqrt(step2) <= o.parameter_tolerance * (x_norm + o.parameter_tolerance):
            break
        cost_change = x_cost - cand
        if abs(cost_change) <= o.function_tolerance * x_cost:
            break
        rho = cost_change / mcc
        rec["relative_decrease"] = rho
        if rho > o.min_relative_decrease:
            radius, mu = step_accepted(rho, step_norm, radius, mu)
            x, x_cost = x_new, cand
            _, r, J = evaluate(x)
            rec["successful"] = 1
            rec["cost"] = x_cost + fixed_cost
            rec["gmax"] = gmax_of(x, r, J)
            model = None
        else:
            radius *= 0.5
            rec["cost"] = cand + fixed_cost
    return dict(records=records, x=x, factorizations=factorizations, reused=reused, steps=steps, invalid=invalid)
