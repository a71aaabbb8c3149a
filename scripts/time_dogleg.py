#!/usr/bin/env python
"""LEVENBERG_MARQUARDT against DOGLEG (trust_region_strategy_type) on three windows: a lone 20 KF x 500, the window of
scripts/rejected_steps.py (50 KF x 5 000 from a perturbed start, where steps are rejected) and C2.  Median of 20 solves each (after 3 warm-up
solves): trust-region steps per second (the bench's "LM it/s" unit, for either strategy), ms per solve, linear systems factorised per solve
(bsgpu_num_factorizations), steps that reused their Gauss-Newton step per solve.  Then the time of one reused step: DOGLEG solves of the
rejected-steps window from initial radii and iteration budgets that lead to different numbers of new and reused steps, and a least-squares
fit of
    ms per solve = t0 + t_new * (new Gauss-Newton steps) + t_reuse * (reused steps).
    python scripts/time_dogleg.py"""
import sys
import time

sys.path.insert(0, ".")
import numpy as np

from beam_slam_amd import capi, synthetic
from beam_slam_amd.gpu import GpuSolver


def windows():
    yield "20 KF x 500", synthetic.vio_window(n_kf=20, n_lm=500, seed=20250620), None
    pr = synthetic.vio_window(n_kf=50, n_lm=5000, seed=20250620)
    yield "rejected_steps 50 KF x 5000", pr, pr.values + 0.05 * np.random.default_rng(3).standard_normal(pr.values.size)
    yield "C2 200 KF x 50000", synthetic.c2(), None


def main():
    for name, pr, x0 in windows():
        g = GpuSolver(0)
        pr.load(g)
        g.finalize()
        start = pr.values if x0 is None else x0
        for strategy, label in ((capi.TR_LEVENBERG_MARQUARDT, "LM"), (capi.TR_DOGLEG, "DOGLEG")):
            opt = g.options_vio()
            opt.max_solver_time_in_seconds = 0.0
            opt.max_num_iterations = 20
            opt.trust_region_strategy_type = strategy
            ms, steps, facts, reused, cost = [], [], [], [], 0.0
            for k in range(23):
                g.set_values(start)
                t0 = time.perf_counter()
                s = g.solve(opt)
                dt = time.perf_counter() - t0
                if k < 3:
                    continue
                its = g.iterations()
                rejected = sum(1 for it in its[1:] if it.step_is_valid and not it.step_is_successful)
                ms.append(1e3 * dt)
                steps.append(s.num_linear_solves)
                facts.append(g.num_factorizations())
                reused.append(rejected if strategy == capi.TR_DOGLEG else 0)
                cost = s.final_cost
            m = float(np.median(ms))
            print("%-28s %-6s %8.0f steps/s  %8.3f ms/solve  %5.1f factorisations/solve  %5.1f steps  %4.1f reused  final cost %.9g"
                  % (name, label, np.median(steps) / (m * 1e-3), m, np.median(facts), np.median(steps), np.median(reused), cost), flush=True)
        g.close()
    # the time of a reused step against a new one, on the rejected-steps window
    pr = synthetic.vio_window(n_kf=50, n_lm=5000, seed=20250620)
    x0 = pr.values + 0.05 * np.random.default_rng(3).standard_normal(pr.values.size)
    g = GpuSolver(0)
    pr.load(g)
    g.finalize()
    rows, t = [], []
    for radius, iters in ((1e2, 20), (1e4, 20), (1e6, 20), (1e8, 20), (1e10, 20), (1e2, 10), (1e6, 10), (1e10, 10)):
        opt = g.options_vio()
        opt.max_solver_time_in_seconds = 0.0
        opt.max_num_iterations = iters
        opt.trust_region_strategy_type = capi.TR_DOGLEG
        opt.initial_trust_region_radius = radius
        ms = []
        for k in range(18):
            g.set_values(x0)
            t0 = time.perf_counter()
            s = g.solve(opt)
            if k >= 3:
                ms.append(1e3 * (time.perf_counter() - t0))
        n_new = g.num_factorizations()
        n_reuse = s.num_linear_solves - n_new
        rows.append([1.0, n_new, n_reuse])
        t.append(float(np.median(ms)))
        print("  radius %-8.0e %2d iterations: %2d new + %2d reused steps  %7.3f ms/solve" % (radius, iters, n_new, n_reuse, t[-1]), flush=True)
    A = np.array(rows)
    if np.linalg.matrix_rank(A) == 3:
        c = np.linalg.lstsq(A, np.array(t), rcond=None)[0]
        print("fit: %.3f ms + %.1f us per new Gauss-Newton step + %.1f us per reused step" % (c[0], 1e3 * c[1], 1e3 * c[2]))
    else:
        print("fit: the radii did not vary the numbers of new and reused steps independently")
    g.close()


if __name__ == "__main__":
    main()
