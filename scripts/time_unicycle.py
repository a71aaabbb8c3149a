"""Times BSGPU_F_UNICYCLE windows on one device: LM iterations per second of a 200-state unicycle chain, and of the reference-sized
standalone-VO window (20 key frames x 500 landmarks) with unicycle factors against the same window with IMU factors.  Each solve runs a
fixed number of LM iterations (tolerances 0) from the same start, after one warm-up solve; median of --reps.  With --kernel-stats CSV
(the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/time_unicycle.py`) it also prints the unicycle kernels' mean time per launch.
    python scripts/time_unicycle.py [--reps 10] [--iters 20] [--kernel-stats PATH]"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beam_slam_amd import synthetic  # noqa: E402
from beam_slam_amd.gpu import GpuSolver  # noqa: E402


def lm_rate(pr, iters, reps):
    g = GpuSolver(0)
    pr.load(g)
    o = g.options_default()
    o.max_num_iterations = iters
    o.function_tolerance = o.gradient_tolerance = o.parameter_tolerance = 0.0
    x0 = pr.values.copy()
    rates = []
    for rep in range(reps + 1):
        g.set_values(x0)
        t0 = time.perf_counter()
        s = g.solve(o)
        dt = time.perf_counter() - t0
        if rep:
            rates.append(s.num_iterations / dt)
    return float(np.median(rates)), int(s.num_iterations)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    chain = lm_rate(synthetic.unicycle_window(n_states=200), a.iters, a.reps)
    print(f"unicycle chain, 200 states: {chain[0]:.0f} LM it/s ({chain[1]} iterations per solve)")
    vo_uni = lm_rate(synthetic.unicycle_window(n_states=20, n_lm=500, seed=20250620), a.iters, a.reps)
    vo_imu = lm_rate(synthetic.vio_window(n_kf=20, n_lm=500), a.iters, a.reps)
    print(f"VO 20 KF x 500 landmarks: unicycle factors {vo_uni[0]:.0f} LM it/s, IMU factors {vo_imu[0]:.0f} LM it/s "
          f"(ratio {vo_uni[0] / vo_imu[0]:.3f})")
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "unicycle" in row.get("Name", ""):
                    print(f"{row['Name'][:90]}: {row['Calls']} launches, {float(row['AverageNs']) / 1e3:.2f} us per launch")


if __name__ == "__main__":
    main()
