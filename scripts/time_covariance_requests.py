"""Times Graph::getCovariance through the C-ABI: the publisher's pose / velocity pairs (bs_publishers/src/odometry_3d_publisher.cpp:66-82,
without an angular-velocity variable: (p,p), (p,q), (q,q), (v,v) of the newest keyframe) as four bsgpu_covariance calls against one
bsgpu_covariance_requests call, on a 20 KF x 500 window and on C2; and the 3x3 covariance of every landmark of the 20 KF x 500 window in
one call.  Wall time of the blocking calls (median of --reps after one warm-up), in milliseconds.
    python scripts/time_covariance_requests.py [--reps 10] [--skip-c2]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from beam_slam_amd import synthetic  # noqa: E402
from beam_slam_amd.gpu import GpuSolver  # noqa: E402


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def window(name, pr, reps, all_landmarks):
    g = GpuSolver(0)
    pr.load(g)
    opt = g.options_default()
    opt.max_num_iterations = 10
    g.solve(opt)
    kf = pr.meta["kf_blocks"]
    q, p, v = int(kf[-1, 0]), int(kf[-1, 1]), int(kf[-1, 2])
    pairs = [(p, p), (p, q), (q, q), (v, v)]
    per_pair = median_ms(lambda: [g.covariance(a, b) for a, b in pairs], reps)
    batched = median_ms(lambda: g.covariance_requests(pairs), reps)
    got = g.covariance_requests(pairs)
    dev = max(np.abs(m - g.covariance(a, b)).max() / np.abs(g.covariance(a, a)).max() for (a, b), m in zip(pairs, got))
    print(f"{name}: publisher pairs (p,p) (p,q) (q,q) (v,v): 4 x bsgpu_covariance {per_pair:.3f} ms, one bsgpu_covariance_requests "
          f"{batched:.3f} ms ({per_pair / batched:.2f}x; largest difference {dev:.1e} of the diagonal scale)", flush=True)
    if all_landmarks:
        lm = [int(b) for b in pr.meta["lm_blocks"]]
        lpairs = [(b, b) for b in lm]
        t = median_ms(lambda: g.covariance_requests(lpairs), max(1, reps // 2))
        passes = -(-len(lm) // 21)
        print(f"{name}: 3x3 covariance of all {len(lm)} landmarks in one bsgpu_covariance_requests: {t:.3f} ms ({passes} factorisation passes)",
              flush=True)
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-c2", action="store_true")
    a = ap.parse_args()
    window("20 KF x 500", synthetic.c1(), a.reps, True)
    if not a.skip_c2:
        window("C2 (200 KF x 50 000)", synthetic.c2(), a.reps, False)


if __name__ == "__main__":
    main()
