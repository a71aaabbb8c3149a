"""Times VisualOdometry::LocalizeFrame's refinement through the C-ABI: bsgpu_localize_frames on one frame of 200 observations and on
64 frames x 200 in one call, against the route the ABI offered before it on the same device — a one-pose context (constant landmark
blocks, BSGPU_F_REPROJ factors) through bsgpu_finalize + bsgpu_solve + bsgpu_covariance_joint({p, q}).  Wall time of the blocking
calls (median of --reps after one warm-up), in milliseconds.  Options: Ceres' defaults; Cauchy loss, a = 1.
    python scripts/time_localize_frames.py [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from beam_slam_amd import capi  # noqa: E402
from beam_slam_amd.gpu import GpuSolver  # noqa: E402
from beam_slam_amd.problem import Problem  # noqa: E402
from frame_cases import CASES, K, R_CB, T_CB, camera, make_frame  # noqa: E402,F401


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--obs", type=int, default=200)
    ap.add_argument("--frames", type=int, default=64)
    a = ap.parse_args()
    g = GpuSolver(0)
    g.set_cameras([camera()])
    opts = g.options_default()
    frames = [make_frame(1000 + i, a.obs, 3.0, 0.2, outlier_frac=0.05) for i in range(a.frames)]

    def call(frs):
        starts = np.concatenate([[0], np.cumsum([len(f["points"]) for f in frs])]).astype(np.int32)
        return g.localize_frames(starts, np.concatenate([f["pixels"] for f in frs]), np.stack([f["q_init"] for f in frs]),
                                 np.stack([f["p_init"] for f in frs]), 0, points=np.concatenate([f["points"] for f in frs]),
                                 loss_kind=capi.LOSS_CAUCHY, loss_a=1.0, options=opts)

    one = call(frames[:1])
    batch = call(frames)
    t_one = median_ms(lambda: call(frames[:1]), a.reps)
    t_batch = median_ms(lambda: call(frames), a.reps)

    # the composed route: a context per frame, described, finalized, solved and asked for its covariance
    fr = frames[0]
    c = GpuSolver(0)

    def composed():
        pr = Problem()
        pr.add_camera(*K, R_CB, T_CB)
        qb = pr.add_quat(fr["q_init"])
        pb = pr.add_block(fr["p_init"])
        lms = pr.add_blocks(fr["points"], const=True)
        n = len(lms)
        idx = np.stack([np.full(n, qb), np.full(n, pb), lms, np.zeros(n, np.int32)], 1)
        pr.add_factors(capi.F_REPROJ, idx, np.concatenate([fr["pixels"], np.ones((n, 1))], 1), capi.LOSS_CAUCHY, 1.0)
        pr.load(c)
        c.finalize()
        s = c.solve(opts)
        cov = c.covariance_joint([pb, qb], [3, 3])
        return s, cov
    s, cov = composed()
    t_comp = median_ms(composed, a.reps)
    print(f"localize_frames 1 x {a.obs} obs:          {t_one:8.3f} ms   ({int(one['iterations'][0])} LM iterations, status {int(one['status'][0])})")
    print(f"localize_frames {a.frames} x {a.obs} obs in one call: {t_batch:8.3f} ms   ({t_batch / a.frames * 1e3:.1f} us per frame, "
          f"iterations {int(batch['iterations'].min())}..{int(batch['iterations'].max())}, {int((batch['status'] == 0).sum())} refined)")
    print(f"composed route 1 x {a.obs} (finalize + solve + covariance_joint): {t_comp:8.3f} ms   ({s.num_iterations} LM iterations)")
    d = np.abs(cov - one["cov"][0]).max() / np.abs(np.diag(cov)).max()
    print(f"  composed vs localize_frames on frame 0: final cost {s.final_cost:.12g} vs {one['final_cost'][0]:.12g}, covariance rel diff {d:.2e}")


if __name__ == "__main__":
    main()
