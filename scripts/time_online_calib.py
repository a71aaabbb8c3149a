#!/usr/bin/env python
"""What estimating the camera extrinsics costs: a 10-iteration LM solve of the 20 KF x 500 window and of C2's 200 KF x 50 000 window,
three ways, alternating in one process —
    type-0   every reprojection factor a BSGPU_F_REPROJ on the equivalent camera (today's path),
    const    every factor a BSGPU_F_REPROJ_ONLINE_CALIB, the extrinsic pair constant (today's path: the camera is folded at finalize()),
    free     the same factors, the pair estimated (csrc/k_calib.hip: pair entries, C rows, full pose part, host-decided steps).
Prints microseconds per LM iteration from the solve's device events (bsgpu_summary.device_time_in_seconds / iterations taken): median,
minimum and maximum over the repetitions — the spread of repeated identical solves is what the two constant figures are to agree within.
    python scripts/time_online_calib.py [--reps 15] [--small-only]
The new kernels' own times: rocprofv3 --kernel-trace --stats -- python scripts/time_online_calib.py --reps 3 --only free"""
import argparse
import sys

sys.path.insert(0, ".")
import numpy as np

from beam_slam_amd import synthetic
from beam_slam_amd.gpu import GpuSolver


def variants(n_kf, n_lm, seed):
    free = synthetic.vio_window(n_kf=n_kf, n_lm=n_lm, seed=seed, online_calib=True, free_extrinsics=True)
    const = synthetic.vio_window(n_kf=n_kf, n_lm=n_lm, seed=seed, online_calib=True, free_extrinsics=False)
    qe, pe = const.meta["ext_blocks"]
    plain = synthetic.vio_window(n_kf=n_kf, n_lm=n_lm, seed=seed)
    R_cb = synthetic.quat_to_rot(const.block(qe)).T
    plain.cameras[0].R_cam_baselink[:] = list(R_cb.ravel())
    plain.cameras[0].t_cam_baselink[:] = list(-R_cb @ const.block(pe))
    return {"type-0": plain, "const": const, "free": free}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--only", default=None, help="one of type-0, const, free")
    a = ap.parse_args()
    sizes = [("20 KF x 500", 20, 500, 7)] + ([] if a.small_only else [("C2 200 KF x 50000", 200, 50000, 20250620)])
    for name, n_kf, n_lm, seed in sizes:
        prs = variants(n_kf, n_lm, seed)
        if a.only:
            prs = {a.only: prs[a.only]}
        solvers, us = {}, {k: [] for k in prs}
        for k, pr in prs.items():
            g = GpuSolver(0)
            pr.load(g)
            g.finalize()
            solvers[k] = g
        opt = next(iter(solvers.values())).options_vio()
        opt.max_solver_time_in_seconds = 0.0
        opt.max_num_iterations = 10
        info = {}
        for rep in range(a.reps + 3):
            for k, g in solvers.items():   # alternating: drift of the device's clocks hits the three alike
                g.reset_values()
                s = g.solve(opt)
                if rep >= 3:
                    us[k].append(1e6 * s.device_time_in_seconds / max(1, s.num_iterations))
                info[k] = (s.num_iterations, s.final_cost)
        for k in prs:
            v = np.array(us[k])
            print("%-18s %-7s %9.1f us / LM iteration  (min %9.1f  max %9.1f, %d solves)  %2d iterations  final cost %.9g"
                  % (name, k, np.median(v), v.min(), v.max(), v.size, info[k][0], info[k][1]), flush=True)
        if "free" in us and "const" in us:
            print("%-18s free / const = %.2f" % (name, np.median(us["free"]) / np.median(us["const"])), flush=True)
        for g in solvers.values():
            g.close()


if __name__ == "__main__":
    main()
