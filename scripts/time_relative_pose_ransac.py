"""Times the seven-point RANSAC two-view bootstrap through the C-ABI: bsgpu_relative_pose_ransac on one set of 300 matches with 30 %
outliers and on 64 such sets in one call, with the reference's call (100 iterations, no early termination, 5 px) unless told otherwise.  Each
figure is taken twice: HIP events recorded around the blocking call (the device clock over upload, kernel and download), and the
host clock around the same call (it ends in a stream synchronise).  Median and range of --reps calls after a warm-up.  Beside them,
as context only, the wall time of the shared header's serial loop (seven_point.h sp7_ransac_serial, g++ -O2 -march=native, one CPU core) on
the same inputs; that is not a statement about libbeam, which was not available to compare against.  The kernel's own time comes
from a profiler run:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/time_relative_pose_ransac.py --reps 5 --no-cpu
    python scripts/time_relative_pose_ransac.py [--reps 30]"""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seven_point_ref as ref  # noqa: E402
from beam_slam_amd import capi  # noqa: E402
from beam_slam_amd.gpu import GpuSolver  # noqa: E402


class HipEvents:
    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.e0, self.e1 = ctypes.c_void_p(), ctypes.c_void_p()
        assert self.hip.hipEventCreate(ctypes.byref(self.e0)) == 0 and self.hip.hipEventCreate(ctypes.byref(self.e1)) == 0

    def time_ms(self, fn):
        ms = ctypes.c_float(0.0)
        assert self.hip.hipEventRecord(self.e0, None) == 0
        fn()
        assert self.hip.hipEventRecord(self.e1, None) == 0 and self.hip.hipEventSynchronize(self.e1) == 0
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.e0, self.e1) == 0
        return float(ms.value)


def stats(ts):
    return f"median {np.median(ts):8.3f} ms  (min {np.min(ts):.3f}, max {np.max(ts):.3f}, n = {len(ts)})"


def cpu_serial(frames, a, seed):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "time_seven_point_cpu")
        subprocess.check_call(["g++", "-O2", "-march=native", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                               os.path.join(ROOT, "scripts", "time_seven_point_cpu.cpp"), "-o", exe])
        out = {}
        for name, group in (("1", frames[:1]), (str(len(frames)), frames)):
            lines = [f"{len(group)} {a.prob!r} {a.threshold!r} {a.max_iters} {seed} {a.cpu_reps}"]
            for s in group:
                lines.append(f"{len(s['px_first'])} " + " ".join(repr(float(v)) for v in s["K"]))
                lines += [" ".join(repr(float(v)) for v in (*p, *q)) for p, q in zip(s["px_first"], s["px_last"])]
            path = os.path.join(tmp, "frames.txt")
            with open(path, "w") as f:
                f.write("\n".join(lines) + "\n")
            txt = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.splitlines()
            out[name] = ([float(t.split()[1]) for t in txt if t.startswith("MS")], [int(v) for v in txt[-1].split()[1:]])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--prob", type=float, default=0.0)
    ap.add_argument("--threshold", type=float, default=5.0)
    ap.add_argument("--max-iters", type=int, default=100)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    seed = 11
    frames = [ref.make_pair(3000 + k, a.matches, int(round(a.outliers * a.matches))) for k in range(a.sets)]
    g = GpuSolver(0)
    cam = capi.Camera()
    cam.fx, cam.fy, cam.cx, cam.cy = ref.K_DEFAULT
    cam.R_cam_baselink[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    cam.t_cam_baselink[:] = [0.0, 0.0, 0.0]
    g.set_cameras([cam])
    ev = HipEvents()

    def call(group):
        ms = np.concatenate([[0], np.cumsum([len(s["px_first"]) for s in group])]).astype(np.int32)
        return g.relative_pose_ransac(ms, np.concatenate([s["px_first"] for s in group]), np.concatenate([s["px_last"] for s in group]), 0,
                                      prob=a.prob, threshold_px=a.threshold, max_iters=a.max_iters, seed=seed)

    for name, group in ((f"1 x {a.matches}", frames[:1]), (f"{a.sets} x {a.matches} in one call", frames)):
        out = call(group)
        call(group)
        evs, walls = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            evs.append(ev.time_ms(lambda: call(group)))
            walls.append(1e3 * (time.perf_counter() - t0))
        ok = sum(bool(np.array_equal(m, s["labels"])) for m, s in zip(np.split(out["mask"], len(group)), group))
        print(f"relative_pose_ransac {name}: samples consumed {int(out['n_iters'].min())}..{int(out['n_iters'].max())}, "
              f"{ok} of {len(group)} masks equal the labels")
        print(f"    HIP events around the call: {stats(evs)}")
        print(f"    host clock around the call: {stats(walls)}   ({np.median(walls) / len(group) * 1e3:.1f} us per set)")
    if not a.no_cpu:
        cpu = cpu_serial(frames, a, seed)
        for name, (ts, iters) in cpu.items():
            print(f"seven_point.h serial loop on one CPU core, {name} x {a.matches}: {stats(ts)}   (samples consumed {min(iters)}..{max(iters)})")
        print("    (context only: not libbeam, which was not available to compare against)")


if __name__ == "__main__":
    main()
