"""Times the visual-inertial alignment through the C-ABI: bsgpu_inertial_alignment on one path of 30 frames at 10 Hz with 200 Hz IMU
samples, and on 64 such candidate paths (one IMU stream, positions rescaled per candidate) in one call, with the reference's
parameters.  Each figure is taken twice: HIP events recorded around the blocking call (the device clock over upload, kernel and
download), and the host clock around the same call.  Median and range of --reps calls after a warm-up.  Beside them the wall time of
the shared header's serial loop (inertial_align.h on one lane, g++ -O2 -march=native, one CPU core) on the same inputs.  The kernel's
own time comes from a profiler run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_inertial_alignment.py --reps 5 --no-cpu
    python scripts/time_inertial_alignment.py [--reps 30]"""
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
import align_ref as ref  # noqa: E402
from beam_slam_amd import gpu  # noqa: E402


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


def cpu_serial(groups, a):
    f = lambda v: " ".join(repr(float(x)) for x in np.ravel(v))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "time_align_cpu")
        subprocess.check_call(["g++", "-O2", "-march=native", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                               os.path.join(ROOT, "scripts", "time_align_cpu.cpp"), "-o", exe])
        out = {}
        for name, (fs, tf, qf, pf, rng, t, w, acc) in groups:
            lines = [f"{len(fs) - 1} {len(tf)} {len(t)} {int(a.bridge_gap)} 1 {a.cpu_reps}", " ".join(str(int(v)) for v in fs),
                     " ".join(str(int(v)) for v in rng.ravel())]
            lines += [f([tf[i], *qf[i], *pf[i]]) for i in range(len(tf))] + [f([t[i], *w[i], *acc[i]]) for i in range(len(t))]
            path = os.path.join(tmp, "paths.txt")
            with open(path, "w") as fh:
                fh.write("\n".join(lines) + "\n")
            txt = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.splitlines()
            out[name] = ([float(ln.split()[1]) for ln in txt if ln.startswith("MS")], [int(v) for v in txt[-1].split()[1:]])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cpu-reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--paths", type=int, default=64)
    ap.add_argument("--bridge-gap", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    base = ref.make_path(0.1002 + 0.1 * np.arange(a.frames))
    cands = [dict(base, pf=base["pf"] * (1.0 + 0.01 * k)) for k in range(a.paths)]
    groups = [(f"1 x {a.frames} frames", ref.batch(cands[:1])),
              (f"{a.paths} x {a.frames} frames in one call", ref.batch(cands, {k: 0 for k in range(1, a.paths)}))]
    ev = HipEvents()
    for name, arrays in groups:
        call = lambda: gpu.inertial_alignment(*arrays, bridge_gap=a.bridge_gap, apply_scale=True)
        out = call()
        call()
        evs, walls = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            evs.append(ev.time_ms(call))
            walls.append(1e3 * (time.perf_counter() - t0))
        print(f"inertial_alignment {name}: {int((out['status'] == 0).sum())} of {len(out['status'])} paths aligned, scale "
              f"{out['scale'].min():.4f}..{out['scale'].max():.4f}, {len(arrays[5])} IMU samples")
        print(f"    HIP events around the call: {stats(evs)}")
        print(f"    host clock around the call: {stats(walls)}   ({np.median(walls) / len(out['status']) * 1e3:.1f} us per path)")
    if not a.no_cpu:
        for name, (ts, status) in cpu_serial(groups, a).items():
            print(f"inertial_align.h serial loop on one CPU core, {name}: {stats(ts)}   ({status.count(0)} of {len(status)} paths aligned)")


if __name__ == "__main__":
    main()
