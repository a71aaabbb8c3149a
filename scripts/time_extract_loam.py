"""Times the LOAM feature extraction through the C-ABI at the shipped parameters (config/matchers/loam_vlp16.json,
capi.LOAM_FEATURE_DEFAULTS): bsgpu_extract_loam_features on 1, 10 and 20 VLP-16 revolutions per call, the ring taken from the
elevation.  The scans are the revolutions of time_register_loam.py (16 rings x 1 812 azimuths cast from inside the 20 x 14 x 5 m room of
the tests along a path, 1 cm range noise).
Each figure is taken twice: HIP events recorded around the blocking call (the device clock over upload, kernels and download), and the
host clock around the same call, which also holds the packing of the picks into the caller's arrays.  Median and range of --reps calls
after a warm-up.  Beside them the wall time of the shared header's serial loop (loam_features.h on one core, g++ -O2 -march=native) on
the same scans: the only baseline there is, since libbeam's extractor is not in the reference checkout.  The kernels' own time comes
from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_extract_loam.py --reps 3 --no-cpu
    python scripts/time_extract_loam.py [--reps 20]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from test_loam_features import feat_command  # noqa: E402
from time_register_scans import HipEvents, revolution, stats  # noqa: E402
from time_register_gicp import pose  # noqa: E402
from beam_slam_amd import capi, gpu  # noqa: E402


def cpu_serial(groups, a):
    params = {k: v for k, v in capi.LOAM_FEATURE_DEFAULTS.items() if k != "downsample_less_flat_features"}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "time_loam_features_cpu")
        subprocess.check_call(["g++", "-O2", "-march=native", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                               os.path.join(ROOT, "scripts", "time_loam_features_cpu.cpp"), "-o", exe])
        out = {}
        for name, scans in groups:
            path = os.path.join(tmp, "scans.bin")
            np.concatenate([feat_command(s, None, **params) for s in scans]).tofile(path)
            txt = subprocess.run([exe, str(a.cpu_reps), path], capture_output=True, text=True, check=True).stdout.splitlines()
            out[name] = ([float(ln.split()[1]) for ln in txt if ln.startswith("MS")], txt[-1])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    scans = [revolution(pose([0.0, 0.0, 0.01 * k], [-2.0 + 0.12 * k, 0.02 * k, 0.0]), rng) for k in range(20)]
    groups = [(f"{n} revolution{'s' if n > 1 else ''} per call", scans[:n]) for n in (1, 10, 20)]
    ev = HipEvents()
    for name, ss in groups:
        start, pts = np.cumsum([0] + [len(s) for s in ss]), np.concatenate(ss)
        call = lambda: gpu.extract_loam_features(start, pts)
        out = call()
        per = [tuple(int(out[k + "_start"][s + 1] - out[k + "_start"][s]) for k in ("edge", "weak_edge", "surf", "weak_surf")) for s in range(len(ss))]
        print(f"extract_loam_features {name} ({len(ss[0])} points each): SHARP / LESS_SHARP / FLAT / LESS_FLAT of the first {per[0]}, "
              f"of the call {tuple(int(sum(p[k] for p in per)) for k in range(4))}")
        evs, walls = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            evs.append(ev.time_ms(call))
            walls.append(1e3 * (time.perf_counter() - t0))
        print(f"    HIP events around the call: {stats(evs)}")
        print(f"    host clock around the call: {stats(walls)}   ({np.median(walls) / len(ss):.3f} ms per scan)")
        bare = lambda: gpu.extract_loam_features(start, pts, weak=False, labels=False, curvature=False, with_points=False)
        walls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            bare()
            walls.append(1e3 * (time.perf_counter() - t0))
        print(f"    host clock, strong indices only:  {stats(walls)}   ({np.median(walls) / len(ss):.3f} ms per scan)")
    if not a.no_cpu:
        for name, (ts, counts) in cpu_serial(groups, a).items():
            print(f"loam_features.h serial loop on one CPU core, {name}: {stats(ts)}   ({counts.split()[1]} in the first scan)")


if __name__ == "__main__":
    main()
