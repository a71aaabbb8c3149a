"""Times bsgpu_build_registration_maps through the C-ABI on three shapes:
  (a) the shipped scan-to-map LOAM map (registration/scan_to_map.json: map_size 45, leaf 0.1 m): bsgpu_extract_loam_features' strong
      features of 45 cast VLP-16 revolutions, two classes (edges, surfaces) in one call;
  (b) the slow configuration (scan_to_map_slow.json): 200 scans;
  (c) a loop-closure aggregate: 21 whole revolutions of 28 992 points at leaf 0.1 m, as one map and as four maps in one call.
The scans are the revolutions of time_register_loam.py (16 rings x 1 812 azimuths cast from inside the 20 x 14 x 5 m room of the tests
along a path, 1 cm range noise), each in its own frame with its pose as T_map_scan.
Each figure is taken twice: HIP events recorded around the blocking call (the device clock over upload, kernels and download), and the
host clock around the same call, which also holds the packing into the caller's arrays.  Median and range of --reps calls after a
warm-up.  Beside them the wall time of the shared header's serial contract (registration_map.h on one core, g++ -O2 -march=native) on
the same input: the only baseline there is, since libbeam's VoxelDownsample is not in the reference checkout.  The kernels' own time
comes from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_registration_map.py --reps 3 --no-cpu
    python scripts/time_registration_map.py [--reps 20]"""
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
from test_registration_map import map_command, stack_scans  # noqa: E402
from time_register_scans import HipEvents, revolution, stats  # noqa: E402
from time_register_gicp import pose  # noqa: E402
from beam_slam_amd import gpu  # noqa: E402


def cpu_serial(runs, a):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "time_registration_map_cpu")
        subprocess.check_call(["g++", "-O2", "-march=native", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                               os.path.join(ROOT, "scripts", "time_registration_map_cpu.cpp"), "-o", exe])
        out = {}
        for name, run in runs:
            path = os.path.join(tmp, "call.bin")
            map_command(*run).tofile(path)
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
    poses = [pose([0.0, 0.0, 0.004 * k], [-5.0 + 0.05 * k, 0.01 * k, 0.0]) for k in range(200)]
    scans = [revolution(T, rng) for T in poses]
    feats = [gpu.extract_loam_features(np.cumsum([0] + [len(s) for s in scans[b:b + 20]]), np.concatenate(scans[b:b + 20]), weak=False, labels=False,
                                       curvature=False) for b in range(0, 200, 20)]
    edges = [f["edge_points"][f["edge_start"][k]:f["edge_start"][k + 1]] for f in feats for k in range(20)]
    surfs = [f["surf_points"][f["surf_start"][k]:f["surf_start"][k + 1]] for f in feats for k in range(20)]
    T = np.stack(poses)
    runs = []
    for name, n in (("(a) LOAM map of 45 scans", 45), ("(b) LOAM map of 200 scans", 200)):
        runs.append((name, stack_scans([edges[:n], surfs[:n]]) + (np.concatenate([T[:n], T[:n]]), 0.1)))
    runs.append(("(c) aggregate of 21 revolutions, one map", stack_scans([scans[:21]]) + (T[:21], 0.1)))
    runs.append(("(c) aggregates of 21 revolutions, four maps in one call", stack_scans([scans[b:b + 21] for b in (0, 40, 80, 120)]) +
                 (np.concatenate([T[b:b + 21] for b in (0, 40, 80, 120)]), 0.1)))
    ev = HipEvents()
    for name, run in runs:
        call = lambda: gpu.build_registration_maps(*run)
        out = call()
        print(f"build_registration_maps {name}: {len(run[2])} points in {len(run[1]) - 1} scans -> {np.diff(out['map_start']).tolist()} voxels")
        evs, walls = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            evs.append(ev.time_ms(call))
            walls.append(1e3 * (time.perf_counter() - t0))
        print(f"    HIP events around the call: {stats(evs)}")
        print(f"    host clock around the call: {stats(walls)}")
    if not a.no_cpu:
        for name, (ts, counts) in cpu_serial(runs, a).items():
            print(f"registration_map.h serial contract on one CPU core, {name}: {stats(ts)}   ({counts})")


if __name__ == "__main__":
    main()
