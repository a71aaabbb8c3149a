"""Times the Scan Context loop-closure search through the C-ABI at the shipped shape (reloc_candidate_search_scan_context.json, SCManager's
constants): a query submap and a candidate submap of 30 lidar keyframes each, every keyframe aggregated with its num_scans_to_aggregate =
20 neighbours by GetTimesToAggregate's rule (11 members at a submap's ends, 21 in its middle), VLP-16 revolutions of 16 x 1 812 = 28 992
points cast from inside the tests' place A; then 30 queries against 30 candidates with K = 10 and search_ratio 0.1.
bsgpu_scan_context_describe (one call: 60 scans, 60 aggregates) and bsgpu_scan_context_match (one call: one set) are each timed twice: HIP
events recorded around the blocking call (the device clock over upload, kernels and download) and the host clock around the same call.
Median and range of --reps calls after a warm-up.  Beside them the wall time of the shared header's serial loops (scan_context.h on one
core, g++ -O2 -march=native) on the same inputs, and the kernels' own times from a profiler run of this script's own (a child process
under rocprofv3 --kernel-trace --stats; --no-profile leaves it out).
    python scripts/time_scan_context.py [--reps 20]"""
import argparse
import csv
import ctypes
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_context_ref as ref  # noqa: E402
from scan_context_ref import describe_command  # noqa: E402
from beam_slam_amd import capi, gpu  # noqa: E402


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
    return f"median {np.median(ts):9.3f} ms  (min {np.min(ts):.3f}, max {np.max(ts):.3f}, n = {len(ts)})"


def ids_to_aggregate(n_keyframes, center, n_agg=20):
    """GetTimesToAggregate (reloc_candidate_search_scan_context.cpp:292-311) as positions."""
    return [k for k in range(center - n_agg // 2, center + n_agg // 2 + 1) if 0 <= k < n_keyframes and k != center]


def submaps(n_keyframes, points):
    """(scans, aggregates): the candidate submap's keyframes along a 6 m path through place A, the query's along the same
    path 10 cm aside and turned by 93 degrees; aggregates as lists of (scan, T_ScanCenter_ScanToAgg), the centre first."""
    poses = []
    for side, yaw in ((0.0, 0.0), (0.1, 93.0)):
        for k in range(n_keyframes):
            poses.append(np.hstack([ref.rotz(yaw + 0.5 * k), [[-3.0 + 6.0 * k / (n_keyframes - 1)], [0.5 + side + 0.02 * k], [ref.SENSOR_Z]]]))
    scans = [ref.cast("A", T[0, 3], T[1, 3], np.degrees(np.arctan2(T[1, 0], T[0, 0])), n=points, seed=k) for k, T in enumerate(poses)]
    inv = lambda T: np.hstack([T[:, :3].T, -T[:, :3].T @ T[:, 3:]])
    mul = lambda A, B: np.hstack([A[:, :3] @ B[:, :3], A[:, :3] @ B[:, 3:] + A[:, 3:]])
    aggregates = []
    for first in (n_keyframes, 0):                  # the query's aggregates first, then the candidates'
        for c in range(n_keyframes):
            aggregates.append([(first + c, ref.EYE)] + [(first + k, mul(inv(poses[first + c]), poses[first + k])) for k in ids_to_aggregate(n_keyframes, c)])
    return scans, aggregates


def kernel_times(a):
    """The kernels' own times: this script again, as a child under the profiler, with few repetitions and nothing else."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "sc", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--reps", "3", "--no-cpu", "--no-profile", "--keyframes", str(a.keyframes), "--points", str(a.points)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            print(f"kernel times: the profiler run failed (exit {r.returncode}): {r.stderr[-500:]}")
            return
        print("kernel times (rocprofv3 --kernel-trace --stats, name, calls, average us, total us):")
        for row in csv.DictReader(open(files[0])):
            if "sc_" in row["Name"]:
                print(f"    {row['Name'].split('(')[0]:40s} {row['Calls']:>5s} {float(row['AverageNs']) / 1e3:10.1f} {float(row['TotalDurationNs']) / 1e3:12.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--keyframes", type=int, default=30)
    ap.add_argument("--points", type=int, default=16 * 1812)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    scans, aggregates = submaps(a.keyframes, a.points)
    nq = a.keyframes
    ss = np.cumsum([0] + [len(s) for s in scans])
    ms = np.cumsum([0] + [len(m) for m in aggregates])
    pts = np.concatenate(scans)
    mscan = np.array([k for m in aggregates for k, _ in m], np.int32)
    mT = np.stack([T for m in aggregates for _, T in m])
    sc = capi.SC_DEFAULTS
    describe = lambda: gpu.scan_context_describe(ss, pts, ms, mscan, mT, sc["lidar_height"], sc["max_radius"])
    d = describe()
    match = lambda: gpu.scan_context_match([0, nq], d["desc"][:nq], [0, len(aggregates) - nq], d["desc"][nq:], sc["n_tree_candidates"],
                                           sc["search_ratio"], sc["dist_thres"])
    m = match()
    ev = HipEvents()
    print(f"{len(scans)} scans of {a.points} points, {len(aggregates)} aggregates of {ms[1]} .. {np.diff(ms).max()} members ({int(ms[-1])} members, "
          f"{int(sum(len(scans[k]) for k in mscan)) / 1e6:.1f} M point transforms); {nq} queries x {len(aggregates) - nq} candidates")
    print(f"best_cand {[int(v) for v in m['best_cand']]}")
    print(f"best_dist {[float(f'{v:.3f}') for v in m['best_dist']]}, best_shift {[int(v) for v in m['best_shift']]}")
    for name, call in (("scan_context_describe", describe), ("scan_context_match", match)):
        evs, walls = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            evs.append(ev.time_ms(call))
            walls.append(1e3 * (time.perf_counter() - t0))
        print(f"{name}:\n    HIP events around the call: {stats(evs)}\n    host clock around the call: {stats(walls)}")
    if not a.no_cpu:
        with tempfile.TemporaryDirectory() as tmp:
            exe, path = os.path.join(tmp, "time_scan_context_cpu"), os.path.join(tmp, "describe.bin")
            subprocess.check_call(["g++", "-O2", "-march=native", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                                   os.path.join(ROOT, "scripts", "time_scan_context_cpu.cpp"), "-o", exe])
            describe_command(scans, aggregates, sc["lidar_height"], sc["max_radius"]).tofile(path)
            txt = subprocess.run([exe, str(a.cpu_reps), path, str(nq), str(sc["n_tree_candidates"]), str(sc["search_ratio"]), str(sc["dist_thres"])],
                                 capture_output=True, text=True, check=True).stdout.splitlines()
            t = np.array([[float(v) for v in ln.split()[1:]] for ln in txt if ln.startswith("MS")])
            same = [int(v) for v in txt[-2].split()[1:]] == list(m["best_cand"])
            print(f"scan_context.h serial loops on one CPU core: describe {stats(t[:, 0])}\n"
                  f"                                             match    {stats(t[:, 1])}   (best_cand equal to the device's: {same})")
    if not a.no_profile:
        kernel_times(a)


if __name__ == "__main__":
    main()
