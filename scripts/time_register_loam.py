"""Times the LOAM feature registration through the C-ABI at the shipped parameters (config/matchers/loam_vlp16.json and
config/optimization/ceres_config.json, capi.LOAM_DEFAULTS): bsgpu_register_scans_loam scan-to-scan (a scan's features against the
previous scan's) and scan-to-map (against the features of 20 earlier scans in one frame), each as 1 pair and as 10 pairs in one call.
The scans are VLP-16 revolutions (16 rings x 1 812 azimuths) cast from inside the 20 x 14 x 5 m room of the tests, 1 cm range noise; the
features are the library's own: bsgpu_extract_loam_features at the shipped parameters (capi.LOAM_FEATURE_DEFAULTS), ring by elevation,
all scans of the path in one call, and of its output the STRONG clouds, which is what every shipped matcher file registers.
Each figure is taken twice: HIP events recorded around the blocking call (the device clock over upload, kernels and download), and the
host clock around the same call.  Median and range of --reps calls after a warm-up.  Beside them the wall time of the shared header's
serial loop (loam.h on one core, g++ -O2 -march=native) on the same inputs: the only baseline there is, since libbeam's matcher is not
in the reference checkout.  The kernels' own time comes from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_register_loam.py --reps 3 --no-cpu
    python scripts/time_register_loam.py [--reps 20]"""
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
import icp_ref as ref  # noqa: E402
from test_loam import reg_command  # noqa: E402
from time_register_scans import HipEvents, revolution, stats  # noqa: E402
from time_register_gicp import compose, inverse, pose  # noqa: E402
from beam_slam_amd import capi, gpu  # noqa: E402

def features(clouds):
    """[(edges, surfaces)] of the revolutions: the strong clouds of one bsgpu_extract_loam_features call"""
    out = gpu.extract_loam_features(np.cumsum([0] + [len(c) for c in clouds]), np.concatenate(clouds), weak=False, labels=False, curvature=False)
    es, ss = out["edge_start"], out["surf_start"]
    return [(out["edge_points"][es[k]:es[k + 1]].copy(), out["surf_points"][ss[k]:ss[k + 1]].copy()) for k in range(len(clouds))]


def cpu_serial(groups, a, params):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "time_loam_cpu")
        subprocess.check_call(["g++", "-O2", "-march=native", "-ffp-contract=off", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I",
                               os.path.join(ROOT, "beam_slam_amd", "csrc"), os.path.join(ROOT, "scripts", "time_loam_cpu.cpp"), "-o", exe])
        out = {}
        for name, pairs in groups:
            path = os.path.join(tmp, "pairs.bin")
            np.concatenate([reg_command(c, T_init=Ti, **params) for c, Ti in pairs]).tofile(path)
            txt = subprocess.run([exe, str(a.cpu_reps), path], capture_output=True, text=True, check=True).stdout.splitlines()
            out[name] = ([float(ln.split()[1]) for ln in txt if ln.startswith("MS")], txt[-2], txt[-1])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--map-scans", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    # a path through the room: a scan every 12 cm with a slow yaw; the pose estimates carry drift, so that T_init brings the target
    # within reach and the matcher has a correction to find
    n_scans = a.map_scans + a.pairs
    poses = [pose([0.0, 0.0, 0.01 * k], [-2.0 + 0.12 * k, 0.02 * k, 0.0]) for k in range(n_scans + 1)]
    feats = features([revolution(T, rng) for T in poses])
    drift = pose([0.003, -0.002, 0.006], [0.04, -0.03, 0.01])
    scan_pairs, map_pairs = [], []
    for k in range(a.map_scans, a.map_scans + a.pairs):
        tgt = feats[k + 1]
        T_est = compose(compose(inverse(poses[k]), poses[k + 1]), drift)
        scan_pairs.append(((feats[k][0], feats[k][1], tgt[0], tgt[1]), T_est))
        # the map: the features of the map_scans scans before the target, in scan k's frame
        me = np.concatenate([ref.transform(compose(inverse(poses[k]), poses[j]), feats[j][0]) for j in range(k - a.map_scans + 1, k + 1)])
        ms = np.concatenate([ref.transform(compose(inverse(poses[k]), poses[j]), feats[j][1]) for j in range(k - a.map_scans + 1, k + 1)])
        map_pairs.append(((me, ms, tgt[0], tgt[1]), T_est))
    groups = [("scan-to-scan, 1 pair", scan_pairs[:1]), (f"scan-to-scan, {a.pairs} pairs in one call", scan_pairs),
              (f"scan-to-map of {a.map_scans} scans, 1 pair", map_pairs[:1]), (f"scan-to-map of {a.map_scans} scans, {a.pairs} pairs in one call", map_pairs)]
    params = {k: v for k, v in capi.LOAM_DEFAULTS.items() if k not in ("grid_cell", "inner")}
    ev = HipEvents()
    for name, ps in groups:
        args = []
        for c in range(4):
            args += [np.cumsum([0] + [len(p[0][c]) for p in ps]), np.concatenate([p[0][c] for p in ps])]
        ti = np.stack([p[1] for p in ps])
        call = lambda: gpu.register_scans_loam(*args, ti, **params)
        out = call()
        print(f"register_scans_loam {name} (reference {len(ps[0][0][0])} + {len(ps[0][0][1])}, target {len(ps[0][0][2])} + {len(ps[0][0][3])} features): "
              f"status {list(out['status'])}, outer / inner iterations {list(zip(out['n_iters'].tolist(), out['n_inner'].tolist()))}, "
              f"kept {list(zip(out['n_edge'].tolist(), out['n_surf'].tolist()))}, cost {[float(f'{m:.3e}') for m in out['cost']]}")
        evs, walls = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            evs.append(ev.time_ms(call))
            walls.append(1e3 * (time.perf_counter() - t0))
        print(f"    HIP events around the call: {stats(evs)}")
        print(f"    host clock around the call: {stats(walls)}   ({np.median(walls) / len(ps):.3f} ms per pair)")
    if not a.no_cpu:
        for name, (ts, iters, status) in cpu_serial(groups, a, params).items():
            print(f"loam.h serial loop on one CPU core, {name}: {stats(ts)}   ({iters}; {status})")


if __name__ == "__main__":
    main()
