"""Times the GICP loop-closure alignment through the C-ABI at the shipped parameters (config/matchers/gicp.json and PCL's defaults,
capi.GICP_DEFAULTS): bsgpu_register_scans_gicp on one pair of aggregated scans — each the union of 21 VLP-16 revolutions (16 rings x
1 812 azimuths) cast from inside the 20 x 14 x 5 m room from poses along a path, brought into the centre revolution's frame, 1 cm range
noise, voxel-reduced here (NumPy, cell centroids) to 0.05 m and then to 0.1 m as the reference's filters and the matcher's res do — and
on four candidate pairs against one query in one call.  Each figure is taken twice: HIP events recorded around the blocking call (the
device clock over upload, kernels and download), and the host clock around the same call.  Median and range of --reps calls after a
warm-up, per --grid-cell value (a performance knob only: the results are asserted equal, bit for bit).  Beside them the wall time of
the shared header's serial loop (gicp.h on one core: grids, covariances and iterations, g++ -O2 -march=native) on the same inputs.  The
kernels' own time comes from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_register_gicp.py --reps 3 --no-cpu --grid-cell 0.5
    python scripts/time_register_gicp.py [--reps 10]"""
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
from test_gicp import reg_command  # noqa: E402
from time_register_scans import HipEvents, revolution, stats  # noqa: E402
from beam_slam_amd import capi, gpu  # noqa: E402


def voxel(P, leaf):
    """the centroid of the points of every occupied cell of edge `leaf` (pcl::VoxelGrid's rule), in the order of the cells' keys"""
    key = np.floor(P / leaf).astype(np.int64)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    return np.stack([np.bincount(inv, weights=P[:, a]) / cnt for a in range(3)], axis=1)


def pose(r, t):
    return np.hstack([ref.rotvec(r), np.asarray(t, float)[:, None]])


def compose(A, B):
    return np.hstack([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]])


def inverse(A):
    return np.hstack([A[:, :3].T, (-A[:, :3].T @ A[:, 3])[:, None]])


def aggregate(centre, rng, n=21, step=0.12):
    """n revolutions from poses along a straight path through `centre` (step m apart, a slow yaw), in the centre's frame, filtered"""
    clouds = []
    for k in range(-(n // 2), n // 2 + 1):
        T = compose(centre, pose([0.0, 0.0, 0.01 * k], [step * k, 0.02 * k, 0.0]))
        rel = compose(inverse(centre), T)
        clouds.append(ref.transform(rel, revolution(T, rng)))
    return voxel(voxel(np.concatenate(clouds), 0.05), 0.1)


def cpu_serial(groups, a, grid_cell):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "time_gicp_cpu")
        subprocess.check_call(["g++", "-O2", "-march=native", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                               os.path.join(ROOT, "scripts", "time_gicp_cpu.cpp"), "-o", exe])
        out = {}
        params = {k: v for k, v in capi.GICP_DEFAULTS.items() if k != "grid_cell"}
        for name, pairs in groups:
            path = os.path.join(tmp, "pairs.bin")
            np.concatenate([reg_command(S, Q, T_init=Ti, grid_cell=grid_cell, **params) for S, Q, Ti in pairs]).tofile(path)
            txt = subprocess.run([exe, str(a.cpu_reps), path], capture_output=True, text=True, check=True).stdout.splitlines()
            out[name] = ([float(ln.split()[1]) for ln in txt if ln.startswith("MS")], txt[-2], txt[-1])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--grid-cell", type=float, nargs="+", default=[0.25, 0.5, 1.0])
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    # the query aggregate, and candidate aggregates from an earlier pass a few decimetres away; the pose estimates carry drift, so
    # that T_init brings the query within reach and the matcher has a correction to find
    T_query = pose([0.01, -0.02, 0.04], [0.25, -0.15, 0.05])
    query = aggregate(T_query, rng)
    pairs = []
    for k in range(a.pairs):
        T_cand = pose([0.004 * k, 0.0, -0.01 * k], [-0.2 * k, 0.1 * k, 0.0])
        T_est = compose(inverse(T_cand), T_query)
        T_est = np.hstack([ref.rotvec([0.006, -0.004, 0.02]) @ T_est[:, :3], (T_est[:, 3] + [0.15, -0.1, 0.04])[:, None]])
        pairs.append((aggregate(T_cand, rng), query, T_est))
    groups = [(f"1 pair of {len(pairs[0][0])} x {len(query)} points", pairs[:1]), (f"{a.pairs} candidate pairs in one call", pairs)]
    ev = HipEvents()
    for name, ps in groups:
        rs, ts = np.cumsum([0] + [len(p[0]) for p in ps]), np.cumsum([0] + [len(p[1]) for p in ps])
        rp, tp, ti = np.concatenate([p[0] for p in ps]), np.concatenate([p[1] for p in ps]), np.stack([p[2] for p in ps])
        first = None
        for h in a.grid_cell:
            call = lambda: gpu.register_scans_gicp(rs, rp, ts, tp, ti, grid_cell=h, covariances=False)
            out = call()
            if first is None:
                first = out
                print(f"register_scans_gicp {name} (source points {[int(v) for v in np.diff(rs)]}): status {list(out['status'])}, "
                      f"outer / inner iterations {list(zip(out['n_iters'].tolist(), out['n_inner'].tolist()))}, correspondences {list(out['n_corr'])}, "
                      f"cost {[float(f'{m:.3e}') for m in out['cost']]}")
            assert all(out[k].tobytes() == first[k].tobytes() for k in first), "grid_cell changed a result"
            evs, walls = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                evs.append(ev.time_ms(call))
                walls.append(1e3 * (time.perf_counter() - t0))
            print(f"  grid_cell {h}:")
            print(f"    HIP events around the call: {stats(evs)}")
            print(f"    host clock around the call: {stats(walls)}   ({np.median(walls) / len(ps):.3f} ms per pair)")
    if not a.no_cpu:
        for name, (ts, iters, status) in cpu_serial(groups, a, capi.GICP_DEFAULTS["grid_cell"]).items():
            print(f"gicp.h serial loop on one CPU core, {name}: {stats(ts)}   ({iters}; {status})")


if __name__ == "__main__":
    main()
