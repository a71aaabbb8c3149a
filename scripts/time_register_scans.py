"""Times the ICP scan registration through the C-ABI at the shipped ICP parameters (config/matchers/icp.json): bsgpu_register_scans on
one pair of VLP-16 revolutions (16 rings x 1 812 azimuths = 28 992 points each, cast from inside a 20 x 14 x 5 m room, the second from
a pose 0.25 m and 2.6 degrees away, 1 cm range noise), and on three such pairs in one call (the reference's num_neighbors = 3).  Each
figure is taken twice: HIP events recorded around the blocking call (the device clock over upload, kernels and download), and the host
clock around the same call.  Median and range of --reps calls after a warm-up.  Beside them the wall time of the shared header's
serial loop (icp.h on one core: grid build and iterations, g++ -O2 -march=native) on the same inputs.  The kernels' own time comes from
a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_register_scans.py --reps 5 --no-cpu
    python scripts/time_register_scans.py [--reps 30]"""
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
import icp_ref as ref  # noqa: E402
from test_icp import reg_command  # noqa: E402
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
    return f"median {np.median(ts):8.3f} ms  (min {np.min(ts):.3f}, max {np.max(ts):.3f}, n = {len(ts)})"


def revolution(T_world_lidar, rng, rings=16, azimuths=1812, sigma=0.01):
    """One VLP-16 revolution from inside the room of the tests (icp_ref.BOX, centred at the origin): rings at -15 .. +15 degrees, each
    ray cast to the first wall, range noise sigma; the points in the lidar's frame."""
    R, t = T_world_lidar[:, :3], T_world_lidar[:, 3]
    el = np.deg2rad(np.linspace(-15.0, 15.0, rings))[:, None]
    az = np.linspace(0.0, 2.0 * np.pi, azimuths, endpoint=False)[None, :]
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=2).reshape(-1, 3)
    dw = d @ R.T
    with np.errstate(divide="ignore", invalid="ignore"):
        hit = np.where(dw > 0, (0.5 * ref.BOX - t) / dw, np.where(dw < 0, (-0.5 * ref.BOX - t) / dw, np.inf))
    rng_m = hit.min(axis=1) + sigma * rng.standard_normal(len(d))
    cloud = d * rng_m[:, None]
    assert np.isfinite(cloud).all()
    return cloud


def cpu_serial(groups, a):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "time_icp_cpu")
        subprocess.check_call(["g++", "-O2", "-march=native", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "beam_slam_amd", "csrc"),
                               os.path.join(ROOT, "scripts", "time_icp_cpu.cpp"), "-o", exe])
        out = {}
        for name, pairs in groups:
            path = os.path.join(tmp, "pairs.bin")
            np.concatenate([reg_command(S, Q, T_init=Ti, **capi.ICP_DEFAULTS) for S, Q, Ti in pairs]).tofile(path)
            txt = subprocess.run([exe, str(a.cpu_reps), path], capture_output=True, text=True, check=True).stdout.splitlines()
            out[name] = ([float(ln.split()[1]) for ln in txt if ln.startswith("MS")], txt[-2], txt[-1])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    pose = lambda r, t: np.hstack([ref.rotvec(r), np.asarray(t, float)[:, None]])
    T_tgt = pose([0.01, -0.02, 0.04], [0.25, -0.15, 0.05])
    tgt = revolution(T_tgt, rng)
    # the neighbours: earlier scans from poses a few decimetres back along the same motion; the pose estimates carry the odometry's
    # error, so that T_init brings the target within reach and ICP has a correction to find
    pairs = []
    for k in range(a.pairs):
        T_ref = pose([0.004 * k, 0.0, -0.01 * k], [-0.2 * k, 0.1 * k, 0.0])
        R, t = T_ref[:, :3], T_ref[:, 3]
        T_est = np.hstack([R.T @ T_tgt[:, :3], (R.T @ (T_tgt[:, 3] - t))[:, None]])       # inv(T_ref) T_tgt ...
        T_est = np.hstack([ref.rotvec([0.003, -0.002, 0.01]) @ T_est[:, :3], (T_est[:, 3] + [0.06, -0.04, 0.02])[:, None]])   # ... with an error
        pairs.append((revolution(T_ref, rng), tgt, T_est))
    groups = [(f"1 pair of 2 x {len(tgt)} points", pairs[:1]), (f"{a.pairs} such pairs in one call", pairs)]
    ev = HipEvents()
    for name, ps in groups:
        rs, ts = np.cumsum([0] + [len(p[0]) for p in ps]), np.cumsum([0] + [len(p[1]) for p in ps])
        rp, tp, ti = np.concatenate([p[0] for p in ps]), np.concatenate([p[1] for p in ps]), np.stack([p[2] for p in ps])
        call = lambda: gpu.register_scans(rs, rp, ts, tp, ti)
        out = call()
        call()
        evs, walls = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            evs.append(ev.time_ms(call))
            walls.append(1e3 * (time.perf_counter() - t0))
        print(f"register_scans {name}: status {list(out['status'])}, iterations {list(out['n_iters'])}, correspondences {list(out['n_corr'])}, "
              f"mse {[float(f'{m:.3e}') for m in out['mse']]}")
        print(f"    HIP events around the call: {stats(evs)}")
        print(f"    host clock around the call: {stats(walls)}   ({np.median(walls) / len(ps):.3f} ms per pair)")
    if not a.no_cpu:
        for name, (ts, iters, status) in cpu_serial(groups, a).items():
            print(f"icp.h serial loop on one CPU core, {name}: {stats(ts)}   ({iters}; {status})")


if __name__ == "__main__":
    main()
