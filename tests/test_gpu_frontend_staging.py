"""What the packing of the front-end entry points (beam_slam_amd/csrc/bsgpu_frontend.cpp on staging.h) can get wrong and their kernels
cannot: an output segment that moves or goes missing with the optional outputs the caller asks for, and an item whose neighbours are
empty.  Through the raw C-ABI, every output array pre-filled with 0x5A bytes so that what is compared was written by the call.

Shapes: three items per call, sizes (0, m, 0) and (m, 0, m); m = 12 matches (five-point), 12 pairs (P3P), 16 matches (seven-point),
8 observations (localisation, min_points 4), 3 views per track, 4 frames with 44 IMU samples, 10 samples per pre-integrated interval.
Every non-empty item must come back with status 0: the comparisons are of computed results.

bsgpu_preintegrate, bsgpu_inertial_alignment and bsgpu_triangulate have no optional output; for them test_optional_outputs compares two
calls, and test_empty_items is what tests their packing."""
import ctypes as C

import numpy as np
import pytest

import align_ref
import essential_ref
import frame_cases
import p3p_ref
import seven_point_ref
from beam_slam_amd import capi, synthetic

pytestmark = pytest.mark.gpu
SEED = 77
_TYPES = {np.dtype(np.int32): capi._ip, np.dtype(np.float64): capi._dp, np.dtype(np.uint8): capi._bp}


def _p(a):
    return None if a is None else a.ctypes.data_as(_TYPES[a.dtype])


def _starts(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _cat(items, key, width):
    return np.ascontiguousarray(np.concatenate([np.zeros((0, width))] + [np.asarray(it[key], float).reshape(-1, width) for it in items if it]))


class Call:
    """One entry point: `outputs` name -> (dtype, "item" | "elem", values per item or element), `optional` the names that may be NULL,
    run(items, out) -> return code, with out[name] an array or None.  An item is a dict, or None for an empty one."""
    optional = ()

    def size(self, item):
        raise NotImplementedError

    def __call__(self, items, want=None):
        """-> {name: per-item list of arrays} of the outputs given: the required ones and those of `want` (None: all)."""
        sizes = [self.size(it) if it else 0 for it in items]
        st = _starts(sizes)
        out = {}
        for name, (dtype, per, width) in self.outputs.items():
            given = name not in self.optional or want is None or name in want
            out[name] = np.frombuffer(bytearray(b"\x5a" * ((len(items) if per == "item" else int(st[-1])) * width * np.dtype(dtype).itemsize)), dtype) if given else None
        assert self.run(items, st, out) == capi.OK
        res = {}
        for name, a in out.items():
            _, per, w = self.outputs[name]
            if a is not None:
                res[name] = [a[k * w:(k + 1) * w] if per == "item" else a[st[k] * w:st[k + 1] * w] for k in range(len(items))]
        return res


class Essential(Call):
    outputs = dict(mask=(np.uint8, "elem", 1), status=(np.int32, "item", 1), E=(np.float64, "item", 9), n_inliers=(np.int32, "item", 1),
                   n_iters=(np.int32, "item", 1), best_sample=(np.int32, "item", 5))
    optional = ("E", "n_inliers", "n_iters", "best_sample")
    size = staticmethod(lambda it: len(it["px_prev"]))
    make = staticmethod(lambda k: essential_ref.make_set(500 + k, 12, 0.25))

    def __init__(self, g, lib):
        self.g, self.fn = g, lib.bsgpu_essential_ransac
        self.fn.argtypes = capi.ESSENTIAL_RANSAC_ARGTYPES

    def run(self, items, st, o):
        K = np.array([it["K"] if it else essential_ref.K_DEFAULT for it in items], float)
        return self.fn(self.g._ctx, len(items), _p(st), _p(_cat(items, "px_prev", 2)), _p(_cat(items, "px_cur", 2)), _p(K), 0.99, 1.0, 200, SEED,
                       _p(o["mask"]), _p(o["E"]), _p(o["n_inliers"]), _p(o["n_iters"]), _p(o["best_sample"]), _p(o["status"]))


class AbsolutePose(Call):
    outputs = dict(mask=(np.uint8, "elem", 1), q=(np.float64, "item", 4), p=(np.float64, "item", 3), status=(np.int32, "item", 1),
                   T_cam_world=(np.float64, "item", 12), n_inliers=(np.int32, "item", 1), n_iters=(np.int32, "item", 1),
                   best_sample=(np.int32, "item", 3))
    optional = ("T_cam_world", "n_inliers", "n_iters", "best_sample")
    size = staticmethod(lambda it: len(it["pixels"]))
    make = staticmethod(lambda k: p3p_ref.make_frame(600 + k, 12, 3))

    def __init__(self, g, lib):
        self.g, self.fn = g, lib.bsgpu_absolute_pose_ransac
        self.fn.argtypes = capi.ABSOLUTE_POSE_RANSAC_ARGTYPES

    def run(self, items, st, o):
        cam = np.zeros(len(items), np.int32)
        return self.fn(self.g._ctx, len(items), _p(st), _p(_cat(items, "pixels", 2)), _p(_cat(items, "points", 3)), _p(cam), 0.99, 5.0, 100, SEED, 0,
                       _p(o["mask"]), _p(o["q"]), _p(o["p"]), _p(o["T_cam_world"]), _p(o["n_inliers"]), _p(o["n_iters"]), _p(o["best_sample"]),
                       _p(o["status"]))


class RelativePose(Call):
    outputs = dict(mask=(np.uint8, "elem", 1), q=(np.float64, "item", 8), p=(np.float64, "item", 6), pair_valid=(np.int32, "item", 1),
                   status=(np.int32, "item", 1), T_last_first=(np.float64, "item", 12), points=(np.float64, "elem", 3),
                   valid_mask=(np.uint8, "elem", 1), inlier_ratio=(np.float64, "item", 1), n_inliers=(np.int32, "item", 1),
                   n_iters=(np.int32, "item", 1), best_sample=(np.int32, "item", 7))
    optional = ("T_last_first", "points", "valid_mask", "inlier_ratio", "n_inliers", "n_iters", "best_sample")
    size = staticmethod(lambda it: len(it["px_first"]))
    make = staticmethod(lambda k: seven_point_ref.make_pair(700 + k, 16, 4))

    def __init__(self, g, lib):
        self.g, self.fn = g, lib.bsgpu_relative_pose_ransac
        self.fn.argtypes = capi.RELATIVE_POSE_RANSAC_ARGTYPES

    def run(self, items, st, o):
        cam = np.zeros(len(items), np.int32)
        return self.fn(self.g._ctx, len(items), _p(st), _p(_cat(items, "px_first", 2)), _p(_cat(items, "px_last", 2)), _p(cam), 0.99, 5.0, 100, SEED,
                       0, 10.0, 0.5, _p(o["mask"]), _p(o["T_last_first"]), _p(o["q"]), _p(o["p"]), _p(o["points"]), _p(o["valid_mask"]),
                       _p(o["inlier_ratio"]), _p(o["pair_valid"]), _p(o["n_inliers"]), _p(o["n_iters"]), _p(o["best_sample"]), _p(o["status"]))


class Localize(Call):
    outputs = dict(q=(np.float64, "item", 4), p=(np.float64, "item", 3), status=(np.int32, "item", 1), cov=(np.float64, "item", 36),
                   avg_reproj=(np.float64, "item", 1), final_cost=(np.float64, "item", 1), iterations=(np.int32, "item", 1))
    optional = ("cov", "avg_reproj", "final_cost", "iterations")
    size = staticmethod(lambda it: len(it["pixels"]))
    make = staticmethod(lambda k: frame_cases.make_frame(800 + k, 8, 2.0, 0.1))

    def __init__(self, g, lib):
        self.g, self.fn = g, lib.bsgpu_localize_frames
        dp, ip = capi._dp, capi._ip
        self.fn.argtypes = [C.c_void_p, C.c_int32, ip, dp, dp, ip, ip, dp, dp, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                            C.c_int32, C.POINTER(capi.Options), dp, dp, dp, dp, dp, ip, ip]

    def run(self, items, st, o):
        cam = np.zeros(len(items), np.int32)
        qi = np.array([it["q_init"] if it else [1.0, 0, 0, 0] for it in items], float)
        pi = np.array([it["p_init"] if it else [0.0, 0, 0] for it in items], float)
        opts = self.g.options_default()
        return self.fn(self.g._ctx, len(items), _p(st), _p(_cat(items, "pixels", 2)), _p(_cat(items, "points", 3)), None, _p(cam), _p(qi), _p(pi),
                       capi.LOSS_HUBER, 2.0, 1.0, 0, 4, frame_cases.WIDTH, frame_cases.HEIGHT, C.byref(opts), _p(o["q"]), _p(o["p"]), _p(o["cov"]),
                       _p(o["avg_reproj"]), _p(o["final_cost"]), _p(o["iterations"]), _p(o["status"]))


class Triangulate(Call):
    outputs = dict(points=(np.float64, "item", 3), status=(np.int32, "item", 1))
    size = staticmethod(lambda it: len(it["q_block"]))

    def __init__(self, g, lib):
        """Its own context: a small window's poses on the device; the items are that window's first tracks of three views or more,
        cut to three."""
        self.g, self.fn = g, lib.bsgpu_triangulate
        self.fn.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        pr = synthetic.vio_window(n_kf=6, n_lm=40, seed=2)
        pr.load(g)
        idx = np.concatenate([f[0] for f in pr.factors[capi.F_REPROJ]])
        consts = np.concatenate([f[1] for f in pr.factors[capi.F_REPROJ]])
        lms, counts = np.unique(idx[:, 2], return_counts=True)
        self.tracks = []
        for lm in lms[counts >= 3][:3]:
            rows = np.flatnonzero(idx[:, 2] == lm)[:3]
            self.tracks.append(dict(q_block=idx[rows, 0].astype(np.int32), p_block=idx[rows, 1].astype(np.int32), pixels=consts[rows, :2].copy()))
        assert len(self.tracks) == 3

    def make(self, k):
        return self.tracks[k]

    def run(self, items, st, o):
        blocks = lambda key: np.ascontiguousarray(np.concatenate([np.zeros(0, np.int32)] + [it[key] for it in items if it]), np.int32)
        qb, pb, px = blocks("q_block"), blocks("p_block"), _cat(items, "pixels", 2)
        return self.fn(self.g._ctx, len(items), st.ctypes.data, qb.ctypes.data, pb.ctypes.data, px.ctypes.data, 0, 1, -1.0, -1.0,
                       o["points"].ctypes.data, o["status"].ctypes.data)


class Alignment(Call):
    outputs = dict(gravity=(np.float64, "item", 3), bg=(np.float64, "item", 3), scale=(np.float64, "item", 1), excitation=(np.float64, "item", 1),
                   gyro_rank=(np.int32, "item", 1), status=(np.int32, "item", 1), velocity=(np.float64, "elem", 3), q_out=(np.float64, "elem", 4),
                   p_out=(np.float64, "elem", 3), v_out=(np.float64, "elem", 3))
    size = staticmethod(lambda it: len(it["tf"]))
    # 4 frames 50 ms apart from 52 ms on, samples at 200 Hz from 0 to three past the last frame: 44 of them
    make = staticmethod(lambda k: align_ref.make_path(0.0502 + 0.002 * k + 0.05 * np.arange(4)))

    def __init__(self, g, lib):
        self.fn = lib.bsgpu_inertial_alignment
        self.fn.argtypes = capi.INERTIAL_ALIGNMENT_ARGTYPES

    def run(self, items, st, o):
        s0 = _starts([len(it["t"]) if it else 0 for it in items])
        rng = np.ascontiguousarray(np.stack([s0[:-1], s0[1:]], 1), np.int32)
        return self.fn(0, len(items), _p(st), _p(_cat(items, "tf", 1)), _p(_cat(items, "qf", 4)), _p(_cat(items, "pf", 3)), _p(rng),
                       _p(_cat(items, "t", 1)), _p(_cat(items, "w", 3)), _p(_cat(items, "a", 3)), 1, capi.ALIGN_MIN_EXCITATION, 1,
                       capi.ALIGN_SCALE_MIN, capi.ALIGN_SCALE_MAX, capi.ALIGN_RANK_TOL, _p(o["gravity"]), _p(o["bg"]), _p(o["scale"]),
                       _p(o["excitation"]), _p(o["gyro_rank"]), _p(o["velocity"]), _p(o["q_out"]), _p(o["p_out"]), _p(o["v_out"]), _p(o["status"]))


class Preintegrate(Call):
    outputs = dict(consts=(np.float64, "item", 287))
    size = staticmethod(lambda it: len(it["t"]))

    def __init__(self, g, lib):
        self.fn = lib.bsgpu_preintegrate
        self.fn.argtypes = [C.c_int, C.c_int32] + [C.c_void_p] * 11 + [C.c_double, C.c_void_p]

    @staticmethod
    def make(k):
        """10 samples at 200 Hz of the alignment cases' motion, the interval ending 2 ms after the last."""
        path = align_ref.make_path(np.array([0.047]), n_after=0)
        return dict(t=path["t"], w=path["w"] * (1.0 + 0.1 * k), a=path["a"], t_end=path["t"][-1] + 0.002, bg=[0.01 * k, -0.02, 0.015], ba=[0.1, 0.05 * k, -0.02])

    def run(self, items, st, o):
        te = np.array([it["t_end"] if it else 1.0 for it in items], float)
        bg = np.array([it["bg"] if it else [0.0, 0, 0] for it in items], float)
        ba = np.array([it["ba"] if it else [0.0, 0, 0] for it in items], float)
        covs = [np.ascontiguousarray(np.eye(3) * s) for s in (1e-4, 1e-3, 1e-8, 1e-7)]
        t, w, a = _cat(items, "t", 1), _cat(items, "w", 3), _cat(items, "a", 3)
        return self.fn(0, len(items), st.ctypes.data, t.ctypes.data, w.ctypes.data, a.ctypes.data, te.ctypes.data, bg.ctypes.data, ba.ctypes.data,
                       covs[0].ctypes.data, covs[1].ctypes.data, covs[2].ctypes.data, covs[3].ctypes.data, 1.0, o["consts"].ctypes.data)


CALLS = dict(essential=Essential, absolute_pose=AbsolutePose, relative_pose=RelativePose, localize=Localize, triangulate=Triangulate,
             alignment=Alignment, preintegrate=Preintegrate)


@pytest.fixture(scope="module")
def calls(gpu_solver_cls):
    """name -> (the call, its three items).  One context with the camera of the localisation cases (the intrinsics of the P3P and
    seven-point sets) for the calls that name a camera, another that holds a window for bsgpu_triangulate."""
    from beam_slam_amd import gpu
    cams, window = gpu_solver_cls(0), gpu_solver_cls(0)
    cams.set_cameras([frame_cases.camera()])
    made = {}
    for name, cls in CALLS.items():
        call = cls(window if name == "triangulate" else cams, gpu.lib())
        made[name] = (call, [call.make(k) for k in range(3)])
    yield made
    cams.close()
    window.close()


def _same(a, b, ka, kb, names, tag):
    for name in names:
        assert a[name][ka].tobytes() == b[name][kb].tobytes(), (tag, name, ka, kb)


@pytest.mark.parametrize("name", list(CALLS))
def test_optional_outputs(calls, name):
    """Every optional output given, none of them, and each one alone: the required outputs and whichever optional one was given hold the
    same bits in every call."""
    call, (a, b, c) = calls[name]
    for items in ([None, b, None], [a, None, c]):
        full = call(items)
        if "status" in full:
            assert all(int(full["status"][k][0]) == 0 for k, it in enumerate(items) if it)
        assert not any(v.tobytes() == b"\x5a" * v.nbytes and v.nbytes for vs in full.values() for v in vs)   # every output was written
        for want in [()] + [(o,) for o in call.optional]:
            got = call(items, want)
            assert set(got) == set(call.outputs) - set(call.optional) | set(want)
            for k in range(3):
                _same(got, full, k, k, got, (name, want))


@pytest.mark.parametrize("name", list(CALLS))
def test_empty_items(calls, name):
    """(0, m, 0) and (m, 0, m): each non-empty item holds the bits it has alone behind as many empty items (the position decides a
    RANSAC set's sampler stream); an empty item's element-wise outputs are empty."""
    call, (a, b, c) = calls[name]
    for items in ([None, b, None], [a, None, c]):
        out = call(items)
        for k, it in enumerate(items):
            if it:
                _same(out, call([None] * k + [it]), k, k, out, name)
            else:
                assert all(len(out[o][k]) == 0 for o, (_, per, _) in call.outputs.items() if per == "elem")
