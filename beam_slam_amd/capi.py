"""ctypes view of include/bsgpu.h.

The same declarations serve the product library (prefix ``bsgpu_``, loaded by
:mod:`beam_slam_amd.gpu`) and — in tests only — the CPU oracle (prefix ``bso_``), because the
oracle deliberately exports the same entry points.  Nothing in this module computes anything.
"""
import ctypes as C

import numpy as np

OK = 0
ERR_INVALID, ERR_DEVICE, ERR_UNSUPPORTED, ERR_NUMERIC = -1, -2, -3, -4

MANIFOLD_EUCLIDEAN, MANIFOLD_QUAT_RIGHT = 0, 1
LOSS_TRIVIAL, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2

F_REPROJ = 0
F_REPROJ_ONLINE_CALIB = 1
F_IMU_DELTA = 2
F_IMU_PRIOR = 3
F_RELPOSE_EXT = 4
F_RELPOSE = 5
F_ABSPOSE = 6
F_ABS_VEC3 = 7
F_REL_VEC3 = 8
F_GRAVITY = 9
F_IDP_REPROJ = 10
F_IDP_REPROJ_UNARY = 11
F_UNICYCLE = 12
F_NUM_TYPES = 13

LINEAR_AUTO, LINEAR_SCHUR_CHOLESKY, LINEAR_PCG, LINEAR_SCHUR_PCG = 0, 1, 2, 3
TR_LEVENBERG_MARQUARDT, TR_DOGLEG, TR_SUBSPACE_DOGLEG = 0, 1, 2
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2


class Options(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32),
        ("linear_solver_type", C.c_int32),
        ("jacobi_scaling", C.c_int32),
        ("max_num_consecutive_invalid_steps", C.c_int32),
        ("max_solver_time_in_seconds", C.c_double),
        ("function_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
        ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double),
        ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double),
        ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double),
        ("pcg_max_iterations", C.c_int32),
        ("trust_region_strategy_type", C.c_int32),
        ("pcg_tolerance", C.c_double),
    ]


class Summary(C.Structure):
    _fields_ = [
        ("termination_type", C.c_int32),
        ("is_solution_usable", C.c_int32),
        ("num_iterations", C.c_int32),
        ("num_successful_steps", C.c_int32),
        ("num_unsuccessful_steps", C.c_int32),
        ("num_parameters_tangent", C.c_int32),
        ("num_residuals", C.c_int32),
        ("linear_solver_used", C.c_int32),
        ("num_linear_solves", C.c_int32),
        ("num_inner_iterations", C.c_int32),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("fixed_cost", C.c_double),
        ("total_time_in_seconds", C.c_double),
        ("device_time_in_seconds", C.c_double),
        ("time_eval_seconds", C.c_double),
        ("time_assemble_seconds", C.c_double),
        ("time_linear_solve_seconds", C.c_double),
        ("message", C.c_char * 160),
    ]


class Iteration(C.Structure):
    _fields_ = [
        ("iteration", C.c_int32),
        ("step_is_valid", C.c_int32),
        ("step_is_successful", C.c_int32),
        ("reserved0", C.c_int32),
        ("cost", C.c_double),
        ("cost_change", C.c_double),
        ("gradient_max_norm", C.c_double),
        ("gradient_norm", C.c_double),
        ("step_norm", C.c_double),
        ("relative_decrease", C.c_double),
        ("trust_region_radius", C.c_double),
        ("model_cost_change", C.c_double),
    ]


class Camera(C.Structure):
    _fields_ = [
        ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
        ("R_cam_baselink", C.c_double * 9),
        ("t_cam_baselink", C.c_double * 3),
    ]


#: every symbol include/bsgpu.h declares (without prefix); tests check the library exports them all
SYMBOLS = [
    "nidx", "nconst", "nres", "options_default", "options_vio", "create", "create_error", "destroy",
    "last_error", "abi_version", "clear", "set_blocks", "set_values", "set_cameras", "add_factors", "add_factors_indirect", "sync_factors_indirect",
    "add_marginal",
    "finalize", "solve", "get_blocks", "reset_values", "num_iterations_recorded", "get_iteration",
    "evaluate", "num_residuals", "num_parameters_tangent", "tangent_offset", "covariance", "marginalize", "get_marginal",
    "reprojection_errors", "preintegrate", "triangulate", "time_reproj_jacobian_ms", "reproj_jacobian_bytes", "dense_solve", "plan_info",
    "profile_step", "time_eval_ms", "eval_bytes", "bsr_info", "covariance_joint", "update_marginal", "solve_batch", "batch_stats", "set_plan_preference",
    "covariance_requests", "localize_frames", "num_factorizations", "essential_ransac", "absolute_pose_ransac",
    "relative_pose_ransac", "inertial_alignment", "register_scans", "register_scans_error", "register_scans_gicp", "register_scans_loam", "extract_loam_features", "build_registration_maps", "backsub_tangent_table",
    "scan_context_describe", "scan_context_match", "scan_context_error",
]

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_bp = C.POINTER(C.c_uint8)

#: bsgpu_essential_ransac: per-set status values, the set-size limit and the typed prototype
RANSAC_OK, RANSAC_TOO_FEW, RANSAC_NO_MODEL = 0, 1, 2
RANSAC_MAX_MATCHES = 65536
ESSENTIAL_RANSAC_ARGTYPES = [C.c_void_p, C.c_int32, _ip, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int32, C.c_uint64, _bp, _dp, _ip, _ip,
                             _ip, _ip]
#: bsgpu_absolute_pose_ransac: the typed prototype (status values and the frame-size limit are bsgpu_essential_ransac's)
ABSOLUTE_POSE_RANSAC_ARGTYPES = [C.c_void_p, C.c_int32, _ip, _dp, _dp, _ip, C.c_double, C.c_double, C.c_int32, C.c_uint64, C.c_int32, _bp,
                                 _dp, _dp, _dp, _ip, _ip, _ip, _ip]
#: bsgpu_relative_pose_ransac: the typed prototype (status values and the set-size limit are bsgpu_essential_ransac's)
RELATIVE_POSE_RANSAC_ARGTYPES = [C.c_void_p, C.c_int32, _ip, _dp, _dp, _ip, C.c_double, C.c_double, C.c_int32, C.c_uint64, C.c_int32,
                                 C.c_double, C.c_double, _bp, _dp, _dp, _dp, _dp, _bp, _dp, _ip, _ip, _ip, _ip, _ip]
#: bsgpu_inertial_alignment: per-path status values, the reference's parameters (inertial_alignment.cpp:84, slam_initialization.cpp:313)
#: and the typed prototype
ALIGN_OK, ALIGN_TOO_FEW_FRAMES, ALIGN_BAD_IMU, ALIGN_NOT_EXCITED, ALIGN_RANK_DEFICIENT, ALIGN_SCALE_REJECTED = 0, 1, 2, 3, 4, 5
ALIGN_MIN_EXCITATION, ALIGN_SCALE_MIN, ALIGN_SCALE_MAX, ALIGN_RANK_TOL = 0.25, 0.02, 1.0, 1e-10
INERTIAL_ALIGNMENT_ARGTYPES = [C.c_int, C.c_int32, _ip, _dp, _dp, _dp, _ip, _dp, _dp, _dp, C.c_int32, C.c_double, C.c_int32, C.c_double,
                               C.c_double, C.c_double, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _dp, _dp, _ip]
#: bsgpu_register_scans: per-pair status values (the first convergence criterion that fired), the limits, the reference's shipped ICP
#: parameters (config/matchers/icp.json; rotation_threshold and rel_mse_eps: PCL's defaults, recalled) and the typed prototype
ICP_MAX_ITERATIONS, ICP_TRANSFORM, ICP_ABS_MSE, ICP_REL_MSE, ICP_TOO_FEW_CORRESPONDENCES = 1, 2, 3, 4, 5
ICP_MAX_CELLS, ICP_MAX_ITER = 1 << 22, 1000
ICP_DEFAULTS = dict(max_corr=1.0, max_iter=50, t_eps=1e-8, fit_eps=1e-2, rotation_threshold=0.99999, rel_mse_eps=1e-5)
REGISTER_SCANS_ARGTYPES = [C.c_int, C.c_int32, _ip, _dp, _ip, _dp, _dp, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double,
                           C.c_double, _dp, _dp, _dp, _ip, _ip, _ip]
#: bsgpu_register_scans_gicp: per-pair status values, the limits, the parameters (k_neighbors, max_iter, r_eps: the reference's
#: config/matchers/gicp.json; gicp_epsilon, max_corr, t_eps, max_inner: PCL's GICP constructor, recalled; inner_eps, grid_cell: this
#: library's own, grid_cell a performance knob that no result depends on) and the typed prototype
GICP_MAX_ITERATIONS, GICP_TRANSFORM, GICP_TOO_FEW_CORRESPONDENCES, GICP_DEGENERATE = 1, 2, 5, 6
GICP_MAX_K, GICP_MAX_INNER = 32, 64
GICP_DEFAULTS = dict(k_neighbors=10, gicp_epsilon=1e-3, max_corr=5.0, max_iter=100, r_eps=1e-8, t_eps=5e-4, max_inner=20, inner_eps=1e-10,
                     grid_cell=0.5)
REGISTER_SCANS_GICP_ARGTYPES = [C.c_int, C.c_int32, _ip, _dp, _ip, _dp, _dp, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double,
                                C.c_double, C.c_int32, C.c_double, C.c_double, _dp, _dp, _dp, _ip, _ip, _ip, _ip, _dp, _dp]
#: bsgpu_register_scans_loam: per-pair status values, the limits, the reference's shipped parameters (config/matchers/loam_vlp16.json:
#: max_correspondence_distance, min_number_measurements, max_correspondence_iterations, the two convergence criteria;
#: config/optimization/ceres_config.json: HUBER with scaling 1, and under "inner" the solver options it sets over Ceres' defaults;
#: grid_cell: this library's own, a performance knob that no result depends on) and the typed prototype
LOAM_MAX_ITERATIONS, LOAM_TRANSFORM, LOAM_TOO_FEW_MEASUREMENTS, LOAM_SOLVER_FAILED = 1, 2, 5, 6
LOAM_MAX_OUTER, LOAM_MAX_INNER, LOAM_MAX_FEATURES = 100, 1000, 65536
LOSS_TRIVIAL, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2
LOAM_DEFAULTS = dict(max_corr=0.5, min_measurements=30, max_outer=10, conv_translation_m=1e-3, conv_rotation_deg=0.1, loss_kind=LOSS_HUBER,
                     loss_a=1.0, grid_cell=0.5,
                     inner=dict(max_num_iterations=50, function_tolerance=1e-8, gradient_tolerance=1e-10, parameter_tolerance=1e-8))
REGISTER_SCANS_LOAM_ARGTYPES = [C.c_int, C.c_int32, _ip, _dp, _ip, _dp, _ip, _dp, _ip, _dp, _dp, C.c_double, C.c_int32, C.c_int32, C.c_double,
                                C.c_double, C.POINTER(Options), C.c_int32, C.c_double, C.c_double, _dp, _dp, _dp, _dp, _ip, _ip, _ip, _ip, _ip]
#: bsgpu_extract_loam_features: the labels, the axes, the limits, the reference's shipped parameters (config/matchers/loam_vlp16.json;
#: loam_vlp16_init.json: 3 regions, curvature_region 3, 15 less sharp) and the typed prototype
LOAM_DROPPED, LOAM_LESS_FLAT, LOAM_FLAT, LOAM_LESS_SHARP, LOAM_SHARP = -1, 0, 1, 2, 3
AXIS_X, AXIS_Y, AXIS_Z = 0, 1, 2
LOAM_MAX_RINGS, LOAM_MAX_RING_POINTS, LOAM_MAX_CURVATURE_REGION, LOAM_MAX_REGIONS = 128, 4096, 16, 64
LOAM_FEATURE_DEFAULTS = dict(number_of_beams=16, fov_deg=30.0, vertical_axis=AXIS_Z, n_feature_regions=6, curvature_region=5, max_corner_sharp=2,
                             max_corner_less_sharp=20, max_surface_flat=4, surface_curvature_threshold=0.1, downsample_less_flat_features=0)
EXTRACT_LOAM_FEATURES_ARGTYPES = [C.c_int, C.c_int32, _ip, _dp, _ip, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_double, C.c_int32, _ip, _ip, _dp, _ip, _ip, _dp, _ip, _ip, _dp, _ip, _ip, _dp, _ip, _dp]
#: bsgpu_build_registration_maps: the cap, the device sort's tile (tests follow it), the merge-only sentinel, the cell range and the
#: typed prototype
MAP_MAX_POINTS, MAP_SORT_TILE, MAP_MERGE_ONLY, MAP_CELL_RANGE = 8388608, 1024, -1.0, 1048576
BUILD_REGISTRATION_MAPS_ARGTYPES = [C.c_int, C.c_int32, _ip, _ip, _dp, _dp, C.c_double, _ip, _dp, _ip]
#: bsgpu_scan_context_describe / bsgpu_scan_context_match: the descriptor's shape, the limits, the reference's shipped parameters
#: (SCManager's LIDAR_HEIGHT, PC_MAX_RADIUS, NUM_CANDIDATES_FROM_TREE, SEARCH_RATIO, SC_DIST_THRES, recalled) and the typed prototypes
SC_RINGS, SC_SECTORS, SC_MAX_CANDIDATES, SC_MAX_TREE_CANDIDATES, SC_MAX_SCAN_POINTS = 20, 60, 65536, 64, 65535 * 4096
SC_DEFAULTS = dict(lidar_height=2.0, max_radius=80.0, n_tree_candidates=10, search_ratio=0.1, dist_thres=0.3)
SCAN_CONTEXT_DESCRIBE_ARGTYPES = [C.c_int, C.c_int32, _ip, _dp, C.c_int32, _ip, _ip, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _ip]
SCAN_CONTEXT_MATCH_ARGTYPES = [C.c_int, C.c_int32, _ip, _dp, _ip, _dp, C.c_int32, C.c_double, C.c_double, _ip, _dp, _ip, _dp, _dp, _ip]


def _ptr(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


class SolverError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class Solver:
    """Thin handle over one context of a library exporting the bsgpu.h entry points."""

    def __init__(self, lib, prefix, device=0):
        self._lib, self._p = lib, prefix
        f = self._f
        f("create").restype = C.c_void_p
        f("create").argtypes = [C.c_int]
        f("destroy").argtypes = [C.c_void_p]
        f("last_error").restype = C.c_char_p
        f("last_error").argtypes = [C.c_void_p]
        f("set_blocks").argtypes = [C.c_void_p, C.c_int32, _dp, _ip, _bp, _bp, _bp]
        f("set_values").argtypes = [C.c_void_p, _dp, C.c_int64]
        f("set_cameras").argtypes = [C.c_void_p, C.c_int32, C.POINTER(Camera)]
        f("add_factors").argtypes = [C.c_void_p, C.c_int32, C.c_int32, _ip, _dp, _ip, _dp]
        f("add_marginal").argtypes = [C.c_void_p, C.c_int32, _ip, C.c_int32, _dp, _dp, _dp]
        f("marginalize").argtypes = [C.c_void_p, C.c_int32, _ip, _ip, _ip, _ip]
        f("get_marginal").argtypes = [C.c_void_p, _ip, _dp, _dp, _dp]
        f("finalize").argtypes = [C.c_void_p]
        f("clear").argtypes = [C.c_void_p]
        f("solve").argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(Summary)]
        f("get_blocks").argtypes = [C.c_void_p, _dp, C.c_int64]
        f("reset_values").argtypes = [C.c_void_p]
        f("num_iterations_recorded").argtypes = [C.c_void_p]
        f("get_iteration").argtypes = [C.c_void_p, C.c_int32, C.POINTER(Iteration)]
        f("evaluate").argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
        f("num_residuals").argtypes = [C.c_void_p]
        f("num_parameters_tangent").argtypes = [C.c_void_p]
        f("tangent_offset").argtypes = [C.c_void_p, C.c_int32]
        f("covariance").argtypes = [C.c_void_p, C.c_int32, C.c_int32, _dp]
        f("options_default").argtypes = [C.POINTER(Options)]
        f("options_vio").argtypes = [C.POINTER(Options)]
        self._ctx = f("create")(device)
        if not self._ctx:
            why = ""
            try:
                ce = f("create_error")
                ce.restype = C.c_char_p
                why = ce().decode()
            except AttributeError:
                pass
            raise SolverError(ERR_DEVICE, f"{prefix}create({device}) failed: {why}")
        self._nvalues = 0

    def _f(self, name):
        return getattr(self._lib, self._p + name)

    def has(self, name):
        """Whether the library behind this handle exports the entry point (the test oracle has only what its tests need)."""
        return hasattr(self._lib, self._p + name)

    def _chk(self, rc):
        if rc != OK:
            raise SolverError(rc, self._f("last_error")(self._ctx).decode())

    def close(self):
        if getattr(self, "_ctx", None):
            self._f("destroy")(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- options ---------------------------------------------------------------------------
    def options_default(self):
        o = Options()
        self._f("options_default")(C.byref(o))
        return o

    def options_vio(self):
        o = Options()
        self._f("options_vio")(C.byref(o))
        return o

    # -- problem ---------------------------------------------------------------------------
    def clear(self):
        self._chk(self._f("clear")(self._ctx))

    def set_blocks(self, values, offset, size, manifold, is_const):
        values = np.ascontiguousarray(values, np.float64)
        offset = np.ascontiguousarray(offset, np.int32)
        size = np.ascontiguousarray(size, np.uint8)
        manifold = np.ascontiguousarray(manifold, np.uint8)
        is_const = np.ascontiguousarray(is_const, np.uint8)
        self._nvalues = values.size
        self._chk(self._f("set_blocks")(self._ctx, offset.size, _ptr(values, _dp), _ptr(offset, _ip),
                                        _ptr(size, _bp), _ptr(manifold, _bp), _ptr(is_const, _bp)))

    def set_values(self, values):
        values = np.ascontiguousarray(values, np.float64)
        self._chk(self._f("set_values")(self._ctx, _ptr(values, _dp), values.size))

    def set_cameras(self, cams):
        arr = (Camera * len(cams))(*cams)
        self._chk(self._f("set_cameras")(self._ctx, len(cams), arr))

    def add_factors(self, ftype, block_idx, consts, loss_kind=None, loss_a=None):
        block_idx = np.ascontiguousarray(block_idx, np.int32)
        consts = np.ascontiguousarray(consts, np.float64)
        n = block_idx.shape[0] if block_idx.ndim == 2 else 0
        if loss_kind is not None:
            loss_kind = np.ascontiguousarray(np.broadcast_to(loss_kind, (n,)), np.int32)
        if loss_a is not None:
            loss_a = np.ascontiguousarray(np.broadcast_to(loss_a, (n,)), np.float64)
        self._chk(self._f("add_factors")(self._ctx, ftype, n, _ptr(block_idx, _ip), _ptr(consts, _dp),
                                         _ptr(loss_kind, _ip), _ptr(loss_a, _dp)))

    def add_factors_indirect(self, ftype, slot_idx, slot_to_block, consts, loss_kind=None, loss_a=None):
        """add_factors for a caller that keeps its tables across solves: the block columns of slot_idx hold caller-side variable
        slots, translated through slot_to_block on the way in (camera columns are not translated)."""
        slot_idx = np.ascontiguousarray(slot_idx, np.int32)
        slot_to_block = np.ascontiguousarray(slot_to_block, np.int32)
        consts = np.ascontiguousarray(consts, np.float64)
        n = slot_idx.shape[0] if slot_idx.ndim == 2 else 0
        if loss_kind is not None:
            loss_kind = np.ascontiguousarray(np.broadcast_to(loss_kind, (n,)), np.int32)
        if loss_a is not None:
            loss_a = np.ascontiguousarray(np.broadcast_to(loss_a, (n,)), np.float64)
        fn = self._f("add_factors_indirect")
        fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _ip, C.c_int32, _ip, _dp, _ip, _dp]
        fn.restype = C.c_int
        self._chk(fn(self._ctx, ftype, n, _ptr(slot_idx, _ip), slot_to_block.size, _ptr(slot_to_block, _ip), _ptr(consts, _dp),
                     _ptr(loss_kind, _ip), _ptr(loss_a, _dp)))

    def sync_factors_indirect(self, ftype, slot_idx, slot_to_block, consts, loss_kind=None, loss_a=None, changed_rows=None):
        """add_factors_indirect for a type's WHOLE table plus the rows that differ from the table of the previous call for the type
        (None: no promise, the table is read whole).  The back-end keeps slot-named host / device copies of the reprojection table
        across clear() and patches them (include/bsgpu.h)."""
        slot_idx = np.ascontiguousarray(slot_idx, np.int32)
        slot_to_block = np.ascontiguousarray(slot_to_block, np.int32)
        consts = np.ascontiguousarray(consts, np.float64)
        n = slot_idx.shape[0] if slot_idx.ndim == 2 else 0
        if loss_kind is not None:
            loss_kind = np.ascontiguousarray(np.broadcast_to(loss_kind, (n,)), np.int32)
        if loss_a is not None:
            loss_a = np.ascontiguousarray(np.broadcast_to(loss_a, (n,)), np.float64)
        if changed_rows is not None:
            changed_rows = np.ascontiguousarray(changed_rows, np.int32)
        fn = self._f("sync_factors_indirect")
        fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _ip, C.c_int32, _ip, _dp, _ip, _dp, C.c_int32, _ip]
        fn.restype = C.c_int
        self._chk(fn(self._ctx, ftype, n, _ptr(slot_idx, _ip), slot_to_block.size, _ptr(slot_to_block, _ip), _ptr(consts, _dp),
                     _ptr(loss_kind, _ip), _ptr(loss_a, _dp), -1 if changed_rows is None else changed_rows.size,
                     _ptr(changed_rows, _ip) if changed_rows is not None and changed_rows.size else None))

    def add_marginal(self, blocks, A, b, xbar):
        """fuse_constraints::MarginalConstraint: r = b + sum_i A_i (x_i [-] xbar_i)."""
        blocks = np.ascontiguousarray(blocks, np.int32)
        A = np.ascontiguousarray(np.atleast_2d(A), np.float64)
        b = np.ascontiguousarray(b, np.float64)
        xbar = np.ascontiguousarray(xbar, np.float64)
        assert A.shape[0] == b.size
        self._chk(self._f("add_marginal")(self._ctx, blocks.size, _ptr(blocks, _ip), A.shape[0], _ptr(A, _dp), _ptr(b, _dp),
                                          _ptr(xbar, _dp)))

    def update_marginal(self, index, A, b, xbar):
        """Replaces the payload of the index-th dense prior in place (bsgpu_update_marginal): no re-finalize."""
        A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64); xbar = np.ascontiguousarray(xbar, np.float64)
        fn = self._f("update_marginal")
        assert A.ndim == 2 and b.size == A.shape[0]
        fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]
        self._chk(fn(self._ctx, int(index), A.shape[0], A.shape[1], xbar.size, A.ctypes.data_as(_dp), b.ctypes.data_as(_dp), xbar.ctypes.data_as(_dp)))

    def covariance_joint(self, blocks, tangent_sizes):
        """Joint marginal covariance (D x D, D = sum of tangent sizes <= 64) of several pose-side blocks (bsgpu_covariance_joint)."""
        bl = np.ascontiguousarray(blocks, np.int32)
        D = int(np.sum(tangent_sizes))
        out = np.zeros((D, D))
        fn = self._f("covariance_joint")
        fn.argtypes = [C.c_void_p, C.c_int32, _ip, _dp]
        self._chk(fn(self._ctx, int(bl.size), bl.ctypes.data_as(_ip), out.ctypes.data_as(_dp)))
        return out

    def covariance_requests(self, pairs):
        """Graph::getCovariance(requests, matrices) (bsgpu_covariance_requests): the ts(a) x ts(b) marginal covariance of every
        (block_a, block_b) pair, any non-constant block (landmarks included), from one linearisation.  Returns a list of arrays."""
        pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        n = pr.shape[0]
        fn = self._f("covariance_requests")
        fn.argtypes = [C.c_void_p, C.c_int32, _ip, C.POINTER(C.c_int64), _dp]
        if n == 0:
            self._chk(fn(self._ctx, 0, None, None, None))
            return []
        # sizes only (no device work): the tangent size of each distinct block from its (b, b) entry, then the offsets of the pairs
        blocks = np.unique(pr)
        diag = np.ascontiguousarray(np.repeat(blocks, 2).astype(np.int32))
        off_d = np.zeros(blocks.size + 1, np.int64)
        self._chk(fn(self._ctx, blocks.size, diag.ctypes.data_as(_ip), off_d.ctypes.data_as(C.POINTER(C.c_int64)), None))
        ts = {int(b): int(round(np.sqrt(off_d[i + 1] - off_d[i]))) for i, b in enumerate(blocks)}
        off = np.zeros(n + 1, np.int64)
        self._chk(fn(self._ctx, n, pr.ctypes.data_as(_ip), off.ctypes.data_as(C.POINTER(C.c_int64)), None))
        out = np.zeros(int(off[-1]))
        self._chk(fn(self._ctx, n, pr.ctypes.data_as(_ip), None, out.ctypes.data_as(_dp)))
        return [out[off[i]:off[i + 1]].reshape(ts[int(a)], ts[int(b)]) for i, (a, b) in enumerate(pr)]

    def localize_frames(self, obs_start, pixels, q_init, p_init, camera, points=None, lm_block=None, loss_kind=LOSS_TRIVIAL, loss_a=1.0,
                        sqrt_info=1.0, truncate_pixels=False, min_points=20, image_width=0, image_height=0, options=None):
        """VisualOdometry::LocalizeFrame for a batch of frames (bsgpu_localize_frames): frame f holds observations
        [obs_start[f], obs_start[f+1]) with pixels (n x 2) and either world points (n x 3) or landmark blocks (n) of this context.
        Returns a dict of arrays: q (F x 4), p (F x 3), cov (F x 6 x 6, [p, q tangent]), avg_reproj, final_cost, iterations, status."""
        os_ = np.ascontiguousarray(obs_start, np.int32)
        F = os_.size - 1
        pix = np.ascontiguousarray(pixels, np.float64).reshape(-1, 2)
        pts = None if points is None else np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        lmb = None if lm_block is None else np.ascontiguousarray(lm_block, np.int32)
        cam = np.ascontiguousarray(np.broadcast_to(np.asarray(camera, np.int32), (F,)))
        qi = np.ascontiguousarray(q_init, np.float64).reshape(F, 4)
        pi = np.ascontiguousarray(p_init, np.float64).reshape(F, 3)
        o = options if options is not None else self.options_default()
        out = dict(q=np.zeros((F, 4)), p=np.zeros((F, 3)), cov=np.zeros((F, 6, 6)), avg_reproj=np.zeros(F), final_cost=np.zeros(F),
                   iterations=np.zeros(F, np.int32), status=np.zeros(F, np.int32))
        fn = self._f("localize_frames")
        fn.argtypes = [C.c_void_p, C.c_int32, _ip, _dp, _dp, _ip, _ip, _dp, _dp, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32,
                       C.c_int32, C.c_int32, C.POINTER(Options), _dp, _dp, _dp, _dp, _dp, _ip, _ip]
        self._chk(fn(self._ctx, F, _ptr(os_, _ip), _ptr(pix, _dp), _ptr(pts, _dp), _ptr(lmb, _ip), _ptr(cam, _ip), _ptr(qi, _dp), _ptr(pi, _dp),
                     int(loss_kind), float(loss_a), float(sqrt_info), 1 if truncate_pixels else 0, int(min_points), int(image_width),
                     int(image_height), C.byref(o), _ptr(out["q"], _dp), _ptr(out["p"], _dp), _ptr(out["cov"], _dp),
                     _ptr(out["avg_reproj"], _dp), _ptr(out["final_cost"], _dp), _ptr(out["iterations"], _ip), _ptr(out["status"], _ip)))
        return out

    def marginalize(self, blocks, sizes):
        """fuse_constraints::marginalizeVariables at the current values: returns (kept_blocks, A, b, xbar), the payload
        of the MarginalConstraint that replaces every factor touching `blocks`.  `sizes` = ambient block sizes."""
        blocks = np.ascontiguousarray(blocks, np.int32)
        nk, nr, nc = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._chk(self._f("marginalize")(self._ctx, blocks.size, _ptr(blocks, _ip), C.byref(nk), C.byref(nr), C.byref(nc)))
        kept = np.zeros(nk.value, np.int32)
        self._chk(self._f("get_marginal")(self._ctx, _ptr(kept, _ip), None, None, None))
        A = np.zeros((nr.value, nc.value)); b = np.zeros(nr.value)
        xbar = np.zeros(int(sum(sizes[k] for k in kept)))
        self._chk(self._f("get_marginal")(self._ctx, _ptr(kept, _ip), _ptr(A, _dp), _ptr(b, _dp), _ptr(xbar, _dp)))
        return kept, A, b, xbar

    def finalize(self):
        self._chk(self._f("finalize")(self._ctx))

    # -- solve -----------------------------------------------------------------------------
    def solve(self, options=None):
        o = options if options is not None else self.options_default()
        s = Summary()
        self._chk(self._f("solve")(self._ctx, C.byref(o), C.byref(s)))
        return s

    @staticmethod
    def solve_batch(solvers, options=None):
        """bsgpu_solve_batch: the solvers' windows at once (landmark windows advance together, one set of launches per LM iteration;
        any other window on a library thread of its own); returns their summaries."""
        n = len(solvers)
        first = solvers[0]
        opts = options if isinstance(options, (list, tuple)) else [options if options is not None else first.options_default()]
        oa = (Options * len(opts))(*opts)
        sa = (Summary * n)()
        ca = (C.c_void_p * n)(*[sv._ctx for sv in solvers])
        fn = first._f("solve_batch")
        fn.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(Options), C.c_int32, C.POINTER(Summary)]
        rc = fn(ca, n, oa, 1 if len(opts) > 1 else 0, sa)
        if rc != OK:
            for sv in solvers:
                msg = sv._f("last_error")(sv._ctx).decode()
                if msg:
                    raise SolverError(rc, msg)
            raise SolverError(rc, "solve_batch failed")
        return list(sa)

    def get_blocks(self):
        out = np.empty(self._nvalues, np.float64)
        self._chk(self._f("get_blocks")(self._ctx, _ptr(out, _dp), out.size))
        return out

    def reset_values(self):
        self._chk(self._f("reset_values")(self._ctx))

    def num_factorizations(self):
        """Linear systems the last solve assembled and solved (bsgpu_num_factorizations): every Gauss-Newton / LM attempt, DOGLEG's mu
        retries included; a DOGLEG step that reuses its Gauss-Newton step after a rejection does not count."""
        fn = self._f("num_factorizations")
        fn.argtypes = [C.c_void_p]
        fn.restype = C.c_int
        return fn(self._ctx)

    def iterations(self):
        n = self._f("num_iterations_recorded")(self._ctx)
        out = []
        for i in range(n):
            it = Iteration()
            self._chk(self._f("get_iteration")(self._ctx, i, C.byref(it)))
            out.append(it)
        return out

    # -- evaluate --------------------------------------------------------------------------
    def num_residuals(self):
        return self._f("num_residuals")(self._ctx)

    def num_parameters_tangent(self):
        return self._f("num_parameters_tangent")(self._ctx)

    def tangent_offset(self, block):
        return self._f("tangent_offset")(self._ctx, block)

    def evaluate(self, residuals=True, gradient=True, jacobian=False):
        self.finalize()
        m, n = self.num_residuals(), self.num_parameters_tangent()
        cost = C.c_double(0.0)
        r = np.zeros(m) if residuals else None
        g = np.zeros(n) if gradient else None
        J = np.zeros((m, n)) if jacobian else None
        self._chk(self._f("evaluate")(self._ctx, C.byref(cost), _ptr(r, _dp), _ptr(g, _dp), _ptr(J, _dp)))
        return cost.value, r, g, J

    def covariance(self, block_a, block_b, ta=3, tb=3):
        out = np.zeros((ta, tb))
        self._chk(self._f("covariance")(self._ctx, block_a, block_b, _ptr(out, _dp)))
        return out
