"""Loader of the product library libbsgpu.so (HIP kernels + C-ABI of include/bsgpu.h).

There is deliberately no fallback: if the library has not been built (``__graft_entry__.build()`` or
``make -C beam_slam_amd/csrc``) or no HIP device is usable, this module raises.
"""
import ctypes
import os

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libbsgpu.so")
_LIB = None


class GpuLibraryMissing(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GpuLibraryMissing(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  beam_slam_amd has no CPU fallback.")
        _LIB = ctypes.CDLL(LIB_PATH)
        _LIB.bsgpu_time_reproj_jacobian_ms.restype = ctypes.c_double
        _LIB.bsgpu_time_reproj_jacobian_ms.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        _LIB.bsgpu_time_eval_ms.restype = ctypes.c_double
        _LIB.bsgpu_time_eval_ms.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        _LIB.bsgpu_eval_bytes.restype = ctypes.c_int64
        _LIB.bsgpu_eval_bytes.argtypes = [ctypes.c_void_p]
        _LIB.bsgpu_reproj_jacobian_bytes.restype = ctypes.c_int64
        _LIB.bsgpu_reproj_jacobian_bytes.argtypes = [ctypes.c_void_p]
        _LIB.bsgpu_dense_solve.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int32, ctypes.POINTER(ctypes.c_double)]
    return _LIB


def dense_solve(A, b, device=0, max_chains=4):
    """A x = b (SPD) through the reduced-camera-system kernels; returns (x, milliseconds)."""
    import numpy as np
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    x = np.empty_like(b)
    ms = ctypes.c_double(0.0)
    rc = lib().bsgpu_dense_solve(device, A.shape[0], A.ctypes.data, b.ctypes.data, x.ctypes.data, int(max_chains),
                                 ctypes.byref(ms))
    if rc != 0:
        raise capi.SolverError(rc, "bsgpu_dense_solve failed")
    return x, ms.value


def preintegrate(sample_start, t, w, a, t_end, bg, ba, cov_w, cov_a, cov_bg, cov_ba, info_weight=1.0, device=0):
    """bs_common::PreIntegrator::Integrate for a batch of intervals on the device -> (n, 287) BSGPU_F_IMU_DELTA consts."""
    import numpy as np
    f64 = lambda x: np.ascontiguousarray(x, np.float64)
    ss = np.ascontiguousarray(sample_start, np.int32)
    n = ss.size - 1
    t, w, a, t_end, bg, ba = f64(t), f64(w), f64(a), f64(t_end), f64(bg), f64(ba)
    covs = [f64(np.asarray(c, float) * (np.eye(3) if np.ndim(c) == 0 else 1.0)) for c in (cov_w, cov_a, cov_bg, cov_ba)]
    out = np.empty((n, 287))
    fn = lib().bsgpu_preintegrate
    fn.argtypes = [ctypes.c_int, ctypes.c_int32] + [ctypes.c_void_p] * 11 + [ctypes.c_double, ctypes.c_void_p]
    rc = fn(device, n, ss.ctypes.data, t.ctypes.data, w.ctypes.data, a.ctypes.data, t_end.ctypes.data, bg.ctypes.data, ba.ctypes.data,
            covs[0].ctypes.data, covs[1].ctypes.data, covs[2].ctypes.data, covs[3].ctypes.data, float(info_weight), out.ctypes.data)
    if rc != 0:
        raise capi.SolverError(rc, "bsgpu_preintegrate failed")
    return out


def inertial_alignment(frame_start, t_frame, q_frame, p_frame, imu_range, t, w, a, bridge_gap=False,
                       min_excitation=capi.ALIGN_MIN_EXCITATION, apply_scale=True, scale_min=capi.ALIGN_SCALE_MIN,
                       scale_max=capi.ALIGN_SCALE_MAX, rank_tol=capi.ALIGN_RANK_TOL, device=0):
    """bsgpu_inertial_alignment: imu::EstimateParameters, the scale gate and AlignPathAndVelocities for a batch of candidate paths.
    Path k holds frames [frame_start[k], frame_start[k+1]) (stamp, T_WORLD_BASELINK as wxyz / xyz) and the IMU samples
    [imu_range[k, 0], imu_range[k, 1]) of t / w / a.  Returns a dict of arrays: gravity (P x 3), bg (P x 3), scale, excitation,
    gyro_rank, status (P); velocity, p_out, v_out (F x 3), q_out (F x 4)."""
    import numpy as np
    f64 = lambda x, shape: np.ascontiguousarray(x, np.float64).reshape(shape)
    fs = np.ascontiguousarray(frame_start, np.int32).reshape(-1)
    P = fs.size - 1
    ir = np.ascontiguousarray(imu_range, np.int32).reshape(-1, 2)
    tf, qf, pf = f64(t_frame, (-1,)), f64(q_frame, (-1, 4)), f64(p_frame, (-1, 3))
    t, w, a = f64(t, (-1,)), f64(w, (-1, 3)), f64(a, (-1, 3))
    F = tf.size
    if P < 0 or ir.shape[0] != P or qf.shape[0] != F or pf.shape[0] != F or w.shape[0] != t.size or a.shape[0] != t.size:
        raise capi.SolverError(capi.ERR_INVALID, "inertial_alignment: array sizes do not agree")
    if P > 0 and (int(fs.max()) > F or int(ir.max()) > t.size):
        raise capi.SolverError(capi.ERR_INVALID, "inertial_alignment: frame_start / imu_range name more frames or samples than were passed")
    out = dict(gravity=np.zeros((P, 3)), bg=np.zeros((P, 3)), scale=np.zeros(P), excitation=np.zeros(P), gyro_rank=np.zeros(P, np.int32),
               velocity=np.zeros((F, 3)), q_out=np.zeros((F, 4)), p_out=np.zeros((F, 3)), v_out=np.zeros((F, 3)), status=np.zeros(P, np.int32))
    fn = lib().bsgpu_inertial_alignment
    fn.argtypes = capi.INERTIAL_ALIGNMENT_ARGTYPES
    _dp, _ip = capi._dp, capi._ip
    d = lambda x: x.ctypes.data_as(_dp)
    rc = fn(device, P, fs.ctypes.data_as(_ip), d(tf), d(qf), d(pf), ir.ctypes.data_as(_ip), d(t), d(w), d(a), int(bool(bridge_gap)),
            float(min_excitation), int(bool(apply_scale)), float(scale_min), float(scale_max), float(rank_tol), d(out["gravity"]),
            d(out["bg"]), d(out["scale"]), d(out["excitation"]), out["gyro_rank"].ctypes.data_as(_ip), d(out["velocity"]), d(out["q_out"]),
            d(out["p_out"]), d(out["v_out"]), out["status"].ctypes.data_as(_ip))
    if rc != 0:
        raise capi.SolverError(rc, "bsgpu_inertial_alignment failed")
    return out


def register_scans(ref_start, ref_points, tgt_start, tgt_points, T_init=None, max_corr=capi.ICP_DEFAULTS["max_corr"],
                   max_iter=capi.ICP_DEFAULTS["max_iter"], t_eps=capi.ICP_DEFAULTS["t_eps"], fit_eps=capi.ICP_DEFAULTS["fit_eps"],
                   rotation_threshold=capi.ICP_DEFAULTS["rotation_threshold"], rel_mse_eps=capi.ICP_DEFAULTS["rel_mse_eps"], device=0):
    """bsgpu_register_scans: point-to-point ICP (the reference's matcher in its shipped ICP configuration) for a batch of scan pairs.
    Pair p registers the reference cloud ref_points[ref_start[p]:ref_start[p+1]] onto the target cloud
    tgt_points[tgt_start[p]:tgt_start[p+1]] (moved by T_init[p], 3 x 4, first when given).  Returns a dict of arrays: T_refest_ref and
    T_ref_tgt (P x 3 x 4), mse, n_corr, n_iters, status (P)."""
    import numpy as np
    rs = np.ascontiguousarray(ref_start, np.int32).reshape(-1)
    ts = np.ascontiguousarray(tgt_start, np.int32).reshape(-1)
    rp = np.ascontiguousarray(ref_points, np.float64).reshape(-1, 3)
    tp = np.ascontiguousarray(tgt_points, np.float64).reshape(-1, 3)
    P = rs.size - 1
    ti = None if T_init is None else np.ascontiguousarray(T_init, np.float64).reshape(-1, 3, 4)
    if P < 0 or ts.size != P + 1 or (ti is not None and ti.shape[0] != P):
        raise capi.SolverError(capi.ERR_INVALID, "register_scans: array sizes do not agree")
    if int(rs.max()) > rp.shape[0] or int(ts.max()) > tp.shape[0]:
        raise capi.SolverError(capi.ERR_INVALID, "register_scans: ref_start / tgt_start name more points than were passed")
    out = dict(T_refest_ref=np.zeros((P, 3, 4)), T_ref_tgt=np.zeros((P, 3, 4)), mse=np.zeros(P), n_corr=np.zeros(P, np.int32),
               n_iters=np.zeros(P, np.int32), status=np.zeros(P, np.int32))
    fn = lib().bsgpu_register_scans
    fn.argtypes = capi.REGISTER_SCANS_ARGTYPES
    _dp, _ip = capi._dp, capi._ip
    d = lambda x: None if x is None else x.ctypes.data_as(_dp)
    i = lambda x: x.ctypes.data_as(_ip)
    rc = fn(device, P, i(rs), d(rp), i(ts), d(tp), d(ti), float(max_corr), int(max_iter), float(t_eps), float(fit_eps),
            float(rotation_threshold), float(rel_mse_eps), d(out["T_refest_ref"]), d(out["T_ref_tgt"]), d(out["mse"]), i(out["n_corr"]),
            i(out["n_iters"]), i(out["status"]))
    if rc != 0:
        raise capi.SolverError(rc, register_scans_error())
    return out


def register_scans_gicp(ref_start, ref_points, tgt_start, tgt_points, T_init=None, k_neighbors=capi.GICP_DEFAULTS["k_neighbors"],
                        gicp_epsilon=capi.GICP_DEFAULTS["gicp_epsilon"], max_corr=capi.GICP_DEFAULTS["max_corr"],
                        max_iter=capi.GICP_DEFAULTS["max_iter"], r_eps=capi.GICP_DEFAULTS["r_eps"], t_eps=capi.GICP_DEFAULTS["t_eps"],
                        max_inner=capi.GICP_DEFAULTS["max_inner"], inner_eps=capi.GICP_DEFAULTS["inner_eps"],
                        grid_cell=capi.GICP_DEFAULTS["grid_cell"], covariances=True, device=0):
    """bsgpu_register_scans_gicp: Generalized ICP (the reference's matcher in its shipped GICP configuration) for a batch of scan pairs,
    clouds and roles as in register_scans.  Returns a dict of arrays: T_refest_ref and T_ref_tgt (P x 3 x 4), cost, n_corr, n_iters,
    n_inner, status (P) and, unless covariances is false, ref_cov and tgt_cov (6 per point: xx, xy, xz, yy, yz, zz)."""
    import numpy as np
    rs = np.ascontiguousarray(ref_start, np.int32).reshape(-1)
    ts = np.ascontiguousarray(tgt_start, np.int32).reshape(-1)
    rp = np.ascontiguousarray(ref_points, np.float64).reshape(-1, 3)
    tp = np.ascontiguousarray(tgt_points, np.float64).reshape(-1, 3)
    P = rs.size - 1
    ti = None if T_init is None else np.ascontiguousarray(T_init, np.float64).reshape(-1, 3, 4)
    if P < 0 or ts.size != P + 1 or (ti is not None and ti.shape[0] != P):
        raise capi.SolverError(capi.ERR_INVALID, "register_scans_gicp: array sizes do not agree")
    if int(rs.max()) > rp.shape[0] or int(ts.max()) > tp.shape[0]:
        raise capi.SolverError(capi.ERR_INVALID, "register_scans_gicp: ref_start / tgt_start name more points than were passed")
    out = dict(T_refest_ref=np.zeros((P, 3, 4)), T_ref_tgt=np.zeros((P, 3, 4)), cost=np.zeros(P), n_corr=np.zeros(P, np.int32),
               n_iters=np.zeros(P, np.int32), n_inner=np.zeros(P, np.int32), status=np.zeros(P, np.int32))
    if covariances:
        out.update(ref_cov=np.zeros((max(int(rs[-1]), 0), 6)), tgt_cov=np.zeros((max(int(ts[-1]), 0), 6)))
    fn = lib().bsgpu_register_scans_gicp
    fn.argtypes = capi.REGISTER_SCANS_GICP_ARGTYPES
    _dp, _ip = capi._dp, capi._ip
    d = lambda x: None if x is None else x.ctypes.data_as(_dp)
    i = lambda x: x.ctypes.data_as(_ip)
    rc = fn(device, P, i(rs), d(rp), i(ts), d(tp), d(ti), int(k_neighbors), float(gicp_epsilon), float(max_corr), int(max_iter), float(r_eps),
            float(t_eps), int(max_inner), float(inner_eps), float(grid_cell), d(out["T_refest_ref"]), d(out["T_ref_tgt"]), d(out["cost"]),
            i(out["n_corr"]), i(out["n_iters"]), i(out["n_inner"]), i(out["status"]), d(out.get("ref_cov")), d(out.get("tgt_cov")))
    if rc != 0:
        raise capi.SolverError(rc, register_scans_error())
    return out


def loam_options(inner=None):
    """The inner solve's options: Ceres' defaults (bsgpu_options_default) under the fields of capi.LOAM_DEFAULTS["inner"], then under
    `inner` (a dict of fields; a capi.Options is taken as it is)."""
    if isinstance(inner, capi.Options):
        return inner
    o = capi.Options()
    fn = lib().bsgpu_options_default
    fn.argtypes = [ctypes.POINTER(capi.Options)]
    fn.restype = None
    fn(ctypes.byref(o))
    for k, v in dict(capi.LOAM_DEFAULTS["inner"], **(inner or {})).items():
        setattr(o, k, v)
    return o


def register_scans_loam(ref_edge_start, ref_edges, ref_surf_start, ref_surfs, tgt_edge_start, tgt_edges, tgt_surf_start, tgt_surfs, T_init=None,
                        max_corr=capi.LOAM_DEFAULTS["max_corr"], min_measurements=capi.LOAM_DEFAULTS["min_measurements"],
                        max_outer=capi.LOAM_DEFAULTS["max_outer"], conv_translation_m=capi.LOAM_DEFAULTS["conv_translation_m"],
                        conv_rotation_deg=capi.LOAM_DEFAULTS["conv_rotation_deg"], inner=None, loss_kind=capi.LOAM_DEFAULTS["loss_kind"],
                        loss_a=capi.LOAM_DEFAULTS["loss_a"], grid_cell=capi.LOAM_DEFAULTS["grid_cell"], device=0):
    """bsgpu_register_scans_loam: LOAM registration from feature clouds (the reference's matcher in its shipped LOAM configuration) for a
    batch of scan pairs.  Pair p moves the target's edge features tgt_edges[tgt_edge_start[p]:tgt_edge_start[p+1]] and surface features
    (under T_init[p], 3 x 4, first when given) onto the reference's, which are searched.  inner: see loam_options.  Returns a dict of
    arrays: T_refest_ref and T_ref_tgt (P x 3 x 4), cov (P x 6 x 6, tangent [p, theta]), cost, n_edge, n_surf, n_iters, n_inner, status (P)."""
    import numpy as np
    starts = [np.ascontiguousarray(a, np.int32).reshape(-1) for a in (ref_edge_start, ref_surf_start, tgt_edge_start, tgt_surf_start)]
    clouds = [np.ascontiguousarray(a, np.float64).reshape(-1, 3) for a in (ref_edges, ref_surfs, tgt_edges, tgt_surfs)]
    P = starts[0].size - 1
    ti = None if T_init is None else np.ascontiguousarray(T_init, np.float64).reshape(-1, 3, 4)
    if P < 0 or any(a.size != P + 1 for a in starts) or (ti is not None and ti.shape[0] != P):
        raise capi.SolverError(capi.ERR_INVALID, "register_scans_loam: array sizes do not agree")
    if any(int(a.max()) > c.shape[0] for a, c in zip(starts, clouds)):
        raise capi.SolverError(capi.ERR_INVALID, "register_scans_loam: a start table names more points than were passed")
    out = dict(T_refest_ref=np.zeros((P, 3, 4)), T_ref_tgt=np.zeros((P, 3, 4)), cov=np.zeros((P, 6, 6)), cost=np.zeros(P),
               n_edge=np.zeros(P, np.int32), n_surf=np.zeros(P, np.int32), n_iters=np.zeros(P, np.int32), n_inner=np.zeros(P, np.int32),
               status=np.zeros(P, np.int32))
    fn = lib().bsgpu_register_scans_loam
    fn.argtypes = capi.REGISTER_SCANS_LOAM_ARGTYPES
    _dp, _ip = capi._dp, capi._ip
    d = lambda x: None if x is None else x.ctypes.data_as(_dp)
    i = lambda x: x.ctypes.data_as(_ip)
    opt = loam_options(inner)
    rc = fn(device, P, i(starts[0]), d(clouds[0]), i(starts[1]), d(clouds[1]), i(starts[2]), d(clouds[2]), i(starts[3]), d(clouds[3]), d(ti),
            float(max_corr), int(min_measurements), int(max_outer), float(conv_translation_m), float(conv_rotation_deg), ctypes.byref(opt),
            int(loss_kind), float(loss_a), float(grid_cell), d(out["T_refest_ref"]), d(out["T_ref_tgt"]), d(out["cov"]), d(out["cost"]),
            i(out["n_edge"]), i(out["n_surf"]), i(out["n_iters"]), i(out["n_inner"]), i(out["status"]))
    if rc != 0:
        raise capi.SolverError(rc, register_scans_error())
    return out


def extract_loam_features(scan_start, points, ring=None, weak=True, labels=True, curvature=True, with_points=True, device=0, **params):
    """bsgpu_extract_loam_features: LOAM feature extraction (the reference's LoamFeatureExtractor in its shipped configuration) for a
    batch of scans.  Scan s is points[scan_start[s]:scan_start[s+1]]; ring: optional, one per point.  params: the keys of
    capi.LOAM_FEATURE_DEFAULTS (vertical_axis also as "X", "Y" or "Z").  Returns a dict of arrays: edge_start, edge_index, edge_points
    (SHARP) and surf_* (FLAT) — the edges / surfs arrays of register_scans_loam —, with weak the same for weak_edge_* (LESS_SHARP) and
    weak_surf_* (LESS_FLAT), with labels label and with curvature curvature, per input point.  with_points false leaves the *_points out."""
    import numpy as np
    unknown = set(params) - set(capi.LOAM_FEATURE_DEFAULTS)
    if unknown:
        raise TypeError(f"extract_loam_features: unknown parameters {sorted(unknown)}")
    P = dict(capi.LOAM_FEATURE_DEFAULTS, **params)
    if isinstance(P["vertical_axis"], str):
        P["vertical_axis"] = {"X": capi.AXIS_X, "Y": capi.AXIS_Y, "Z": capi.AXIS_Z}.get(P["vertical_axis"].upper(), -1)
    ss = np.ascontiguousarray(scan_start, np.int32).reshape(-1)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    rg = None if ring is None else np.ascontiguousarray(ring, np.int32).reshape(-1)
    S = ss.size - 1
    if S < 0 or (rg is not None and rg.size != pts.shape[0]):
        raise capi.SolverError(capi.ERR_INVALID, "extract_loam_features: array sizes do not agree")
    if int(ss.max()) > pts.shape[0]:
        raise capi.SolverError(capi.ERR_INVALID, "extract_loam_features: scan_start names more points than were passed")
    # the capacities of the contract, for the whole call
    n = pts.shape[0]
    cells = S * max(int(P["number_of_beams"]), 0) * max(int(P["n_feature_regions"]), 0)
    sharp, less = max(int(P["max_corner_sharp"]), 0), max(int(P["max_corner_less_sharp"]), 0)
    cap = dict(edge=min(n, cells * min(sharp, less)), surf=min(n, cells * max(int(P["max_surface_flat"]), 0)), weak_edge=min(n, cells * max(less - sharp, 0)),
               weak_surf=n)
    out = {}
    for k in ("edge", "surf") + (("weak_edge", "weak_surf") if weak else ()):
        out[k + "_start"] = np.zeros(S + 1, np.int32)
        out[k + "_index"] = np.zeros(cap[k], np.int32)
        if with_points:
            out[k + "_points"] = np.zeros((cap[k], 3))
    if labels:
        out["label"] = np.zeros(n, np.int32)
    if curvature:
        out["curvature"] = np.zeros(n)
    fn = lib().bsgpu_extract_loam_features
    fn.argtypes = capi.EXTRACT_LOAM_FEATURES_ARGTYPES
    _dp, _ip = capi._dp, capi._ip
    d = lambda x: None if x is None else x.ctypes.data_as(_dp)
    i = lambda x: None if x is None else x.ctypes.data_as(_ip)
    clouds = []
    for k in ("edge", "surf", "weak_edge", "weak_surf"):
        clouds += [i(out.get(k + "_start")), i(out.get(k + "_index")), d(out.get(k + "_points"))]
    rc = fn(device, S, i(ss), d(pts), i(rg), int(P["number_of_beams"]), float(P["fov_deg"]), int(P["vertical_axis"]), int(P["n_feature_regions"]),
            int(P["curvature_region"]), int(P["max_corner_sharp"]), int(P["max_corner_less_sharp"]), int(P["max_surface_flat"]),
            float(P["surface_curvature_threshold"]), int(P["downsample_less_flat_features"]), *clouds, i(out.get("label")), d(out.get("curvature")))
    if rc != 0:
        raise capi.SolverError(rc, register_scans_error())
    for k in ("edge", "surf", "weak_edge", "weak_surf"):
        if k + "_start" in out:
            m = int(out[k + "_start"][-1]) if S > 0 else 0
            out[k + "_index"] = out[k + "_index"][:m]
            if with_points:
                out[k + "_points"] = out[k + "_points"][:m]
    return out


def build_registration_maps(map_scan_start, scan_start, points, T_map_scan=None, voxel_size=0.1, counts=True, device=0):
    """bsgpu_build_registration_maps: the reference clouds of scan-to-map registration (RegistrationMap::GetLoamCloudMap /
    GetPointCloudMap) for a batch of maps.  Map m owns scans map_scan_start[m]:map_scan_start[m+1], scan s is
    points[scan_start[s]:scan_start[s+1]] in its own frame, T_map_scan (optional) is 3 x 4 per scan; voxel_size capi.MAP_MERGE_ONLY
    merges only.  Returns a dict: map_start, map_points (the ref_*_start / ref_* arrays of register_scans_loam) and, with counts,
    map_count."""
    import numpy as np
    ms = np.ascontiguousarray(map_scan_start, np.int32).reshape(-1)
    ss = np.ascontiguousarray(scan_start, np.int32).reshape(-1)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    T = None if T_map_scan is None else np.ascontiguousarray(T_map_scan, np.float64).reshape(-1, 12)
    M = ms.size - 1
    if M < 0 or ss.size < 1 or (M > 0 and int(ms.max()) > ss.size - 1) or (T is not None and T.shape[0] != ss.size - 1):
        raise capi.SolverError(capi.ERR_INVALID, "build_registration_maps: array sizes do not agree")
    if int(ss.max()) > pts.shape[0]:
        raise capi.SolverError(capi.ERR_INVALID, "build_registration_maps: scan_start names more points than were passed")
    n = pts.shape[0]
    out = dict(map_start=np.zeros(M + 1, np.int32), map_points=np.zeros((n, 3)))
    if counts:
        out["map_count"] = np.zeros(n, np.int32)
    fn = lib().bsgpu_build_registration_maps
    fn.argtypes = capi.BUILD_REGISTRATION_MAPS_ARGTYPES
    _dp, _ip = capi._dp, capi._ip
    d = lambda x: None if x is None else x.ctypes.data_as(_dp)
    i = lambda x: None if x is None else x.ctypes.data_as(_ip)
    rc = fn(device, M, i(ms), i(ss), d(pts), d(T), float(voxel_size), i(out["map_start"]), d(out["map_points"]), i(out.get("map_count")))
    if rc != 0:
        raise capi.SolverError(rc, register_scans_error())
    m = int(out["map_start"][-1]) if M > 0 else 0
    out["map_points"] = out["map_points"][:m]
    if counts:
        out["map_count"] = out["map_count"][:m]
    return out


def register_scans_error():
    """What this thread's last failed bsgpu_register_scans objected to."""
    fn = lib().bsgpu_register_scans_error
    fn.restype = ctypes.c_char_p
    fn.argtypes = []
    return fn().decode()


def scan_context_describe(scan_start, points, member_start, member_scan, member_T=None, lidar_height=capi.SC_DEFAULTS["lidar_height"],
                          max_radius=capi.SC_DEFAULTS["max_radius"], device=0):
    """bsgpu_scan_context_describe: the Scan Context descriptor of a batch of aggregated scans.  Scan k is
    points[scan_start[k]:scan_start[k+1]] (lidar frame); aggregate a is the union of its members member_start[a] .. member_start[a+1],
    member m being scan member_scan[m] through member_T[m] (3 x 4; None: identity).  Returns a dict of arrays: desc (A x 20 x 60),
    ring_key (A x 20), sector_key (A x 60), n_binned (A)."""
    import numpy as np
    ss = np.ascontiguousarray(scan_start, np.int32).reshape(-1)
    ms = np.ascontiguousarray(member_start, np.int32).reshape(-1)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    mscan = np.ascontiguousarray(member_scan, np.int32).reshape(-1)
    mT = None if member_T is None else np.ascontiguousarray(member_T, np.float64).reshape(-1, 3, 4)
    S, A = ss.size - 1, ms.size - 1
    if S < 0 or A < 0 or (mT is not None and mT.shape[0] != mscan.size):
        raise capi.SolverError(capi.ERR_INVALID, "scan_context_describe: array sizes do not agree")
    if int(ss.max()) > pts.shape[0] or int(ms.max()) > mscan.size:
        raise capi.SolverError(capi.ERR_INVALID, "scan_context_describe: scan_start / member_start name more entries than were passed")
    out = dict(desc=np.zeros((A, capi.SC_RINGS, capi.SC_SECTORS)), ring_key=np.zeros((A, capi.SC_RINGS)),
               sector_key=np.zeros((A, capi.SC_SECTORS)), n_binned=np.zeros(A, np.int32))
    fn = lib().bsgpu_scan_context_describe
    fn.argtypes = capi.SCAN_CONTEXT_DESCRIBE_ARGTYPES
    _dp, _ip = capi._dp, capi._ip
    d = lambda x: None if x is None else x.ctypes.data_as(_dp)
    i = lambda x: x.ctypes.data_as(_ip)
    rc = fn(device, S, i(ss), d(pts), A, i(ms), i(mscan), d(mT), float(lidar_height), float(max_radius), d(out["desc"]), d(out["ring_key"]),
            d(out["sector_key"]), i(out["n_binned"]))
    if rc != 0:
        raise capi.SolverError(rc, scan_context_error())
    return out


def scan_context_match(query_start, query_desc, cand_start, cand_desc, n_tree_candidates=capi.SC_DEFAULTS["n_tree_candidates"],
                       search_ratio=capi.SC_DEFAULTS["search_ratio"], dist_thres=capi.SC_DEFAULTS["dist_thres"], device=0):
    """bsgpu_scan_context_match: for every query descriptor the best candidate descriptor of its set over column shifts.  Set s holds
    queries query_start[s] .. query_start[s+1] and candidates cand_start[s] .. cand_start[s+1].  Returns a dict of arrays: best_cand
    (index inside the set, -1: none below dist_thres), best_dist, best_shift, yaw (per query); dist_all, shift_all (per query and
    candidate of its set, in order), pair_start (Q + 1: where a query's entries begin in them)."""
    import numpy as np
    qs = np.ascontiguousarray(query_start, np.int32).reshape(-1)
    cs = np.ascontiguousarray(cand_start, np.int32).reshape(-1)
    qd = np.ascontiguousarray(query_desc, np.float64).reshape(-1, capi.SC_RINGS, capi.SC_SECTORS)
    cd = np.ascontiguousarray(cand_desc, np.float64).reshape(-1, capi.SC_RINGS, capi.SC_SECTORS)
    n_sets = qs.size - 1
    if n_sets < 0 or cs.size != qs.size:
        raise capi.SolverError(capi.ERR_INVALID, "scan_context_match: array sizes do not agree")
    if int(qs.max()) > qd.shape[0] or int(cs.max()) > cd.shape[0]:
        raise capi.SolverError(capi.ERR_INVALID, "scan_context_match: query_start / cand_start name more descriptors than were passed")
    Q = max(int(qs[-1]), 0)
    per_query = np.zeros(Q, np.int64)
    if (np.diff(qs) >= 0).all() and (np.diff(cs) >= 0).all() and qs[0] == 0 and cs[0] == 0:
        per_query = np.repeat(np.diff(cs).astype(np.int64), np.diff(qs))
    pair_start = np.concatenate([[0], np.cumsum(per_query)]).astype(np.int64)
    P = int(pair_start[-1])
    out = dict(best_cand=np.zeros(Q, np.int32), best_dist=np.zeros(Q), best_shift=np.zeros(Q, np.int32), yaw=np.zeros(Q),
               dist_all=np.zeros(P), shift_all=np.zeros(P, np.int32), pair_start=pair_start)
    fn = lib().bsgpu_scan_context_match
    fn.argtypes = capi.SCAN_CONTEXT_MATCH_ARGTYPES
    _dp, _ip = capi._dp, capi._ip
    d = lambda x: x.ctypes.data_as(_dp)
    i = lambda x: x.ctypes.data_as(_ip)
    rc = fn(device, n_sets, i(qs), d(qd), i(cs), d(cd), int(n_tree_candidates), float(search_ratio), float(dist_thres), i(out["best_cand"]),
            d(out["best_dist"]), i(out["best_shift"]), d(out["yaw"]), d(out["dist_all"]), i(out["shift_all"]))
    if rc != 0:
        raise capi.SolverError(rc, scan_context_error())
    return out


def scan_context_error():
    """What this thread's last failed bsgpu_scan_context_describe or bsgpu_scan_context_match objected to."""
    fn = lib().bsgpu_scan_context_error
    fn.restype = ctypes.c_char_p
    fn.argtypes = []
    return fn().decode()


class GpuSolver(capi.Solver):
    """One bsgpu context on HIP device `device`."""

    def __init__(self, device=0):
        super().__init__(lib(), "bsgpu_", device)

    def reprojection_errors(self, n):
        """Pixel error of the n reprojection factors (REPROJ then REPROJ_ONLINE_CALIB, insertion order) at the current values."""
        import numpy as np
        out = np.zeros(n)
        fn = lib().bsgpu_reprojection_errors
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(fn(self._ctx, out.ctypes.data))
        return out

    def backsub_tangent_table(self, n):
        """bsgpu_backsub_tangent_table for the n reprojection factors -> (fac_t (n,2), the same joined from the per-camera-pose tables (n,2));
        -2 where a factor is not in the landmark tables."""
        import numpy as np
        ft, jn = np.full((n, 2), -2, np.int32), np.full((n, 2), -2, np.int32)
        fn = lib().bsgpu_backsub_tangent_table
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(fn(self._ctx, ft.ctypes.data, jn.ctypes.data))
        return ft, jn

    def triangulate(self, track_start, q_block, p_block, pixels, camera=0, truncate_pixels=True, max_dist=-1.0, max_reproj=-1.0):
        """bsgpu_triangulate: DLT triangulation of a batch of feature tracks at the current values -> (points (n,3), status (n,))."""
        import numpy as np
        ts = np.ascontiguousarray(track_start, np.int32)
        qb, pb = np.ascontiguousarray(q_block, np.int32), np.ascontiguousarray(p_block, np.int32)
        px = np.ascontiguousarray(pixels, np.float64)
        n = ts.size - 1
        pts, st = np.zeros((n, 3)), np.zeros(n, np.int32)
        fn = lib().bsgpu_triangulate
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                                                                  ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(fn(self._ctx, n, ts.ctypes.data, qb.ctypes.data, pb.ctypes.data, px.ctypes.data, int(camera), int(bool(truncate_pixels)),
                     float(max_dist), float(max_reproj), pts.ctypes.data, st.ctypes.data))
        return pts, st

    def essential_ransac(self, match_start, px_prev, px_cur, K, prob=0.99, threshold_px=1.0, max_iters=1000, seed=0):
        """bsgpu_essential_ransac: cv::findEssentialMat(..., cv::RANSAC, prob, threshold_px, mask) for a batch of match sets.  Set k
        holds matches [match_start[k], match_start[k+1]); px_prev / px_cur (n x 2) pixels; K (n_sets x 4, or 4 for all): fx fy cx cy.
        Returns a dict of arrays: mask (n, uint8), E (S x 3 x 3), n_inliers, n_iters, best_sample (S x 5), status (S)."""
        import numpy as np
        ms = np.ascontiguousarray(match_start, np.int32)
        S = ms.size - 1
        p1 = np.ascontiguousarray(px_prev, np.float64).reshape(-1, 2)
        p2 = np.ascontiguousarray(px_cur, np.float64).reshape(-1, 2)
        Ks = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 4), (S, 4)))
        if p1.shape != p2.shape or (ms.size and p1.shape[0] < int(ms.max())):
            raise capi.SolverError(capi.ERR_INVALID, "essential_ransac: match_start names more matches than were passed")
        out = dict(mask=np.zeros(p1.shape[0], np.uint8), E=np.zeros((S, 3, 3)), n_inliers=np.zeros(S, np.int32), n_iters=np.zeros(S, np.int32),
                   best_sample=np.zeros((S, 5), np.int32), status=np.zeros(S, np.int32))
        fn = lib().bsgpu_essential_ransac
        fn.argtypes = capi.ESSENTIAL_RANSAC_ARGTYPES
        _dp, _ip, _bp = capi._dp, capi._ip, capi._bp
        self._chk(fn(self._ctx, S, ms.ctypes.data_as(_ip), p1.ctypes.data_as(_dp), p2.ctypes.data_as(_dp), Ks.ctypes.data_as(_dp),
                     float(prob), float(threshold_px), int(max_iters), int(seed) & ((1 << 64) - 1), out["mask"].ctypes.data_as(_bp),
                     out["E"].ctypes.data_as(_dp), out["n_inliers"].ctypes.data_as(_ip), out["n_iters"].ctypes.data_as(_ip),
                     out["best_sample"].ctypes.data_as(_ip), out["status"].ctypes.data_as(_ip)))
        return out

    def absolute_pose_ransac(self, obs_start, pixels, points, camera=0, prob=0.0, threshold_px=5.0, max_iters=100, seed=0,
                             truncate_pixels=False):
        """bsgpu_absolute_pose_ransac: beam_cv::AbsolutePoseEstimator::RANSACEstimator(cam, pixels, points, max_iters) for a batch of
        frames.  Frame f holds pairs [obs_start[f], obs_start[f+1]); pixels (n x 2), points (n x 3, world); camera (per frame, or one
        for all): index into set_cameras' table.  prob = 0: the fixed loop; prob in (0, 1): early termination.
        Returns a dict of arrays: mask (n, uint8), q (F x 4, wxyz) / p (F x 3): T_WORLD_BASELINK, localize_frames' q_init / p_init;
        T_cam_world (F x 3 x 4), n_inliers, n_iters, best_sample (F x 3), status (F).  NaN poses where status is not RANSAC_OK."""
        import numpy as np
        os_ = np.ascontiguousarray(obs_start, np.int32)
        F = os_.size - 1
        pix = np.ascontiguousarray(pixels, np.float64).reshape(-1, 2)
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        cam = np.ascontiguousarray(np.broadcast_to(np.asarray(camera, np.int32), (F,)))
        if pix.shape[0] != pts.shape[0] or (os_.size and pix.shape[0] < int(os_.max())):
            raise capi.SolverError(capi.ERR_INVALID, "absolute_pose_ransac: obs_start names more pairs than were passed")
        out = dict(mask=np.zeros(pix.shape[0], np.uint8), q=np.zeros((F, 4)), p=np.zeros((F, 3)), T_cam_world=np.zeros((F, 3, 4)),
                   n_inliers=np.zeros(F, np.int32), n_iters=np.zeros(F, np.int32), best_sample=np.zeros((F, 3), np.int32),
                   status=np.zeros(F, np.int32))
        fn = lib().bsgpu_absolute_pose_ransac
        fn.argtypes = capi.ABSOLUTE_POSE_RANSAC_ARGTYPES
        _dp, _ip, _bp = capi._dp, capi._ip, capi._bp
        self._chk(fn(self._ctx, F, os_.ctypes.data_as(_ip), pix.ctypes.data_as(_dp), pts.ctypes.data_as(_dp), cam.ctypes.data_as(_ip),
                     float(prob), float(threshold_px), int(max_iters), int(seed) & ((1 << 64) - 1), int(bool(truncate_pixels)),
                     out["mask"].ctypes.data_as(_bp), out["q"].ctypes.data_as(_dp), out["p"].ctypes.data_as(_dp),
                     out["T_cam_world"].ctypes.data_as(_dp), out["n_inliers"].ctypes.data_as(_ip), out["n_iters"].ctypes.data_as(_ip),
                     out["best_sample"].ctypes.data_as(_ip), out["status"].ctypes.data_as(_ip)))
        return out

    def relative_pose_ransac(self, match_start, px_first, px_last, camera=0, prob=0.0, threshold_px=5.0, max_iters=100, seed=0,
                             truncate_pixels=False, validate_px=10.0, min_inlier_ratio=0.8):
        """bsgpu_relative_pose_ransac: the two-view bootstrap of ComputePathWithVision — seven-point RANSAC relative pose of the last
        image against the first, triangulation of every match and the validity gate — for a batch of match sets.  Set k holds matches
        [match_start[k], match_start[k+1]); px_first / px_last (n x 2) pixels; camera (per set, or one for all): index into
        set_cameras' table.  prob = 0: the fixed loop; prob in (0, 1): early termination.
        Returns a dict of arrays: mask (n, uint8), T_last_first (S x 3 x 4), q (S x 2 x 4, wxyz) / p (S x 2 x 3): T_WORLD_BASELINK of
        the first and the last image (world = first camera), points (n x 3, first camera's frame), valid_mask (n, uint8),
        inlier_ratio, pair_valid, n_inliers, n_iters, best_sample (S x 7), status (S).  NaN where status is not RANSAC_OK."""
        import numpy as np
        ms = np.ascontiguousarray(match_start, np.int32)
        S = ms.size - 1
        p0 = np.ascontiguousarray(px_first, np.float64).reshape(-1, 2)
        p1 = np.ascontiguousarray(px_last, np.float64).reshape(-1, 2)
        cam = np.ascontiguousarray(np.broadcast_to(np.asarray(camera, np.int32), (S,)))
        if p0.shape != p1.shape or (ms.size and p0.shape[0] < int(ms.max())):
            raise capi.SolverError(capi.ERR_INVALID, "relative_pose_ransac: match_start names more matches than were passed")
        n = p0.shape[0]
        out = dict(mask=np.zeros(n, np.uint8), T_last_first=np.zeros((S, 3, 4)), q=np.zeros((S, 2, 4)), p=np.zeros((S, 2, 3)),
                   points=np.zeros((n, 3)), valid_mask=np.zeros(n, np.uint8), inlier_ratio=np.zeros(S), pair_valid=np.zeros(S, np.int32),
                   n_inliers=np.zeros(S, np.int32), n_iters=np.zeros(S, np.int32), best_sample=np.zeros((S, 7), np.int32),
                   status=np.zeros(S, np.int32))
        fn = lib().bsgpu_relative_pose_ransac
        fn.argtypes = capi.RELATIVE_POSE_RANSAC_ARGTYPES
        _dp, _ip, _bp = capi._dp, capi._ip, capi._bp
        self._chk(fn(self._ctx, S, ms.ctypes.data_as(_ip), p0.ctypes.data_as(_dp), p1.ctypes.data_as(_dp), cam.ctypes.data_as(_ip),
                     float(prob), float(threshold_px), int(max_iters), int(seed) & ((1 << 64) - 1), int(bool(truncate_pixels)),
                     float(validate_px), float(min_inlier_ratio), out["mask"].ctypes.data_as(_bp), out["T_last_first"].ctypes.data_as(_dp),
                     out["q"].ctypes.data_as(_dp), out["p"].ctypes.data_as(_dp), out["points"].ctypes.data_as(_dp),
                     out["valid_mask"].ctypes.data_as(_bp), out["inlier_ratio"].ctypes.data_as(_dp), out["pair_valid"].ctypes.data_as(_ip),
                     out["n_inliers"].ctypes.data_as(_ip), out["n_iters"].ctypes.data_as(_ip), out["best_sample"].ctypes.data_as(_ip),
                     out["status"].ctypes.data_as(_ip)))
        return out

    @staticmethod
    def batch_stats():
        """(windows solved by the batched launches of bsgpu_solve_batch so far in this process, rounds = sets of launches they took)."""
        w, r = ctypes.c_int64(0), ctypes.c_int64(0)
        lib().bsgpu_batch_stats(ctypes.byref(w), ctypes.byref(r))
        return w.value, r.value

    def time_reproj_jacobian_ms(self, reps=20):
        ms = lib().bsgpu_time_reproj_jacobian_ms(self._ctx, int(reps))
        if ms < 0:
            raise capi.SolverError(capi.ERR_DEVICE, "bsgpu_time_reproj_jacobian_ms failed")
        return ms

    def time_eval_ms(self, reps=20):
        """Mean milliseconds of one evaluation of residuals + Jacobians of every factor type (HIP events on the solver's stream)."""
        ms = lib().bsgpu_time_eval_ms(self._ctx, int(reps))
        if ms < 0:
            raise capi.SolverError(capi.ERR_DEVICE, "bsgpu_time_eval_ms failed")
        return ms

    def eval_bytes(self):
        return lib().bsgpu_eval_bytes(self._ctx)

    def bsr_info(self):
        """(block rows, non-zero 3x3 blocks) of the block-sparse PCG path; (0, 0) on the dense Schur path."""
        a, b = ctypes.c_int32(0), ctypes.c_int32(0)
        self._chk(lib().bsgpu_bsr_info(ctypes.c_void_p(self._ctx), ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    PHASES = ("eval_reproj", "eval_other", "landmark", "pairs", "assemble_other", "factor", "backsolve", "backsub", "candidate")

    def profile_step(self, options=None, reps=10):
        """bsgpu_profile_step: {phase: (mean ms, algorithmic work)} of a full LM step timed in situ with HIP events (bytes; flops for
        'factor')."""
        import numpy as np
        opt = options if options is not None else self.options_default()
        ms, work = np.zeros(len(self.PHASES)), np.zeros(len(self.PHASES))
        fn = lib().bsgpu_profile_step
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(fn(self._ctx, ctypes.byref(opt), int(reps), ms.ctypes.data, work.ctypes.data))
        return {name: (float(ms[i]), float(work[i])) for i, name in enumerate(self.PHASES)}

    def set_plan_preference(self, throughput):
        """bsgpu_set_plan_preference: BSGPU_PLAN_THROUGHPUT for a window that is one of many in bsgpu_solve_batch, BSGPU_PLAN_LATENCY (default) otherwise."""
        fn = lib().bsgpu_set_plan_preference
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        self._chk(fn(self._ctx, 1 if throughput else 0))

    def plan_info(self):
        """(independent sub-chains, schedule steps, 64-wide tiles) of the reduced system's Cholesky plan."""
        a, b, c = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self.finalize()
        lib().bsgpu_plan_info(ctypes.c_void_p(self._ctx), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return a.value, b.value, c.value

    def reproj_jacobian_bytes(self):
        return lib().bsgpu_reproj_jacobian_bytes(self._ctx)
