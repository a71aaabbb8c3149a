/*
 * bsgpu.h — C-ABI of the MI355X-native fixed-lag-smoother solve path.
 *
 * This is the drop-in boundary for the ONE call the reference's optimizer makes
 * on its hot path:
 *
 *     summary_ = graph_->optimize(params_.solver_options);
 *         (reference: bs_optimizers/src/fixed_lag_smoother.cpp:281, and the ten
 *          other optimize()/optimizeFor() call sites listed in SURVEY.md §3.4)
 *
 * In the reference that call walks a fuse_core::Graph, builds a ceres::Problem
 * (AddParameterBlock / SetParameterBlockConstant / AddResidualBlock) and runs
 * ceres::Solve.  Nothing like a C interface exists there (it is C++ virtuals all
 * the way down), so the entry points below are what a fuse_core::Graph
 * implementation would bind to hand the flattened problem to the GPU:
 *
 *   bsgpu_set_blocks        <- Graph::createProblem: AddParameterBlock(data,size,
 *                              localParameterization) + SetParameterBlockConstant
 *                              for holdConstant() variables
 *   bsgpu_set_cameras       <- the (K, T_cam_baselink) pair every
 *                              EuclideanReprojectionConstraint carries
 *                              (bs_constraints/.../euclidean_reprojection_constraint.h:80-84)
 *   bsgpu_add_factors       <- AddResidualBlock(c.costFunction(), c.lossFunction(), blocks)
 *   bsgpu_solve             <- ceres::Solve(options, &problem, &summary)
 *   bsgpu_get_blocks        <- variables updated in place through Variable::data()
 *   bsgpu_get_iteration     <- summary.iterations[i]
 *   bsgpu_evaluate          <- ceres::Problem::Evaluate (used by the reference's tests,
 *                              bs_constraints/tests/euclidean_reprojection_test.cpp:150-180)
 *   bsgpu_covariance        <- Graph::getCovariance (bs_publishers/src/odometry_3d_publisher.cpp:82)
 *
 * Plain C types only: pointers, sizes, POD structs.  Host buffers are
 * caller-owned and copied on set/add; device memory is owned by the context.
 * All arithmetic is IEEE double, like the reference.
 *
 * Threading: a context is single-caller (the reference holds
 * optimization_mutex_ around optimize(), fixed_lag_smoother.cpp:185).
 *
 * Error model: every call returns BSGPU_OK (0) or a negative code;
 * bsgpu_last_error() returns a human-readable message for the last failure on
 * the context.  "NO_CONVERGENCE" is not an error (fixed_lag_smoother.cpp:284-285);
 * an unusable solution is reported through summary.is_solution_usable == 0 so
 * the caller can take the reference's fatal path (fixed_lag_smoother.cpp:286-295).
 */
#ifndef BSGPU_H_
#define BSGPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSGPU_ABI_VERSION 1

/* ---- return codes --------------------------------------------------------- */
enum {
  BSGPU_OK = 0,
  BSGPU_ERR_INVALID = -1,     /* bad argument / inconsistent problem          */
  BSGPU_ERR_DEVICE = -2,      /* HIP runtime failure or no device             */
  BSGPU_ERR_UNSUPPORTED = -3, /* problem shape the GPU path does not cover    */
  BSGPU_ERR_NUMERIC = -4      /* non-finite values / fatal linear-solver error */
};

/* ---- manifold kinds (fuse_core::Variable::localParameterization()) -------- */
enum {
  BSGPU_MANIFOLD_EUCLIDEAN = 0, /* nullptr parameterisation                    */
  BSGPU_MANIFOLD_QUAT_RIGHT = 1 /* fuse_variables::Orientation3DLocalParameterization:
                                   x (+) d = x (x) AngleAxisToQuaternion(d),
                                   (w,x,y,z) storage; restated in-tree by
                                   bs_constraints/src/jacobians.cpp:24-35,144-158 */
};

/* ---- loss kinds (fuse_core::Loss -> ceres::LossFunction) ------------------ */
enum {
  BSGPU_LOSS_TRIVIAL = 0,
  BSGPU_LOSS_CAUCHY = 1, /* ceres::CauchyLoss(a): rho(s) = a^2 log(1 + s/a^2)  */
  BSGPU_LOSS_HUBER = 2   /* ceres::HuberLoss(a)                                */
};

/* ---- factor types ----------------------------------------------------------
 * For every type: `block_idx` is n x BSGPU_NIDX(type) int32 (row-major) of
 * indices into the block table, in the constraint's variables() order;
 * `consts` is n x BSGPU_NCONST(type) doubles (row-major).
 */
enum {
  /* bs_constraints::EuclideanReprojectionConstraint
   *   (visual/euclidean_reprojection_function.h:28-179, SizedCostFunction<2,4,3,3>)
   *   idx   : q_WORLD_BASELINK, t_WORLD_BASELINK, P_WORLD, camera-table index
   *   consts: u, v (pixel), w (sqrt information = w * I2)                      */
  BSGPU_F_REPROJ = 0,
  /* bs_constraints::EuclideanReprojectionConstraintOnlineCalib
   *   (visual/euclidean_reprojection_functor_online_calib.h:16-83, AutoDiff<2,4,3,3,4,3>)
   *   idx   : q_WB, t_WB, P, q_BASELINK_CAM, p_BASELINK_CAM, camera-table index (K only)
   *   consts: u, v, w
   *   The two extrinsic blocks are constant in the reference as shipped (bs_variables::
   *   Orientation3D / Position3D::holdConstant() == true, bs_variables/src/orientation_3d.cpp:39-41):
   *   their values are then folded into a derived camera at bsgpu_finalize().  ONE pair per
   *   window may be free instead (both blocks, or one of them) — online calibration: it is
   *   estimated with the window, the landmarks still eliminated, and bsgpu_evaluate, bsgpu_solve,
   *   the covariance queries of pose-side blocks (the pair's two included) and
   *   bsgpu_reprojection_errors work at its current values.  Such a window is solved by LM on the
   *   exact path.  BSGPU_ERR_UNSUPPORTED: a second free pair; such a factor on a landmark block
   *   that is not eliminated (shared with another kind of factor), or whose pose and landmark
   *   blocks are all constant; BSGPU_TR_DOGLEG, BSGPU_LINEAR_PCG / SCHUR_PCG; bsgpu_marginalize;
   *   bsgpu_covariance_requests naming an eliminated landmark of such a window.               */
  BSGPU_F_REPROJ_ONLINE_CALIB = 1,
  /* bs_constraints::RelativeImuState3DStampedConstraint
   *   (inertial/normal_delta_imu_state_3d_cost_functor.h:18-141, AutoDiff<15, 4,3,3,3,3, 4,3,3,3,3>)
   *   idx   : (q,p,v,bg,ba)_i, (q,p,v,bg,ba)_j
   *   consts: dt, dq[4 wxyz], dp[3], dv[3], dq_dbg[9], dp_dbg[9], dp_dba[9],
   *           dv_dbg[9], dv_dba[9] (3x3 row-major), bg_lin[3], ba_lin[3],
   *           A[225] (15x15 row-major = info_weight * sqrt_inv_cov)             */
  BSGPU_F_IMU_DELTA = 2,
  /* bs_constraints::AbsoluteImuState3DStampedConstraint
   *   (inertial/normal_prior_imu_state_3d_cost_functor.h:28-90, AutoDiff<15,4,3,3,3,3>)
   *   idx   : q,p,v,bg,ba        consts: b[16] (q wxyz,p,v,bg,ba), A[225]      */
  BSGPU_F_IMU_PRIOR = 3,
  /* bs_constraints::RelativePose3DStampedWithExtrinsicsConstraint
   *   (relative_pose/delta_pose_3d_with_extrinsics_cost_functor.h:19-109, AutoDiff<6,3,4,3,4,3,4>)
   *   idx   : p1,q1,p2,q2,p_ext,q_ext   consts: d[7] (x,y,z,qw,qx,qy,qz), A[36] */
  BSGPU_F_RELPOSE_EXT = 4,
  /* fuse_constraints::RelativePose3DStampedConstraint (NormalDeltaPose3DCostFunctor)
   *   idx   : p1,q1,p2,q2        consts: d[7], A[36]                           */
  BSGPU_F_RELPOSE = 5,
  /* fuse_constraints::AbsolutePose3DStampedConstraint and
   * bs_constraints::AbsolutePose3DConstraint (global/absolute_pose_3d_constraint.cpp:12-52)
   *   idx   : p,q                consts: b[7] (x,y,z,qw,qx,qy,qz), A[36]       */
  BSGPU_F_ABSPOSE = 6,
  /* fuse_constraints::AbsoluteConstraint<V> for 3-vectors (global/absolute_constraint.h:10-25)
   *   idx   : x                  consts: b[3], A[9];  r = A (x - b)             */
  BSGPU_F_ABS_VEC3 = 7,
  /* fuse_constraints::RelativeConstraint<V> (relative_pose/relative_constraints.h:12-19)
   *   idx   : x1,x2              consts: d[3], A[9];  r = A ((x2 - x1) - d)     */
  BSGPU_F_REL_VEC3 = 8,
  /* bs_constraints::GravityAlignmentStampedConstraint
   *   (global/gravity_alignment_cost_functor.h:32-82, AutoDiff<2,4>)
   *   idx   : q                  consts: g_b[3], A[4] (2x2 row-major)          */
  BSGPU_F_GRAVITY = 9,
  /* bs_constraints::InverseDepthReprojectionConstraint
   *   (visual/inversedepth_reprojection_functor.h:15-136, AutoDiff<2,4,3,4,3,1>;
   *    src/visual/inversedepth_reprojection_constraint.cpp:14-49)
   *   idx   : q_WORLD_BASELINKa, p_WORLD_BASELINKa (anchor), q_WORLD_BASELINKm,
   *           p_WORLD_BASELINKm (measurement), rho (bs_variables::InverseDepthLandmark,
   *           size 1), camera-table index
   *   consts: u, v (pixel), w (sqrt information = w * I2), m[3] (bearing of the
   *           landmark in the anchor camera, InverseDepthLandmark::bearing())
   *   An inverse-depth scalar that only such factors use is eliminated on the
   *   landmark side like a Euclidean landmark (csrc/k_idp.hip; its covariance
   *   is then answered by bsgpu_covariance_requests only; BSGPU_IDP_ELIM=0 at finalize keeps it in the
   *   reduced system).  use_idp is off in every shipped configuration.         */
  BSGPU_F_IDP_REPROJ = 10,
  /* bs_constraints::InverseDepthReprojectionConstraintUnary
   *   (visual/inversedepth_reprojection_functor_unary.h:14-85, AutoDiff<2,4,3,1>)
   *   idx   : q_WORLD_BASELINKa, p_WORLD_BASELINKa, rho, camera-table index
   *   consts: u, v, w, m[3]
   *   The observation in the anchor frame: the residual is constant in every
   *   block (zero Jacobian), it only contributes to the cost.                  */
  BSGPU_F_IDP_REPROJ_UNARY = 11,
  /* bs_constraints::Unicycle3DStateKinematicConstraint
   *   (motion/unicycle_3d_state_cost_functor.h:65-125, unicycle_3d_predict.h:49-196,
   *    src/motion/unicycle_3d_state_kinematic_constraint.cpp:11-31,73-77; AutoDiff<15, 3,4,3,3,3, 3,4,3,3,3>)
   *   idx   : (p, q, v_linear, v_angular, a_linear)_1, (p, q, v_linear, v_angular, a_linear)_2
   *   consts: dt (= stamp2 - stamp1), A[225] (15x15 row-major = covariance.inverse().llt().matrixU())
   *   r = A [p2 - p^; wrap(rpy(q2) - rpy^); v2 - v^; w2 - w^; a2 - a^] with the unicycle prediction
   *   (p^, rpy^, v^, w^, a^) of state 1 over dt; rpy(q): fuse_core getRoll/getPitch/getYaw of the stored q.
   *   bs_models::Unicycle3D (unicycle_3d.cpp:256-261) emits it with covariance process_noise * dt.              */
  BSGPU_F_UNICYCLE = 12,
  BSGPU_F_NUM_TYPES = 13
};

/* number of int32 per factor in block_idx / doubles per factor in consts /
 * residual rows, for a type; -1 for an unknown type */
int bsgpu_nidx(int type);
int bsgpu_nconst(int type);
int bsgpu_nres(int type);

/* ---- linear solver choice (ceres::Solver::Options::linear_solver_type) ----- */
enum {
  BSGPU_LINEAR_AUTO = 0,         /* exact path whenever the reduced system fits */
  BSGPU_LINEAR_SCHUR_CHOLESKY = 1, /* landmark Schur complement + dense FP64
                                      Cholesky of the reduced system: the exact
                                      (SPARSE_NORMAL_CHOLESKY-equivalent) step   */
  BSGPU_LINEAR_PCG = 2,          /* block-Jacobi PCG on the block-sparse normal
                                      equations (inexact; pose-graph sized problems) */
  BSGPU_LINEAR_SCHUR_PCG = 3     /* landmark Schur complement + block-Jacobi PCG on the
                                      reduced camera system (Ceres ITERATIVE_SCHUR with
                                      SCHUR_JACOBI, the preconditioner named by
                                      beam_slam_launch/config/optimization/ceres_config.json:12;
                                      inexact: pcg_tolerance / pcg_max_iterations)        */
};

/* ---- trust-region strategy (ceres::Solver::Options::trust_region_strategy_type)
 * DOGLEG is Ceres' TRADITIONAL_DOGLEG.  It needs an exact linear solve: PCG and SCHUR_PCG are
 * refused (BSGPU_ERR_INVALID), as are an AUTO that resolves to the PCG, inverse-depth factors and
 * bsgpu_localize_frames (BSGPU_ERR_UNSUPPORTED).  SUBSPACE_DOGLEG is not implemented. ---------- */
enum {
  BSGPU_TR_LEVENBERG_MARQUARDT = 0,
  BSGPU_TR_DOGLEG = 1,
  BSGPU_TR_SUBSPACE_DOGLEG = 2   /* BSGPU_ERR_UNSUPPORTED */
};

/* ---- termination (ceres::TerminationType) ---------------------------------- */
enum {
  BSGPU_CONVERGENCE = 0,
  BSGPU_NO_CONVERGENCE = 1,
  BSGPU_FAILURE = 2
};

/* mirrors the ceres::Solver::Options fields the reference sets
 * (beam_slam_launch/config/vio.yaml:7-17) plus the Ceres defaults it relies on */
typedef struct bsgpu_options {
  int32_t max_num_iterations;           /* vio.yaml:13 -> 10; Ceres default 50  */
  int32_t linear_solver_type;           /* BSGPU_LINEAR_*                       */
  int32_t jacobi_scaling;               /* Ceres default 1                      */
  int32_t max_num_consecutive_invalid_steps; /* Ceres default 5                 */
  double max_solver_time_in_seconds;    /* vio.yaml:14 -> 0.05; <=0 = unlimited */
  double function_tolerance;            /* vio.yaml:17 -> 1.5e-7; default 1e-6  */
  double gradient_tolerance;            /* vio.yaml:15 -> 1.5e-7; default 1e-10 */
  double parameter_tolerance;           /* vio.yaml:16 -> 1.5e-7; default 1e-8  */
  double initial_trust_region_radius;   /* 1e4                                  */
  double max_trust_region_radius;       /* 1e16                                 */
  double min_trust_region_radius;       /* 1e-32                                */
  double min_relative_decrease;         /* 1e-3                                 */
  double min_lm_diagonal;               /* 1e-6                                 */
  double max_lm_diagonal;               /* 1e32                                 */
  int32_t pcg_max_iterations;           /* BSGPU_LINEAR_PCG only                */
  int32_t trust_region_strategy_type;   /* BSGPU_TR_*; default LEVENBERG_MARQUARDT */
  double pcg_tolerance;                 /* relative residual |r| / |b| at which an inner solve stops.  Default 1e-10: the reference's
                                           step on this path is the exact SPARSE_NORMAL_CHOLESKY one, and a default-option caller (the
                                           global mapper) gets a step that is equivalent to it (69 inner iterations per LM step on the
                                           5 000-pose graph of BASELINE config 4; 84 at 1e-12).  A caller that wants the inexact step
                                           sets it: at 1e-6 that graph's per-iteration costs stay within 1e-7 and the final cost within
                                           1e-10 of the exact trajectory at 39 inner iterations per LM step (scripts/c4_tolerance.py:
                                           ONE synthetic graph -- measured evidence, not a guarantee; bench.py reports both). */
} bsgpu_options;

/* fills `o` with Ceres' defaults */
void bsgpu_options_default(bsgpu_options* o);
/* fills `o` with the solver options the reference ships for VIO
 * (beam_slam_launch/config/vio.yaml:7-17) */
void bsgpu_options_vio(bsgpu_options* o);

/* mirrors the ceres::Solver::Summary fields the reference reads back
 * (fixed_lag_smoother.cpp:286,705-716) */
typedef struct bsgpu_summary {
  int32_t termination_type;      /* BSGPU_CONVERGENCE / NO_CONVERGENCE / FAILURE */
  int32_t is_solution_usable;    /* Summary::IsSolutionUsable()                  */
  int32_t num_iterations;        /* iterations.size() - 1 (iteration 0 = initial evaluation) */
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int32_t num_parameters_tangent; /* columns of the reduced problem              */
  int32_t num_residuals;
  int32_t linear_solver_used;    /* BSGPU_LINEAR_*                               */
  int32_t num_linear_solves;     /* trust-region steps computed (incl. the one a
                                    parameter/function-tolerance exit does not
                                    record in `iterations`): the unit of the
                                    "LM iterations/s" metric                     */
  int32_t num_inner_iterations;  /* PCG iterations summed over the LM steps (0 on the exact path) */
  double initial_cost;
  double final_cost;
  double fixed_cost;             /* cost of residual blocks with only constant blocks */
  double total_time_in_seconds;  /* wall clock of bsgpu_solve                    */
  double device_time_in_seconds; /* HIP-event time of the LM loop on the stream  */
  double time_eval_seconds;      /* host-timed phase splits (sum <= total)       */
  double time_assemble_seconds;
  double time_linear_solve_seconds;
  char message[160];
} bsgpu_summary;

/* one entry of ceres::Solver::Summary::iterations */
typedef struct bsgpu_iteration {
  int32_t iteration;
  int32_t step_is_valid;
  int32_t step_is_successful;
  int32_t reserved0;
  double cost;
  double cost_change;
  double gradient_max_norm;
  double gradient_norm;
  double step_norm;
  double relative_decrease;
  double trust_region_radius;
  double model_cost_change;
} bsgpu_iteration;

/* one camera-table entry: K (skew-free) and T_cam_baselink */
typedef struct bsgpu_camera {
  double fx, fy, cx, cy;
  double R_cam_baselink[9]; /* row-major */
  double t_cam_baselink[3];
} bsgpu_camera;

typedef struct bsgpu_ctx bsgpu_ctx;

/* ---- life cycle ------------------------------------------------------------ */
/* Creates a context on HIP device `device`.  Returns NULL when no HIP device is
 * usable (there is no CPU fallback); bsgpu_create_error() then says why.       */
bsgpu_ctx* bsgpu_create(int device);
const char* bsgpu_create_error(void);
void bsgpu_destroy(bsgpu_ctx* ctx);
const char* bsgpu_last_error(const bsgpu_ctx* ctx);
int bsgpu_abi_version(void);

/* ---- problem definition ---------------------------------------------------- */
/* Drops blocks, cameras and factors (Graph::clear()). */
int bsgpu_clear(bsgpu_ctx* ctx);

/* Parameter-block table.  `values` is the concatenation of all blocks' ambient
 * coordinates; block b occupies values[offset[b] .. offset[b]+size[b]).
 * manifold[b] in BSGPU_MANIFOLD_*, is_const[b] != 0 <=> SetParameterBlockConstant.
 * Block order defines the deterministic variable index:
 * tangent columns are numbered in block order, pose-side blocks first, then the
 * landmark blocks eliminated by the Schur complement.                           */
int bsgpu_set_blocks(bsgpu_ctx* ctx, int32_t n_blocks, const double* values,
                     const int32_t* offset, const uint8_t* size,
                     const uint8_t* manifold, const uint8_t* is_const);

/* Overwrites the current block values (same layout as bsgpu_set_blocks). */
int bsgpu_set_values(bsgpu_ctx* ctx, const double* values, int64_t n_values);

int bsgpu_set_cameras(bsgpu_ctx* ctx, int32_t n_cameras, const bsgpu_camera* cams);

/* Appends n factors of one type.  loss_kind / loss_a may be NULL (trivial loss).
 * Factor order (type-major, then insertion order) defines the residual index.   */
int bsgpu_add_factors(bsgpu_ctx* ctx, int32_t type, int32_t n,
                      const int32_t* block_idx, const double* consts,
                      const int32_t* loss_kind, const double* loss_a);
/* bsgpu_add_factors for a caller that keeps its factor tables across solves: the block-index columns of `slot_idx` hold
 * caller-side variable slots (stable for the lifetime of a variable) and are translated through
 * slot_to_block[n_slots] (slot -> index in the current bsgpu_set_blocks table) while the rows are copied in; camera
 * columns are copied as they are.  A slot outside [0, n_slots) or mapped to a negative block is an error.  This is what
 * lets bs_optimizers::GpuGraph (beam_slam_amd/host/gpu_graph.h) hand over its persistent packed tables unchanged
 * every cycle although the block order shifts when the window slides.                    */
int bsgpu_add_factors_indirect(bsgpu_ctx* ctx, int32_t type, int32_t n, const int32_t* slot_idx, int32_t n_slots,
                               const int32_t* slot_to_block, const double* consts, const int32_t* loss_kind,
                               const double* loss_a);
/* bsgpu_add_factors_indirect for a type's WHOLE table (one call per type per description, before any other factors of the
 * type) from a caller that also knows what changed: changed_rows[n_changed] lists every row r < n whose contents differ
 * from row r of the table passed to the previous bsgpu_sync_factors_indirect call for this type on this context (rows
 * beyond the previous table's end included; rows that left at the end need no mention).  n_changed < 0: no promise, the
 * table is read whole (the first call).  For BSGPU_F_REPROJ the back-end keeps slot-named copies of the table on the host
 * and on the device ACROSS bsgpu_clear() and patches them — a window that slides by one keyframe sends ~3 500 of 400 000
 * rows, validation and landmark detection run on per-slot use counters, and bsgpu_finalize flattens from the resident
 * device table (the per-cycle rebuild as a delta).  Other types are copied in as by
 * bsgpu_add_factors_indirect.  A wrong change list is the caller's error: BSGPU_SYNC_CHECK=1 in the environment makes the
 * call compare its copy with the table passed and fail on any difference; BSGPU_SYNC_FULL=1 ignores the lists.            */
int bsgpu_sync_factors_indirect(bsgpu_ctx* ctx, int32_t type, int32_t n, const int32_t* slot_idx, int32_t n_slots,
                                const int32_t* slot_to_block, const double* consts, const int32_t* loss_kind,
                                const double* loss_a, int32_t n_changed, const int32_t* changed_rows);

/* Dense linear prior: [EXT] fuse_constraints::MarginalConstraint, what fuse_constraints::marginalizeVariables
 * adds to the graph (bs_optimizers/src/fixed_lag_smoother.cpp:270-271, `pseudo_marginalization: false`):
 *     r = b + sum_i A_i (x_i [-] xbar_i),    [-] = LocalParameterization::Minus(xbar_i, x_i)
 *   blocks : n_blocks indices into the block table (set_blocks first)
 *   A      : n_rows x (sum of the blocks' tangent sizes), row-major, columns in `blocks` order
 *   b      : n_rows
 *   xbar   : the blocks' linearisation points, concatenated (ambient sizes)
 * Jacobian as fuse's MarginalCostFunction: A_i MinusJacobian(x_i), brought to the tangent space with
 * PlusJacobian(x_i) (= A_i for a unit quaternion).  No loss function.  Its residual rows come after those of all fixed-size factor types, in
 * insertion order.  Blocks it touches are never Schur-eliminated.                                            */
int bsgpu_add_marginal(bsgpu_ctx* ctx, int32_t n_blocks, const int32_t* blocks, int32_t n_rows,
                       const double* A, const double* b, const double* xbar);
/* Replaces A, b and xbar of the index-th prior added with bsgpu_add_marginal (same blocks, same n_rows) IN PLACE: nothing is
 * re-flattened, the device tables of a finalized problem stay.  For priors whose contents change from one solve to the next
 * while the graph does not: [EXT] fuse_core::Graph::removeConstraint + addConstraint of a MarginalConstraint on the same
 * variables.  n_rows x n_cols = the shape of A (b: n_rows), n_xbar = the ambient size of xbar: they must be those of the prior
 * as it was added (BSGPU_ERR_INVALID otherwise — a payload of another shape would be read out of bounds).                     */
int bsgpu_update_marginal(bsgpu_ctx* ctx, int32_t index, int32_t n_rows, int32_t n_cols, int32_t n_xbar, const double* A, const double* b,
                          const double* xbar);

/* ---- solve ----------------------------------------------------------------- */
/* Uploads / builds the device-side structure (sorted factor tables, the tile plan of the
 * reduced system): what [EXT] fuse_core::Graph::optimize does in HashGraph::createProblem
 * before ceres::Solve (bs_optimizers/src/fixed_lag_smoother.cpp:281).  Called implicitly by
 * bsgpu_solve when the problem changed; exposed so a caller can keep it out of a timed region. */
int bsgpu_finalize(bsgpu_ctx* ctx);

/* Levenberg-Marquardt (Ceres TrustRegionMinimizer semantics) on the device.
 * On return the best accepted point is the context's current value set.         */
int bsgpu_solve(bsgpu_ctx* ctx, const bsgpu_options* options, bsgpu_summary* summary);
/* Several windows at once — what the reference does with one thread per optimiser (local smoother, global mapper and the
 * submap refinements side by side: bs_models/src/global_mapping/submap_refinement.cpp:35-115): bsgpu_solve of n DISTINCT
 * contexts.  Windows with eliminated Euclidean landmarks on one device (visual / visual-inertial windows, the reference's
 * local smoother and submap refinements) advance TOGETHER: every kernel of the LM step is launched once for all of them
 * (blockIdx.y = window, per-window argument tables; csrc/bsgpu_batch.cpp), the trust-region decisions are taken per window
 * on the host, converged windows drop out — each window's iterations are those of its lone bsgpu_solve.  Any other window
 * (pose graphs, PCG, inverse-depth landmarks, dense priors, other devices) is driven by a host thread of the library on its
 * context's own stream, in the same call — so is a window whose Jacobi-scaling flag or LM-diagonal bounds differ from the
 * first batched window's.  `options` holds one entry (shared) when options_stride == 0, else n entries; summaries: n
 * entries (device_time_in_seconds of a batched window = the batch's).  Every solve runs to its end; returns BSGPU_OK or the code
 * of the first context (lowest index) that failed — its message is that context's bsgpu_last_error.                      */
int bsgpu_solve_batch(bsgpu_ctx* const* ctxs, int32_t n, const bsgpu_options* options, int32_t options_stride,
                      bsgpu_summary* summaries);
/* Process-wide counters of bsgpu_solve_batch (tests, measurements): windows solved by the batched launches so far, and the
 * rounds (one set of launches each) they took.                                                                            */
int bsgpu_batch_stats(int64_t* windows_batched, int64_t* rounds);

/* Copies the current values back (device -> host), layout of bsgpu_set_blocks.  */
int bsgpu_get_blocks(bsgpu_ctx* ctx, double* values, int64_t n_values);

/* Restores the device-resident values to what bsgpu_set_blocks/set_values last
 * uploaded (device-to-device) — lets a benchmark re-solve the same window
 * without touching PCIe.                                                        */
int bsgpu_reset_values(bsgpu_ctx* ctx);

int bsgpu_num_iterations_recorded(const bsgpu_ctx* ctx);
int bsgpu_get_iteration(const bsgpu_ctx* ctx, int32_t i, bsgpu_iteration* out);
/* linear systems the last bsgpu_solve on `ctx` assembled and solved: every Gauss-Newton / LM
 * attempt, each DOGLEG mu retry included; a DOGLEG step that reuses its Gauss-Newton step after a
 * rejection does not count */
int bsgpu_num_factorizations(const bsgpu_ctx* ctx);

/* ---- evaluation (ceres::Problem::Evaluate) --------------------------------- */
/* Evaluates at the current values with the robust-loss corrector applied.
 * Any output may be NULL.
 *   cost      : 1/2 sum rho(|r|^2)                          (1 double)
 *   residuals : num_residuals doubles, factor order = type-major insertion order
 *   gradient  : num_parameters_tangent doubles (J^T r)
 *   jacobian  : dense row-major num_residuals x num_parameters_tangent (only for
 *               small problems: refuses above 64M entries)                      */
int bsgpu_evaluate(bsgpu_ctx* ctx, double* cost, double* residuals,
                   double* gradient, double* jacobian);
int bsgpu_num_residuals(const bsgpu_ctx* ctx);
int bsgpu_num_parameters_tangent(const bsgpu_ctx* ctx);
/* tangent offset of block b in the reduced problem, -1 for constant blocks */
int bsgpu_tangent_offset(const bsgpu_ctx* ctx, int32_t block);

/* ---- true marginalisation ---------------------------------------------------
 * [EXT] fuse_constraints::marginalizeVariables(source, vars_to_marginalize, graph)
 * (bs_optimizers/src/fixed_lag_smoother.cpp:270-271, `pseudo_marginalization: false`) on the device:
 * every factor that touches one of `marg_blocks` is linearised at the current values, the marginalised blocks are
 * eliminated (Schur complement) and the result is the dense linear prior on the other non-constant blocks those
 * factors touch, in the form bsgpu_add_marginal() takes (A upper-trapezoidal, A^T A = marginal information,
 * A^T b = marginal gradient, xbar = current values of the kept blocks).  Directions of the kept blocks the
 * eliminated factors carry no information about give no row (fuse's QR leaves a zero row there).
 * The caller then removes those factors and the marginalised blocks and adds the prior — the transaction
 * marginalizeVariables returns.  The context itself is not modified.
 *   n_kept / n_rows / n_cols : out — number of kept blocks, rows and columns (sum of tangent sizes) of A     */
int bsgpu_marginalize(bsgpu_ctx* ctx, int32_t n_marg, const int32_t* marg_blocks,
                      int32_t* n_kept, int32_t* n_rows, int32_t* n_cols);
/* Result of the last bsgpu_marginalize: kept_blocks[n_kept] (ascending), A[n_rows*n_cols] row-major (columns in
 * kept_blocks order), b[n_rows], xbar[sum of the kept blocks' sizes].                                       */
int bsgpu_get_marginal(const bsgpu_ctx* ctx, int32_t* kept_blocks, double* A, double* b, double* xbar);

/* ---- covariance (Graph::getCovariance) ------------------------------------- */
/* Marginal covariance block (tangent space) between two pose-side blocks at the
 * current values: out is ts(block_a) x ts(block_b) row-major.                   */
int bsgpu_covariance(bsgpu_ctx* ctx, int32_t block_a, int32_t block_b, double* out);
/* The JOINT marginal covariance of several pose-side blocks (distinct, not constant; their tangent dimensions add up to D <= 64):
 * out is D x D row-major, the blocks' tangent coordinates in the order given.  One undamped assembly + one factorisation, as
 * bsgpu_covariance.  What a submap's summary of itself on its boundary key frames is made of (the unit of independence of
 * bs_models/src/lib/global_mapping/submap_refinement.cpp:35-115; shared-pose consensus, beam_slam_amd/sharding.py).            */
int bsgpu_covariance_joint(bsgpu_ctx* ctx, int32_t n_blocks, const int32_t* blocks, double* out);
/* Graph::getCovariance(requests, matrices): the marginal covariance blocks of n_requests (block_a, block_b) pairs, in tangent space,
 * at the current values, from ONE undamped linearisation.  Any non-constant block: pose-side blocks, Euclidean landmarks (eliminated or
 * not), inverse-depth scalars.  block_pairs[2 * n_requests]; offsets[n_requests + 1] (may be NULL) receives where each ts(a) x ts(b)
 * row-major matrix starts in out; out == NULL: sizes only.  n_requests == 0 is accepted (offsets[0] = 0).
 * Every requested block contributes tangent-size rows (a pose-side block its unit vectors, an eliminated landmark the rows of
 * V_l^-1 W_l); they ride through the factorisation 64 at a time, so k rows take ceil(k / 64) factorisations (blocks are not split
 * between passes).  The factored rows are kept on the device: (rows) x (reduced dimension, padded) doubles, at most 1 GiB.
 * Errors: a bad block index, a constant block, a NULL pair list -> INVALID; a reduced system above the dense limit or kept rows above
 * the budget -> UNSUPPORTED; a singular J^T J -> NUMERIC.                                                                          */
int bsgpu_covariance_requests(bsgpu_ctx* ctx, int32_t n_requests, const int32_t* block_pairs, int64_t* offsets, double* out);

/* ---- factor producers either side of the solve ---------
 * Pixel error |z - projection| of every reprojection factor (types REPROJ then REPROJ_ONLINE_CALIB, insertion
 * order) at the current values, un-weighted and without loss — the screening quantity of
 * bs_models/src/visual_odometry.cpp:1247-1272 (ComputeAverageReprojection).  -1 for a point not in front of the
 * camera.  err: bsgpu_nfactors-sized, i.e. n(REPROJ) + n(REPROJ_ONLINE_CALIB) doubles.                          */
int bsgpu_reprojection_errors(bsgpu_ctx* ctx, double* err);

/* Test hook: the tangent offsets (q block, p block; -1 = constant) the landmark back-substitution reads per reprojection factor
 * (fac_t), and the same pair joined from the two tables it is built from (camera-pose id per factor, offsets per camera pose).
 * Both 2 x (n(REPROJ) + n(REPROJ_ONLINE_CALIB)) int32, insertion order as bsgpu_reprojection_errors; the entries of factors that are
 * not in the landmark tables (a landmark shared with another kind of factor) are left as the caller set them.                      */
int bsgpu_backsub_tangent_table(bsgpu_ctx* ctx, int32_t* fac_t, int32_t* joined);

/* bs_common::PreIntegrator::Integrate (bs_common/src/bs_common/preintegrator.cpp:26-143) for a batch of keyframe
 * intervals on the device: interval i integrates samples [sample_start[i], sample_start[i+1]) (time-ordered,
 * t / gyro w[3] / accel a[3] per sample) up to t_end[i] with the bias estimates bg[3i..], ba[3i..], and the
 * continuous-time noise covariances cov_w, cov_a, cov_bg, cov_ba (3x3 row-major each).  An interval may hold no
 * samples (zero delta, the guards' covariances); n_intervals == 0 does nothing.  sample_start must be non-negative
 * and non-decreasing (else INVALID).
 * consts_out: n_intervals x 287 doubles — the constant payload of BSGPU_F_IMU_DELTA (dt, dq, dp, dv, bias
 * Jacobians, bias linearisation point, A = info_weight * sqrt_inv_cov), ready for bsgpu_add_factors.           */
int bsgpu_preintegrate(int device, int32_t n_intervals, const int32_t* sample_start, const double* t, const double* w,
                       const double* a, const double* t_end, const double* bg, const double* ba, const double* cov_w,
                       const double* cov_a, const double* cov_bg, const double* cov_ba, double info_weight,
                       double* consts_out);

/* Visual-inertial alignment for a batch of candidate paths — what SLAMInitialization does between the up-to-scale camera path and
 * its first large solve: imu::EstimateParameters (bs_models/src/lib/imu/inertial_alignment.cpp:4-202: gyroscope bias, gravity,
 * metric scale, a velocity per frame), the scale gate (bs_models/src/slam_initialization.cpp:312-316) and AlignPathAndVelocities
 * (:400-431).  Path k holds frames [frame_start[k], frame_start[k+1]) (frame_start[0] == 0, non-decreasing; stamps strictly
 * increasing within a path; T_WORLD_BASELINK as q_frame wxyz / p_frame xyz) and the IMU samples [imu_range[2k], imu_range[2k+1]) of
 * t / w / a (as in bsgpu_preintegrate; the arrays hold max(imu_range[2k+1]) samples).  The ranges of different paths may overlap or
 * coincide.  A path's results never depend on the other paths of the call, bit for bit.  n_paths == 0 does nothing.  Argument
 * errors -> INVALID: frame_start[0] != 0 or decreasing, a range with first < 0 or last < first, NULL where an array is needed.
 * Per path, in this order (status: BSGPU_ALIGN_*; TOO_FEW_FRAMES is decided before the samples are looked at):
 * (a) Frames.  Frame f owns the samples of the range with t < t_frame[f] that no earlier frame owns (frame 0: every sample before
 *     the first pose).  BAD_IMU where the reference throws or asserts (:23-30, :50-55, preintegrator.cpp:30): a frame owns no
 *     sample, the range's second sample is later than t_frame[0] (or there is none), sample times not strictly increasing, a delta
 *     of no duration, any non-finite input of the path.  Fewer than 4 frames: TOO_FEW_FRAMES (6 (N - 1) rows for 4 + 3 N unknowns;
 *     ComputePathWithVision asserts more than 3 images).
 * (b) Deltas.  Integrate(t_frame[f], bg, 0, jacobian, no covariance, no information) (preintegrator.cpp:91-115) over the owned
 *     samples: consecutive samples, then the remainder from the last one to the stamp — so the delta of frame f starts at its first
 *     owned sample, up to one IMU period after t_frame[f-1].  bridge_gap == 0 is this, the reference.  bridge_gap != 0 runs one
 *     increment first for f >= 1, from t_frame[f-1] to the first owned sample with the last sample frame f-1 owns (skipped when not
 *     longer than 1e-12 s): the delta then spans exactly [t_frame[f-1], t_frame[f]].
 * (c) Excitation (:114-136), deltas at zero bias: g_f = dv_f / dt_f for all N frames, mean = (sum g_f) / (N - 1) as the reference
 *     divides, excitation = sqrt(sum |g_f - mean|^2 / (N - 1)).  The sum starts from zero; the reference's starts from an
 *     uninitialised Eigen::Vector3d.  excitation < min_excitation (reference: 0.25): NOT_EXCITED.
 * (d) Gyroscope bias (:138-161), over j >= 1: A = sum J^T J, b = sum J^T Log(normalize((q_{j-1} dq_j)^* q_j)), J = dq_dbg_j;
 *     bg = A^+ b through a Jacobi eigen-decomposition of the symmetric 3 x 3, an eigenvalue <= 3 * 2^-52 * lambda_max counting as zero
 *     (Eigen::JacobiSVD's default threshold — recalled, not verified); gyro_rank: the eigenvalues kept.  Log: the rotation vector,
 *     angle in [0, pi] ([EXT] beam::RToLieAlgebra — recalled, not verified), taken from the quaternion.
 * (e) Gravity, scale, velocities (:163-202), deltas re-integrated at (bg, 0): for i = j - 1 and dt, dp, dv of frame j
 *         -1/2 dt^2 g + (p_j - p_i) s - dt v_i = R(q_i) dp_j,      -dt g - v_i + v_j = R(q_i) dv_j
 *     in the least-squares sense by Householder reflections on the unknowns ordered v_0 .. v_{N-1}, g, s (not the normal
 *     equations).  RANK_DEFICIENT when the smallest |diagonal| of that triangular factor is <= rank_tol (1e-10) x the largest — a
 *     path whose positions are all equal has a zero scale column; the reference's fullPivHouseholderQr returns a basic solution
 *     there — or when the gravity estimate has no direction.  Otherwise gravity = normalize(g) * 9.80665, scale = s,
 *     velocity[f] = v_f.
 * (f) Gate and alignment.  apply_scale != 0 and scale outside [scale_min, scale_max] (reference: 0.02, 1.0): SCALE_REJECTED.
 *     Otherwise q_a = FromTwoVectors(gravity, (0, 0, -9.80665)), q_out = q_a q, p_out = q_a p (times scale when apply_scale),
 *     v_out = q_a velocity (never scaled, as in the reference).  FromTwoVectors is Eigen's formula where 1 + cos > 2^-52; for
 *     antiparallel vectors the half turn about the unit vector gravity x e_k, e_k the coordinate axis of gravity's smallest
 *     |component| — not Eigen's SVD branch.
 * Outputs per path: gravity (3), bg (3), scale, excitation, gyro_rank; per frame: velocity (3: the least-squares velocities in the
 * input world), q_out, p_out, v_out.  ba is no output: the reference never estimates it (:14).  What a status leaves: TOO_FEW_FRAMES
 * and BAD_IMU: gravity = bg = 0, scale = 1, excitation = 0, gyro_rank = 0, velocity = v_out = 0, q_out / p_out the inputs.
 * NOT_EXCITED: the same with excitation.  RANK_DEFICIENT: excitation, bg and gyro_rank as estimated, the rest as before.
 * SCALE_REJECTED: every estimate, q_out / p_out the inputs and v_out = velocity.                                                  */
enum { BSGPU_ALIGN_OK = 0, BSGPU_ALIGN_TOO_FEW_FRAMES = 1, BSGPU_ALIGN_BAD_IMU = 2, BSGPU_ALIGN_NOT_EXCITED = 3,
       BSGPU_ALIGN_RANK_DEFICIENT = 4, BSGPU_ALIGN_SCALE_REJECTED = 5 };
int bsgpu_inertial_alignment(int device, int32_t n_paths, const int32_t* frame_start, const double* t_frame, const double* q_frame,
                             const double* p_frame, const int32_t* imu_range, const double* t, const double* w, const double* a,
                             int32_t bridge_gap, double min_excitation, int32_t apply_scale, double scale_min, double scale_max,
                             double rank_tol, double* gravity, double* bg, double* scale, double* excitation, int32_t* gyro_rank,
                             double* velocity, double* q_out, double* p_out, double* v_out, int32_t* status);

/* Point-to-point ICP scan registration for a batch of scan pairs — the matcher_->Match() of MultiScanRegistration::MatchScans
 * (bs_models/src/lib/scan_registration/multi_scan_registration.cpp:451-487; the same call in ScanToMapRegistration, in
 * RelocCandidateSearchScanContext::AlignSubmapsFromScanMatches and in submap_alignment.cpp) in the shipped ICP configuration
 * (config/matchers/icp.json: max_corr 1, max_iter 50, t_eps 1e-8, fit_eps 1e-2, res 0, multiscale_steps 0).  [EXT] libbeam's
 * IcpMatcher and PCL's IterativeClosestPoint are not in the reference checkout: the algorithm below is RECALLED, not verified, and it
 * is computed in FP64 where PCL computes in float.
 * Pair p: the reference cloud S = ref_points[3 ref_start[p] .. 3 ref_start[p+1]) (SetRef, PCL's source) and the target cloud
 * tgt_points[3 tgt_start[p] ..) (SetTarget), both packed xyz; T_init (optional, 12 doubles per pair, row-major 3 x 4:
 * T_LidarRefEst_LidarTgt of :454) is applied to the target on the device first (pcl::transformPointCloud of :462), giving Q; NULL is the
 * identity.  T = I; iteration k = 1 .. max_iter:
 *   correspondences   s_i = T S_i; j(i) the nearest point of Q by squared distance in FP64, ties to the lowest target index; kept iff
 *                     d^2 <= max_corr^2.  Fewer than 3 kept: status TOO_FEW_CORRESPONDENCES, T stays as it was.
 *   step              rigid Kabsch / Umeyama without scale over the kept (s_i, Q_j(i)): centroids, 3 x 3 cross-covariance, the rotation
 *                     from its SVD with the determinant fix (a cross-covariance of rank < 2: no rotation), T <- dT T.
 *   convergence       (PCL's DefaultConvergenceCriteria, recalled) the first that fires: k >= max_iter: MAX_ITERATIONS (counts as
 *                     converged, as in PCL); 1/2 (tr dR - 1) >= rotation_threshold and |dt|^2 <= t_eps: TRANSFORM;
 *                     |mse - mse_prev| < fit_eps: ABS_MSE; |mse - mse_prev| / mse_prev < rel_mse_eps: REL_MSE.  mse: the mean of the kept
 *                     SQUARED distances of this iteration; mse_prev starts at +infinity.
 * The nearest neighbour is found through a dense grid over Q's bounding box with cell edge max_corr; the search is exact.  A pair
 * whose grid would have more than BSGPU_ICP_MAX_CELLS cells, a call whose grids together would have more than 16 times as many, or
 * max_iter > BSGPU_ICP_MAX_ITER: UNSUPPORTED.  The sums over the correspondences have a fixed order (chunks of source points), so a
 * pair's results never depend on the other pairs of the call, bit for bit.
 * Outputs per pair: T_refest_ref (12: the matcher's result, maps S onto Q: T_RefEst_Ref of :474); T_ref_tgt (optional, 12:
 * inv(T_refest_ref) T_init, :475 T_LIDARREF_LIDARTGT); mse, n_corr (optional: of the last iteration; mse 0 when nothing was kept);
 * n_iters (optional: steps applied); status (BSGPU_ICP_*; converged unless TOO_FEW_CORRESPONDENCES).  n_pairs == 0 does nothing; an
 * empty cloud gives TOO_FEW_CORRESPONDENCES.  INVALID: NULL where an array is needed, a start table that does not begin at 0 or
 * decreases, a non-finite point or T_init entry, max_corr not positive and finite, max_iter < 1, a negative or NaN tolerance.
 * Nothing is written unless the call succeeds; bsgpu_register_scans_error says what this thread's last failed call objected to.  */
enum { BSGPU_ICP_MAX_ITERATIONS = 1, BSGPU_ICP_TRANSFORM = 2, BSGPU_ICP_ABS_MSE = 3, BSGPU_ICP_REL_MSE = 4,
       BSGPU_ICP_TOO_FEW_CORRESPONDENCES = 5 };
#define BSGPU_ICP_MAX_CELLS (1 << 22)
#define BSGPU_ICP_MAX_ITER 1000
int bsgpu_register_scans(int device, int32_t n_pairs, const int32_t* ref_start, const double* ref_points, const int32_t* tgt_start,
                         const double* tgt_points, const double* T_init, double max_corr, int32_t max_iter, double t_eps,
                         double fit_eps, double rotation_threshold, double rel_mse_eps, double* T_refest_ref, double* T_ref_tgt,
                         double* mse, int32_t* n_corr, int32_t* n_iters, int32_t* status);
const char* bsgpu_register_scans_error(void);

/* Generalized ICP for a batch of scan pairs — the matcher_->Match() of RelocCandidateSearchScanContext::AlignSubmapsFromScanMatches
 * (bs_models/src/lib/reloc/reloc_candidate_search_scan_context.cpp:210-262; the same GicpMatcher in submap_alignment.cpp:52,
 * global_map_batch_optimization.cpp:48, scan_registration_base.cpp:88 and RelocRefinementScanRegistration<GicpMatcher>) in the shipped
 * GICP configuration (config/matchers/gicp.json: corr_rand 10, max_iter 100, r_eps 1e-8, fit_eps 1e-2, res 0.1).  [EXT] libbeam's
 * GicpMatcher and PCL's GeneralizedIterativeClosestPoint are not in the reference checkout: what is taken from them below (the
 * covariances, the correspondence rule, the objective, the outer criterion, the constructor's defaults) is RECALLED, not verified, and
 * everything is computed in FP64.  PCL's GICP loop does not read fit_eps (recalled), so it is no parameter.  res, the matcher's voxel
 * downsampling, is the caller's job: the clouds are registered as they are passed (bsgpu_build_registration_maps is the library's
 * voxel filter).
 * Clouds and roles as in bsgpu_register_scans: S the reference cloud (SetRef, PCL's source), Q the target cloud after T_init (optional,
 * 12 doubles per pair, row-major 3 x 4; NULL: the identity) has been applied to it on the device.
 *   covariances       (PCL's computeCovariances) once per cloud per call.  For a point p of a cloud P, |P| >= k_neighbors = k: its k
 *                     nearest points of P, itself included, in ascending (d^2, index) order; mu their mean; C = (1/k) sum (x - mu)
 *                     (x - mu)^T (PCL: E[x x^T] - mu mu^T; the centred form is the library's choice); its eigen-decomposition with
 *                     eigenvalues in falling order; C' = u1 u1^T + u2 u2^T + gicp_epsilon u3 u3^T.  The target's are those of Q.
 *                     ref_cov, tgt_cov (optional): C' as 6 doubles per point (xx, xy, xz, yy, yz, zz); zeros for a pair that has a
 *                     cloud of fewer than k points.
 *   outer iteration   k = 1 .. max_iter from T = I.  Per source point s = T S_i, j(i) the nearest point of Q by (d^2, index), kept iff
 *                     d^2 < max_corr^2 (strict, as recalled from PCL's nn_dists[0] < dist_threshold); M_i = (C'^Q_j + R C'^S_i R^T)^-1
 *                     with R from T at the start of this outer iteration.  Fewer than 4 kept: TOO_FEW_CORRESPONDENCES, T stays.
 *   inner loop        at most max_inner steps that minimise F(T) = sum r_i^T M_i r_i, r_i = T S_i - q_j(i), correspondences and M_i
 *                     fixed: plain Gauss-Newton with a left update, J = [-[s]x | I], H = sum J^T M J, g = sum J^T M r, xi = -H^-1 g by
 *                     a 6 x 6 Cholesky, T <- [exp(w) | v] T with Rodrigues' formula for w.  It stops after the step whose
 *                     max |xi| < inner_eps.  A pivot <= 1e-12 x that diagonal entry of H ends the pair with BSGPU_GICP_DEGENERATE, T as it
 *                     was before this outer iteration.  PCL minimises the same objective with BFGS over (x, y, z, roll, pitch, yaw): its
 *                     iterates are NOT reproduced; the objective, the correspondences, the covariances and the outer criterion are.
 *   outer criterion   (PCL's delta rule, recalled) with T0 the transform before this outer iteration,
 *                     delta = max(max_kl |R - R0|_kl / r_eps, max_k |t - t0|_k / t_eps): k >= max_iter: MAX_ITERATIONS (counts as converged,
 *                     checked first, as in ICP); otherwise delta < 1: TRANSFORM.
 * A cloud of fewer than k_neighbors points, an empty one included: TOO_FEW_CORRESPONDENCES with T = I and n_iters = 0 (PCL refuses such
 * a cloud, recalled).
 * Both neighbour queries — the k nearest of a cloud in itself, no radius, and the nearest target below max_corr — are exact, ties
 * decided by (d^2, index): a dense grid of cell edge grid_cell over each cloud's bounding box (one for S, used by its covariances
 * only, and one for Q) is searched in shells of cells around the query's cell until nothing that has not been searched can matter.
 * grid_cell is a performance knob only: no result, covariances included, depends on it, bit for bit.  The sums have a fixed order, so
 * a pair's results never depend on the other pairs of the call, bit for bit.
 * Outputs per pair: T_refest_ref (12); T_ref_tgt (optional, 12: inv(T_refest_ref) T_init); cost (optional: F / n_corr of the last pass
 * over the correspondences; 0 when there was none); n_corr (optional: kept in the last outer iteration); n_iters (optional: outer
 * iterations applied); n_inner (optional: Gauss-Newton steps in total); status (BSGPU_GICP_*; converged iff MAX_ITERATIONS or
 * TRANSFORM).  n_pairs == 0 does nothing.
 * UNSUPPORTED: k_neighbors > BSGPU_GICP_MAX_K; a grid of more than BSGPU_ICP_MAX_CELLS cells; grids that together hold more than 16 times
 * as many; max_iter > BSGPU_ICP_MAX_ITER; max_inner > BSGPU_GICP_MAX_INNER.  INVALID: what bsgpu_register_scans refuses, and k_neighbors
 * < 1, max_inner < 1, gicp_epsilon outside (0, 1], grid_cell not positive and finite, a negative or NaN r_eps, t_eps or inner_eps.
 * Nothing is written unless the call succeeds; bsgpu_register_scans_error says what this thread's last failed call objected to.  */
enum { BSGPU_GICP_MAX_ITERATIONS = 1, BSGPU_GICP_TRANSFORM = 2, BSGPU_GICP_TOO_FEW_CORRESPONDENCES = 5, BSGPU_GICP_DEGENERATE = 6 };
#define BSGPU_GICP_MAX_K 32
#define BSGPU_GICP_MAX_INNER 64
int bsgpu_register_scans_gicp(int device, int32_t n_pairs, const int32_t* ref_start, const double* ref_points, const int32_t* tgt_start,
                              const double* tgt_points, const double* T_init, int32_t k_neighbors, double gicp_epsilon, double max_corr,
                              int32_t max_iter, double r_eps, double t_eps, int32_t max_inner, double inner_eps, double grid_cell,
                              double* T_refest_ref, double* T_ref_tgt, double* cost, int32_t* n_corr, int32_t* n_iters, int32_t* n_inner,
                              int32_t* status, double* ref_cov, double* tgt_cov);

/* LOAM feature registration for a batch of scan pairs — the matcher_->Match() of MultiScanLoamRegistration::MatchScans
 * (bs_models/src/lib/scan_registration/multi_scan_registration.cpp:497-531), ScanToMapLoamRegistration (scan_to_map_registration.cpp:
 * 158-188), RelocRefinementLoamRegistration (reloc_refinement_loam_registration.cpp:91-118), submap_alignment.cpp:76-96 and
 * global_map_batch_optimization.cpp:238-247 in the shipped configuration (config/matchers/loam_*.json, optimization/ceres_config.json).
 * The matcher's boundary is kept: LoamPointCloud in, transform and covariance out; feature extraction (LoamFeatureExtractor) is a
 * separate step: bsgpu_extract_loam_features, below; the scan-to-map reference clouds (RegistrationMap::GetLoamCloudMap) come from
 * bsgpu_build_registration_maps, further below.  [EXT] libbeam's LoamMatcher, LoamScanRegistration, CeresPointToLineCostFunction and
 * CeresPointToPlaneCostFunction are not in the reference checkout: everything below is RECALLED, not verified, and where the text says
 * "the library's choice" this library decides something the recollection leaves open.
 *   clouds            pair p has four packed-xyz clouds, start tables as in bsgpu_register_scans: the reference's edge and surface
 *                     features and the target's.  They are the STRONG features of a LoamPointCloud (edges.strong, surfaces.strong):
 *                     every shipped matcher file sets ignore_weak_features and check_strong_features_first.  NOT MODELLED: weak
 *                     features as a second search tier, validate_correspondences, the matcher's max_solver_time_in_seconds.  A caller
 *                     who wants weak features matched passes them concatenated to the strong ones.  T_init (optional, 12 doubles per
 *                     pair, row-major 3 x 4; NULL: the identity) is applied to the target features on the device first.
 *   roles             the reverse of ICP: the reference clouds are searched, the target features are the queries, and it is the target
 *                     that moves.  The estimate is T = T_REF_TGT, starting at the identity.
 *   outer iteration   k = 1 .. max_outer (max_correspondence_iterations; iterate_correspondences false is max_outer = 1).  For each
 *                     target edge e, x = T e and its 2 nearest reference edge points a, b by (d^2, index): kept iff the cloud has 2
 *                     points, the farther has d^2 < max_corr^2 and a != b as points.  For each target surface point the same with its
 *                     3 nearest reference surface points a, b, c: kept iff all three lie below the threshold and n = (b - a) x (c - a),
 *                     as computed, is not the zero vector.  The strict threshold and the treatment of exact degeneracy only are the
 *                     library's choices.  A measurement stores the target point before T.  n_edge + n_surf < min_measurements:
 *                     TOO_FEW_MEASUREMENTS, T as it was before this outer iteration (the reference's Match() returns false).
 *   inner solve       Ceres' Levenberg-Marquardt, as bsgpu_localize_frames restates it for one pose (Jacobi scaling, clamped
 *                     diagonal, the rho test, the radius update, the three tolerances over the ambient (q, p)), from the current T with
 *                     the fields of *inner that bsgpu_localize_frames reads; trust_region_strategy_type must be LM.  The pose is
 *                     (q, p) with x = R(q) e + p, tangent [p, theta], q <- q (x) exp(theta), the exponential from its series (no
 *                     library sine).  One scalar residual per measurement: edge r = |(x - a) x (x - b)| / |a - b|, surface
 *                     r = n . (x - a) / |n|; loss rho(r^2) with loss_kind TRIVIAL or HUBER(loss_a) (shipped: ceres_config.json HUBER,
 *                     scaling 1, 50 iterations, tolerances 1e-8 / 1e-10 / 1e-8).  An edge residual that is exactly 0 has a zero Jacobian
 *                     row (the library's choice: automatic differentiation of the square root at 0 has none).  An unusable inner solve:
 *                     SOLVER_FAILED, T as before this outer iteration.
 *   outer criterion   in this order: k >= max_outer: MAX_ITERATIONS (a success, as in the reference); otherwise with
 *                     D = inv(T_before) T: |D.t| < conv_translation_m and the rotation angle of D < conv_rotation_deg (both): TRANSFORM.
 *                     The angle test compares (tr D.R - 1) / 2 with the cosine of the threshold, which the host takes once; the device
 *                     calls no acos, atan, sin, cos or log.  (A threshold of 0 is never met.)
 * Outputs per pair: T_refest_ref (12) = inv(T), what matcher_->GetResult() is (multi_scan_registration.cpp:522); T_ref_tgt (optional, 12)
 * = T T_init (:523-524); cov (optional, 36): the last inner solve's (J^T J)^-1 at its final pose, J loss-corrected, tangent order
 * [p, theta], standing for matcher_->GetCovariance() (:528) — NaN unless the status is a success, and NaN for a singular J^T J; cost
 * (optional): the last inner solve's final cost; n_edge, n_surf (optional): kept in the last outer iteration; n_iters (optional): outer
 * iterations applied; n_inner (optional): LM iterations in total; status (BSGPU_LOAM_*; converged iff MAX_ITERATIONS or TRANSFORM).
 * n_pairs == 0 does nothing; empty clouds give TOO_FEW_MEASUREMENTS with T = I.
 * Both searches are exact (a dense grid of cell edge grid_cell over each reference cloud, searched in shells): grid_cell is a performance
 * knob that no bit depends on.  Every sum over measurements has a fixed order (the target features, edges then surfaces, in chunks), so
 * a pair's bits depend neither on its neighbours in the call nor on grid_cell.  A pair is one workgroup: a pair far above a local map's
 * few thousand features runs on one compute unit, serially over rounds of features.
 * INVALID: everything bsgpu_register_scans refuses (per table: ref_edge_start, ref_surf_start, tgt_edge_start, tgt_surf_start), and
 * min_measurements < 1, max_outer < 1, a negative or NaN conv_translation_m or conv_rotation_deg, conv_rotation_deg >= 180, grid_cell not
 * positive and finite, an unknown loss_kind, loss_a not positive and finite for HUBER, inner == NULL.  UNSUPPORTED: the grid caps of
 * bsgpu_register_scans_gicp; max_outer > BSGPU_LOAM_MAX_OUTER; inner->max_num_iterations > BSGPU_LOAM_MAX_INNER; more than
 * BSGPU_LOAM_MAX_FEATURES target features in one pair (a pair is one workgroup: the cap bounds a launch's length); BSGPU_LOSS_CAUCHY (its
 * logarithm is not the same function on host and device); a trust-region strategy other than LM.
 * Nothing is written unless the call succeeds; bsgpu_register_scans_error says what this thread's last failed call objected to,
 * prefixed "register_scans_loam: ".  */
enum { BSGPU_LOAM_MAX_ITERATIONS = 1, BSGPU_LOAM_TRANSFORM = 2, BSGPU_LOAM_TOO_FEW_MEASUREMENTS = 5, BSGPU_LOAM_SOLVER_FAILED = 6 };
#define BSGPU_LOAM_MAX_OUTER 100
#define BSGPU_LOAM_MAX_INNER 1000
#define BSGPU_LOAM_MAX_FEATURES 65536
int bsgpu_register_scans_loam(int device, int32_t n_pairs, const int32_t* ref_edge_start, const double* ref_edges, const int32_t* ref_surf_start,
                              const double* ref_surfs, const int32_t* tgt_edge_start, const double* tgt_edges, const int32_t* tgt_surf_start,
                              const double* tgt_surfs, const double* T_init, double max_corr, int32_t min_measurements, int32_t max_outer,
                              double conv_translation_m, double conv_rotation_deg, const bsgpu_options* inner, int32_t loss_kind, double loss_a,
                              double grid_cell, double* T_refest_ref, double* T_ref_tgt, double* cov, double* cost, int32_t* n_edge,
                              int32_t* n_surf, int32_t* n_iters, int32_t* n_inner, int32_t* status);

/* LOAM feature extraction for a batch of scans — the feature_extractor->ExtractFeatures(cloud) that every lidar scan goes through
 * before a matcher sees it (bs_models/src/lib/lidar/scan_pose.cpp:34-37, 63-66, 92-95), in the shipped configuration
 * (config/matchers/loam_*.json).  A raw revolution in, the four clouds of a LoamPointCloud out, the strong ones in exactly the layout
 * bsgpu_register_scans_loam takes.  [EXT] libbeam's LoamFeatureExtractor is not in the reference checkout, only its call sites and its
 * parameter files are: everything below is RECALLED from it and from the LOAM scan registration it derives from, not verified, and
 * where the text says "the library's choice" this library decides something the recollection leaves open.  Arithmetic is FP64 (the
 * original bins float points); every squared length is (x^2 + y^2) + z^2, no product is fused.
 *   scans             scan s is points[3 scan_start[s] .. 3 scan_start[s+1]), packed xyz, start table as in bsgpu_register_scans; ring
 *                     (optional) one int32 per point.
 *   validity          a point is dropped if a coordinate is not finite or |p|^2 < 1e-4.
 *   ring              with ring given: that value, dropped outside [0, number_of_beams).  With ring == NULL, from the elevation: v the
 *                     coordinate along vertical_axis (BSGPU_AXIS_*), h the root of the other two squared, the angle in degrees,
 *                     t = (angle + fov_deg / 2) (beams - 1) / fov_deg + 0.5, the ring trunc(t), dropped outside [0, beams).  The device
 *                     decides this by comparisons only: the host takes the tangents of the beams + 1 boundary angles (t = -1, 1, 2 ..
 *                     beams) once per call and a point is compared as v against tan(beta) h (a boundary at or beyond +-90 degrees is
 *                     infinite).  This form is the library's choice; no atan runs on the device.  A point within rounding of a
 *                     boundary may therefore fall to the other side than an atan would put it.
 *   ring order        a ring's points keep their order of arrival in the scan (a stable partition).  A ring of n points with
 *                     n - 1 <= 2 c, c = curvature_region, is skipped whole.
 *   unreliable        for i in [c, n - 1 - c), dn = |p_{i+1} - p_i|^2, dp = |p_i - p_{i-1}|^2: if dn > 0.1, with r1 = |p_i|,
 *                     r2 = |p_{i+1}|: r1 > r2 and |p_{i+1} - p_i (r2 / r1)| / r2 < 0.1 marks i - c .. i as picked; r1 <= r2 and
 *                     |p_{i+1} (r1 / r2) - p_i| / r1 < 0.1 marks i + 1 .. i + c + 1.  If dn > 0.0002 |p_i|^2 and dp > 0.0002 |p_i|^2, i
 *                     is marked.
 *   curvature         for i in [c, n - c): s = -2 c p_i, then for j = 1 .. c in that order s += p_{i+j}, s += p_{i-j}; the curvature is
 *                     |s|^2.
 *   regions           L = n - 1 - 2 c, G = n_feature_regions; region j covers sp = c + (L j) / G .. ep = c + (L (j + 1)) / G - 1 in
 *                     integer division; a region with ep <= sp is skipped.  The regions of a ring are processed in order, because a
 *                     pick marks neighbours across a region's border.
 *   picks             the total order is the key (curvature, position in the ring); that ties go by position is the library's choice
 *                     (the original's sort leaves them open).  Edges: from the largest key down, until max_corner_less_sharp are taken
 *                     or the region is exhausted; a point is taken iff it is not picked and its curvature >
 *                     surface_curvature_threshold; the first max_corner_sharp taken are SHARP, the rest LESS_SHARP.  Surfaces: from the
 *                     smallest key up, until max_surface_flat are taken; taken iff not picked and curvature < the threshold: FLAT.  A
 *                     taken point is marked as picked: itself, then i + k for k = 1 .. c, stopping at the ring's end or when
 *                     |p_{i+k} - p_{i+k-1}|^2 > 0.05, and the same backwards.  Every other point of a processed region is LESS_FLAT.
 * Outputs, packed with start tables of n_scans + 1 entries, within a scan by ring, then region, then pick order: the STRONG edges
 * (SHARP: edge_start, edge_index — the point's index within its scan —, edge_points, optional: packed xyz, the input's bits) and the
 * STRONG surfaces (FLAT: surf_*), which are the edges / surfs arrays of bsgpu_register_scans_loam.  Optional as a group (all six NULL,
 * or both start tables and both index arrays given): the WEAK clouds LESS_SHARP (weak_edge_*) and LESS_FLAT (weak_surf_*, by ring and
 * position).  They are disjoint from the strong ones — a caller who wants the original's supersets concatenates; the library's choice.
 * label (optional, per input point): BSGPU_LOAM_DROPPED for a point that is invalid, without a ring, in a skipped ring or outside every
 * processed region, else its class.  curvature (optional, per input point): NaN where none is defined.
 * Capacities per scan, which the caller provides: strong edges beams G min(max_corner_sharp, max_corner_less_sharp), weak edges
 * beams G max(max_corner_less_sharp - max_corner_sharp, 0), strong surfaces beams G max_surface_flat, weak surfaces the scan's points
 * (none of them more than the scan's points).
 * n_scans == 0 does nothing; an empty scan gives empty clouds; a scan's outputs depend on nothing else in the call, and no output
 * depends on how the device schedules its lanes.  One workgroup per (scan, ring): a lone revolution uses as many compute units as it
 * has rings.
 * OUT OF SCOPE: the voxel filter of the weak surfaces (downsample_less_flat_features must be 0), deskewing, intensity and time fields,
 * and keeping the features on the device for the matcher: the two calls are chained through host arrays.  The map of the registered
 * scans' features that a scan-to-map matcher reads is bsgpu_build_registration_maps, below.
 * INVALID: NULL where an array is needed, a weak group given in part, everything bsgpu_register_scans refuses of a start table,
 * number_of_beams, n_feature_regions or curvature_region < 1, a negative count, fov_deg not in (0, 180), a threshold that is not
 * finite, an unknown vertical_axis.  UNSUPPORTED: number_of_beams > BSGPU_LOAM_MAX_RINGS, a ring of more than
 * BSGPU_LOAM_MAX_RING_POINTS points, curvature_region > BSGPU_LOAM_MAX_CURVATURE_REGION, n_feature_regions > BSGPU_LOAM_MAX_REGIONS,
 * downsample_less_flat_features != 0.  Nothing is written unless the call succeeds; bsgpu_register_scans_error says what this
 * thread's last failed call objected to, prefixed "extract_loam_features: ".  */
enum { BSGPU_LOAM_DROPPED = -1, BSGPU_LOAM_LESS_FLAT = 0, BSGPU_LOAM_FLAT = 1, BSGPU_LOAM_LESS_SHARP = 2, BSGPU_LOAM_SHARP = 3 };
enum { BSGPU_AXIS_X = 0, BSGPU_AXIS_Y = 1, BSGPU_AXIS_Z = 2 };
#define BSGPU_LOAM_MAX_RINGS 128
#define BSGPU_LOAM_MAX_RING_POINTS 4096
#define BSGPU_LOAM_MAX_CURVATURE_REGION 16
#define BSGPU_LOAM_MAX_REGIONS 64
int bsgpu_extract_loam_features(int device, int32_t n_scans, const int32_t* scan_start, const double* points, const int32_t* ring,
                                int32_t number_of_beams, double fov_deg, int32_t vertical_axis, int32_t n_feature_regions,
                                int32_t curvature_region, int32_t max_corner_sharp, int32_t max_corner_less_sharp, int32_t max_surface_flat,
                                double surface_curvature_threshold, int32_t downsample_less_flat_features, int32_t* edge_start,
                                int32_t* edge_index, double* edge_points, int32_t* surf_start, int32_t* surf_index, double* surf_points,
                                int32_t* weak_edge_start, int32_t* weak_edge_index, double* weak_edge_points, int32_t* weak_surf_start,
                                int32_t* weak_surf_index, double* weak_surf_points, int32_t* label, double* curvature);

/* Registration maps for a batch of maps — the reference clouds of scan-to-map registration: RegistrationMap::GetLoamCloudMap and
 * GetPointCloudMap (bs_models/src/lib/scan_registration/registration_map.cpp:96-135), which ScanToMapLoamRegistration::RegisterScanToMap
 * (scan_to_map_registration.cpp:168-197) rebuilds for every incoming scan from the last map_size registered scans (registration/
 * scan_to_map.json: 45 scans, leaf 0.1 m), and the aggregates that Scan Context and GICP take (reloc_candidate_search_scan_context.cpp:
 * 225-230, global_mapping/utils.cpp:27-43).  One primitive: transform, merge, voxel-reduce.  A "map" is ONE cloud class of one map: the
 * LOAM map is two maps in one call (the scans' edge clouds, then their surface clouds), GetPointCloudMap is one, a batch of
 * loop-closure aggregates one each.  [EXT] libbeam's VoxelDownsample and pcl::VoxelGrid are not in the reference checkout: everything
 * below is RECALLED, not verified, and where the text says "the library's choice" this library decides something the recollection
 * leaves open.  Arithmetic is FP64.
 *   maps              map m owns scans [map_scan_start[m], map_scan_start[m+1]); scan s is points[3 scan_start[s] .. 3 scan_start[s+1]),
 *                     packed xyz in its own (lidar) frame; the call has map_scan_start[n_maps] scans.  Start tables as in
 *                     bsgpu_register_scans.
 *   transform         every point goes through its scan's T_map_scan (12 doubles, row-major 3 x 4) by the fused multiply-adds of the
 *                     scan registrations (point_grid.h: grid_apply).  T_map_scan == NULL: the identity, the points are taken as they are.
 *   voxel             of a transformed point q: (floor(q.x / v), floor(q.y / v), floor(q.z / v)), v = voxel_size; the grid is anchored
 *                     at the origin, as pcl::VoxelGrid anchors it.  A point exactly on a boundary belongs to the upper cell; negative
 *                     coordinates floor, they do not truncate.
 *   output            one point per occupied voxel: the sum of the voxel's transformed points IN INPUT ORDER (scan order, then point
 *                     order), taken sequentially in FP64 from +0.0, divided by their number.
 *   order             within a map ascending (iz, iy, ix): PCL's order of idx = ix' + iy' dx + iz' dx dy, whatever the bounding box.
 *   non-finite        a point with a transformed coordinate that is not finite is dropped when voxel_size > 0.
 *   merge only        voxel_size == -1 (the reference's sentinel): every transformed point is copied in input order, map_count is 1.
 *   stateless         a scan is passed in its own frame with its current T_Map_Scan on every call: the library's choice.  The reference
 *                     stores transformed float clouds and, in UpdateScan, re-transforms them incrementally.
 *   NOT MODELLED      min_points_per_voxel, PCL's float accumulation and inverse_leaf multiply, and libbeam's splitting of a cloud whose
 *                     PCL index would overflow an int (the 63-bit key here — 21 biased bits per axis, iz most significant — has no such
 *                     overflow).
 * Outputs: map_start (n_maps + 1) and map_points (packed xyz; capacity 3 x the call's points) are exactly the layout
 * bsgpu_register_scans_loam takes for ref_edge_start / ref_edges and ref_surf_start / ref_surfs, and bsgpu_register_scans_gicp for its
 * clouds.  map_count (optional, capacity the call's points): input points per output point.
 * n_maps == 0 does nothing; a map without points gives an empty range.  A map's bytes depend neither on its neighbours in the call nor
 * on how the device schedules its lanes: the device sorts (key, index) with a stable radix sort inside each map and sums a voxel's run
 * sequentially; there are no floating-point atomics.
 * INVALID: NULL map_scan_start, scan_start, map_start or map_points, NULL points where a scan has some, everything
 * bsgpu_register_scans refuses of a start table (either one), voxel_size neither -1 nor positive and finite, a non-finite entry of
 * T_map_scan.  UNSUPPORTED: more than BSGPU_MAP_MAX_POINTS points in the call; a finite transformed coordinate with
 * |q / voxel_size| >= 2^20 (the device reports it through a flag that is only ever set to 1).  Nothing is written unless the call
 * succeeds; bsgpu_register_scans_error says what this thread's last failed call objected to, prefixed "build_registration_maps: ".  */
#define BSGPU_MAP_MAX_POINTS 8388608
#define BSGPU_MAP_SORT_TILE 1024      /* keys per workgroup of the device's sort; no output depends on it */
int bsgpu_build_registration_maps(int device, int32_t n_maps, const int32_t* map_scan_start, const int32_t* scan_start, const double* points,
                                  const double* T_map_scan, double voxel_size, int32_t* map_start, double* map_points, int32_t* map_count);

/* Scan Context place recognition — the descriptors and the search of RelocCandidateSearchScanContext::FindRelocCandidates
 * (bs_models/src/lib/reloc/reloc_candidate_search_scan_context.cpp:117-150): the step that decides which scan pairs
 * AlignSubmapsFromScanMatches (:210-262) hands to the matcher (bsgpu_register_scans).  Two stateless calls, so that a caller can keep
 * descriptors per keyframe as SCManager does.  [EXT] SCManager is libbeam's copy of the published Scan Context code (Kim & Kim, IROS
 * 2018) and is not in the reference checkout: everything below is RECALLED, not verified, and it is computed in FP64 where the
 * original bins float points.  BSGPU_SC_RINGS and BSGPU_SC_SECTORS are compile-time constants (the original's PC_NUM_RING, PC_NUM_SECTOR).
 *
 * bsgpu_scan_context_describe (makeScancontext, makeRingkeyFromScancontext, makeSectorkeyFromScancontext; AggregateSubmapScan :264-290).
 * Scan k is points[3 scan_start[k] .. 3 scan_start[k+1]), packed xyz in the lidar frame.  Aggregate a is the union of its members
 * [member_start[a], member_start[a+1]); member m is scan member_scan[m] (a scan may serve many members) through member_T[m] (12 doubles,
 * row-major 3 x 4: T_ScanCenter_ScanToAgg of :280; member_T NULL: every member the identity).  T p is ((T0 x + T1 y) + T2 z) + T3 per
 * row, no product fused.  For a transformed point (x, y, z): r = sqrt(x^2 + y^2); the point is dropped if r > max_radius (or if the
 * transform took r or z out of the finite range); ring = clamp(ceil(r / max_radius * 20), 1, 20) - 1; sector = k for an azimuth
 * (counter-clockwise from +x) in (6 k, 6 (k + 1)] degrees, azimuth 0 and r == 0 going to sector 0.  The sector is decided by
 * comparisons of |y| against tan(6 m degrees) |x| (and the reverse above 45 degrees), never by atan: at a boundary the decision of
 * sc_sector (csrc/scan_context.h) is the contract.  A bin's value is the maximum of z + lidar_height over its points; a bin without a
 * point is 0.  NOT MODELLED: the original marks empty bins with -1000 and so also zeroes a bin whose maximum is exactly -1000.
 * desc: 20 x 60 per aggregate, ring-major; ring_key (optional, 20): the mean of each row; sector_key (optional, 60): the mean of each
 * column; n_binned (optional): the number of points kept.  An aggregate with no member or no point inside the radius is all zeros.
 * n_aggregates == 0 does nothing.  INVALID: NULL where an array is needed, a start table that does not begin at 0 or decreases, a
 * member index out of range, a non-finite point or transform entry, max_radius not positive and finite, a non-finite lidar_height.
 * UNSUPPORTED: a scan of more than BSGPU_SC_MAX_SCAN_POINTS points.
 *
 * bsgpu_scan_context_match (detectLoopClosureID :141, distanceBtnScanContext, fastAlignUsingVkey, distDirectSC).  Set s is one
 * SCManager of :120-132: queries [query_start[s], query_start[s+1]) of query_desc against candidates [cand_start[s], ..) of cand_desc
 * (20 x 60 each, as describe writes them; keys and column norms are recomputed from them).  For a query q and a candidate c:
 *   alignment     shift0 = the s in 0 .. 59 that minimises |sector_key(q) - circshift(sector_key(c), s)| (compared as squared norms),
 *                 the first minimum winning; circshift moves column i to column (i + s) mod 60.
 *   refinement    the shifts shift0 +- 0 .. R modulo 60 in ascending order, R = round(0.5 search_ratio 60) (3 at the shipped 0.1;
 *                 R >= 30: all 60).  Per shift d = 1 - (1/n) sum_j cos(col_j(q), col_j(shifted c)) over the n columns that are non-zero
 *                 on both sides; the first minimum wins.  A shift with n == 0 has distance +infinity (the library's choice: the
 *                 original divides by zero).  Wherever values are compared (alignment norms, shift distances, ring-key
 *                 distances) a NaN, which finite entries near the ends of the FP64 range can make, counts as +infinity.
 *   pre-selection n_tree_candidates = K > 0: only the K candidates of the set nearest in squared ring-key distance are compared, ties
 *                 to the lowest index (the k-d tree's NUM_CANDIDATES_FROM_TREE = 10 nearest of the original, done exactly).  K <= 0 or
 *                 K at or above the set's size: all of them.
 * Per query: the compared candidate of least (distance, index): best_cand (its index inside its set; -1 when that distance is not
 * < dist_thres or the set has no candidate), best_dist and best_shift (still those of the best compared candidate; +infinity and 0
 * when there is none), yaw (optional) = best_shift 2 pi / 60.  dist_all / shift_all (optional): every (query, candidate of its set)
 * entry, queries in order and a query's candidates in order; +infinity and 0 for candidates that the pre-selection left out.
 * NOT MODELLED: NUM_EXCLUDE_RECENT (the reference passes 0 and a caller chooses its candidate range) and the tree-rebuild period.
 * The 60-term sums (means, key norms, the sum of cosines) have one fixed tree and the 20-term sums one fixed chain
 * (csrc/scan_context.h), so an item's results never depend on the other items of the call, bit for bit.
 * INVALID: NULL where an array is needed, bad start tables, non-finite descriptor entries, a negative or NaN search_ratio or
 * dist_thres.  UNSUPPORTED: more than BSGPU_SC_MAX_CANDIDATES candidates in a set, K > BSGPU_SC_MAX_TREE_CANDIDATES.
 * Both: nothing is written unless the call succeeds; bsgpu_scan_context_error says what this thread's last failed call objected to.  */
#define BSGPU_SC_RINGS 20
#define BSGPU_SC_SECTORS 60
#define BSGPU_SC_MAX_CANDIDATES 65536
#define BSGPU_SC_MAX_TREE_CANDIDATES 64
#define BSGPU_SC_MAX_SCAN_POINTS (65535 * 4096)
int bsgpu_scan_context_describe(int device, int32_t n_scans, const int32_t* scan_start, const double* points, int32_t n_aggregates,
                                const int32_t* member_start, const int32_t* member_scan, const double* member_T, double lidar_height,
                                double max_radius, double* desc, double* ring_key, double* sector_key, int32_t* n_binned);
int bsgpu_scan_context_match(int device, int32_t n_sets, const int32_t* query_start, const double* query_desc, const int32_t* cand_start,
                             const double* cand_desc, int32_t n_tree_candidates, double search_ratio, double dist_thres,
                             int32_t* best_cand, double* best_dist, int32_t* best_shift, double* yaw, double* dist_all,
                             int32_t* shift_all);
const char* bsgpu_scan_context_error(void);

/* Landmark triangulation for a batch of feature tracks at the context's CURRENT values (after a solve: the values the
 * solve left on the device) — VisualOdometry::TriangulateLandmark (bs_models/src/visual_odometry.cpp:532-610) and
 * SLAMInitialization::TriangulateLandmark (bs_models/src/slam_initialization.cpp:699-701), i.e. the [EXT]
 * beam_cv::Triangulation::TriangulatePoint(cam, T_cam_world, pixels, max_dist, max_reprojection) call they make.
 * Track i holds views [track_start[i], track_start[i+1]); view o is seen from the keyframe whose orientation /
 * position blocks are q_block[o] / p_block[o] with the measured pixel pixels[2o..2o+1]; `camera` indexes the
 * bsgpu_set_cameras table (K and T_cam_baselink).  truncate_pixels != 0 reproduces the reference's
 * `m.value.cast<int>()` (visual_odometry.cpp:547).  max_dist / max_reproj <= 0 disable that check (the
 * `track_lost_` call at visual_odometry.cpp:600 passes neither; vo_params.json:2-3 ships 30 m / 20 px).
 * points: n_tracks x 3 (world frame); status: n_tracks, 0 = triangulated, 1 = fewer than 2 views (:572),
 * 2 = behind a camera, 3 = farther than max_dist, 4 = re-projection above max_reproj, 5 = point at infinity.   */
int bsgpu_triangulate(bsgpu_ctx* ctx, int32_t n_tracks, const int32_t* track_start, const int32_t* q_block,
                      const int32_t* p_block, const double* pixels, int32_t camera, int32_t truncate_pixels,
                      double max_dist, double max_reproj, double* points, int32_t* status);

/* Frame localisation for a batch of frames — VisualOdometry::LocalizeFrame (bs_models/src/visual_odometry.cpp:217-300): the
 * frame's 2D-3D pairs (GetPixelPointPairs, :612-650), the required_points_to_refine gate, the robust refinement of the pose with
 * its 6x6 covariance ([EXT] beam_cv::PoseRefinement::RefinePose, :240-248) and the screening average of ComputeAverageReprojection
 * (:1247-1272).  libbeam's PoseRefinement is not in the reference checkout, so what PoseRefinement(0.02, true, 0.2) (:72) sets
 * cannot be read: the loss and the LM options are arguments.  The optimisation itself is, by construction, the one-pose
 * BSGPU_F_REPROJ problem: minimise 1/2 sum rho(|w (z - pi(K, T_cam_baselink T_WORLD_BASELINK^-1 P))|^2) over the baselink pose
 * (orientation on BSGPU_MANIFOLD_QUAT_RIGHT, position Euclidean) with bsgpu_solve's trust-region loop (Ceres LM, Jacobi scaling,
 * tolerance exits, invalid-step counting); max_solver_time_in_seconds is not honoured and the linear-solver fields are ignored.
 *   frame f holds observations [obs_start[f], obs_start[f+1]) (obs_start[0] == 0, non-decreasing); pixels: 2 per observation
 *   (truncated to integers when truncate_pixels != 0, the reference's cast<int>(), for the solve and for the average alike).
 *   points: 3 per observation, world frame; OR lm_block: per observation a 3-d Euclidean block of ctx, read at its CURRENT device
 *   values (the context must have been finalized or solved).  Exactly one of the two.
 *   camera: per frame, an index into the bsgpu_set_cameras table.  q_init / p_init: per frame T_WORLD_BASELINK (wxyz, xyz).
 *   loss_kind / loss_a: BSGPU_LOSS_* and its scale; sqrt_info: w of every pair.  min_points: required_points_to_refine.
 *   image_width / image_height: bounds of the average (<= 0: no bounds check).
 * Outputs per frame: q_out / p_out; cov_out (36, may be NULL): the marginal covariance (J^T J)^-1 of [p (3), q tangent (3)] at the
 * returned pose from the undamped, loss-corrected J^T J — bsgpu_covariance_joint({p, q}) of the same problem, in the (x, y, z, roll,
 * pitch, yaw) order LocalizeFrame converts to.  libbeam expresses its covariance on T_CAMERA_WORLD's parameters; this one is on the
 * baselink pose.  avg_reproj (may be NULL): sum of |z - pi| over the pairs with P_c.z > 0 inside the image, divided by ALL of the
 * frame's pairs (0 for an empty frame).  final_cost, iterations (may be NULL).  status: 0 refined (converged or at the iteration
 * cap), 1 fewer than min_points observations (pose returned unchanged, nothing solved), 2 unusable (non-finite values or the
 * invalid-step limit), 3 refined but J^T J singular (a Cholesky pivot not positive or not finite): covariance NaN.  NaN also in
 * cov_out for statuses 1 and 2.
 * The context is not changed (values, iteration record, finalize state); points-only mode needs nothing but cameras.  A frame's
 * results do not depend on the other frames of the call.  Argument errors (bad camera index, an lm_block that is not a 3-d Euclidean
 * block, both or neither of points / lm_block, lm_block without device values, a malformed obs_start) -> INVALID.           */
int bsgpu_localize_frames(bsgpu_ctx* ctx, int32_t n_frames, const int32_t* obs_start, const double* pixels, const double* points,
                          const int32_t* lm_block, const int32_t* camera, const double* q_init, const double* p_init,
                          int32_t loss_kind, double loss_a, double sqrt_info, int32_t truncate_pixels, int32_t min_points,
                          int32_t image_width, int32_t image_height, const bsgpu_options* options, double* q_out, double* p_out,
                          double* cov_out, double* avg_reproj, double* final_cost, int32_t* iterations, int32_t* status);

/* Five-point RANSAC track screening for a batch of match sets — the
 * cv::findEssentialMat(fp1, fp2, K, cv::RANSAC, prob, threshold, mask) call of VisualOdometry::AddMeasurementsToContainer
 * (bs_models/src/visual_odometry.cpp:516-519) and SLAMInitialization (slam_initialization.cpp:898-901), whose mask decides which
 * tracks are erased before a frame is localised.  [EXT] OpenCV is not in the reference checkout: the semantics below are RECALLED
 * from OpenCV 4 (findEssentialMat / RANSACPointSetRegistrator) and could not be verified (DESIGN.md "Essential-matrix RANSAC").
 *   set k holds matches [match_start[k], match_start[k+1]) (match_start[0] == 0, non-decreasing); px_prev / px_cur: 2 per match,
 *   pixels of the previous and the current frame; K: per set (fx, fy, cx, cy).
 *   Pixels are normalised with K, threshold_px is divided by (fx + fy) / 2.  Minimal sample: 5 matches; model: every real essential
 *   matrix of the five-point solver; error: the squared Sampson distance; inlier: error <= threshold^2.  Loop: niters = max_iters;
 *   for sample s = 0, 1, ... while s < niters, every solution of sample s (in ascending order of its first entry, |E|_F = 1, largest
 *   entry positive) whose inlier count is strictly greater than max(best, 4) becomes the best and sets
 *   niters = update(prob, (n - good) / n, 5, niters) [num = log(1 - prob), den = log(1 - (1 - ep)^5); niters when den >= 0 or
 *   -num >= niters * -den, otherwise round(num / den); 0 when ep == 0].  No refit; the mask is the best model's inlier set.
 *   Sampler (part of the contract, all arithmetic mod 2^64): state = seed ^ (k * 0x9E3779B97F4A7C15) ^ (s * 0xBF58476D1CE4E5B9) with
 *   k the set's position in THIS call; each draw is splitmix64 (state += 0x9E3779B97F4A7C15; z = state;
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^= z >> 31; index = z mod n); a draw equal
 *   to an earlier index of the same sample is drawn again.  A sample whose solver finds no real solution counts as an iteration.
 * Outputs: mask (1 per match: 1 keep, 0 erase); E (9 per set, row-major, on normalised coordinates, may be NULL); n_inliers, n_iters
 * (samples the loop consumed), best_sample (5 per set: the winning sample's match indices inside the set) — each may be NULL;
 * status per set: BSGPU_RANSAC_OK; BSGPU_RANSAC_TOO_FEW (fewer than 5 matches: mask all 1 — the reference's erase loop runs over an
 * empty mask and erases nothing — E zeros, n_iters 0, best_sample -1); BSGPU_RANSAC_NO_MODEL (no solution ever reached 5 inliers:
 * mask all 1, E zeros; a decision of this library, OpenCV's behaviour there is not verifiable here).
 * A set's results do not depend on the other sets of the call except through its position k.  The context need not be finalized:
 * only its device and stream are used, and it is not changed.  INVALID: a NULL ctx / match_start / px_prev / px_cur / K / mask /
 * status, a malformed match_start, prob outside (0, 1), threshold_px <= 0, max_iters <= 0, a focal length <= 0.  UNSUPPORTED: a set
 * of more than BSGPU_RANSAC_MAX_MATCHES matches.                                                                                  */
enum { BSGPU_RANSAC_OK = 0, BSGPU_RANSAC_TOO_FEW = 1, BSGPU_RANSAC_NO_MODEL = 2 };
#define BSGPU_RANSAC_MAX_MATCHES 65536
int bsgpu_essential_ransac(bsgpu_ctx* ctx, int32_t n_sets, const int32_t* match_start, const double* px_prev, const double* px_cur,
                           const double* K, double prob, double threshold_px, int32_t max_iters, uint64_t seed, uint8_t* mask,
                           double* E, int32_t* n_inliers, int32_t* n_iters, int32_t* best_sample, int32_t* status);

/* P3P RANSAC frame poses for a batch of frames — the
 * beam_cv::AbsolutePoseEstimator::RANSACEstimator(camera_model, pixels, points, 100) call of
 * bs_models::vision::ComputePathWithVision (bs_models/src/lib/vision/utils.cpp:143-188), which gives every keyframe between the
 * first and the last image of SLAMInitialization's window its pose from 2D-3D pairs (slam_initialization.cpp:216), and the pose a
 * frame needs when there is no frame initialiser or after track_lost_: q_out / p_out are bsgpu_localize_frames' q_init / p_init.
 * [EXT] libbeam is not in the reference checkout: the semantics below are RECALLED and could not be verified (DESIGN.md
 * "Absolute-pose RANSAC").  Recalled: a fixed loop of max_iterations, a random 3-subset per iteration, up to 4 P3P poses each, inlier =
 * reprojection distance below a pixel threshold (default 5), the best count wins, no refit.  This library's own choices: the sampler,
 * the order of a sample's solutions, "strictly greater than max(best, 3)", P_c.z > 0 as part of the inlier test, the optional early
 * termination (prob > 0), TOO_FEW below 4 pairs, and what a frame without a model returns.
 *   frame f holds pairs [obs_start[f], obs_start[f+1]) (obs_start[0] == 0, non-decreasing); pixels: 2 per pair, undistorted,
 *   truncated toward zero when truncate_pixels != 0 (the reference's cast<int>(), utils.cpp:159), for the solve and for the scoring
 *   alike; points: 3 per pair, world frame; camera: per frame, an index into the bsgpu_set_cameras table (pinhole K, T_cam_baselink).
 *   Minimal sample: 3 pairs; model: every real P3P solution T_CAMERA_WORLD = [R|t] (at most 4) with all three depths positive, in
 *   ascending order of the camera-frame depth of the sample's FIRST point; score: P_c = R P + t, inlier iff P_c.z > 0 and
 *   (fx x/z + cx - u)^2 + (fy y/z + cy - v)^2 < threshold_px^2, every multiply-add a fused one.  Loop: niters = max_iters; for sample
 *   s = 0, 1, ... while s < niters, every solution of sample s whose inlier count is strictly greater than max(best, 3) becomes the
 *   best and, when prob lies inside (0, 1), sets niters = update(prob, (n - good) / n, 3, niters) [num = log(1 - prob),
 *   den = log(1 - (1 - ep)^3); niters when den >= 0 or -num >= niters * -den, otherwise round(num / den); 0 when ep == 0].
 *   prob == 0: no early termination — the libbeam loop as recalled; max_iters = 100 is the reference's call.  No refit; the mask is
 *   the best model's inlier set.
 *   Sampler (part of the contract, all arithmetic mod 2^64): state = seed ^ (k * 0x9E3779B97F4A7C15) ^ (s * 0xBF58476D1CE4E5B9) with
 *   k the frame's position in THIS call; three distinct indices by the draw and redraw rule of bsgpu_essential_ransac (splitmix64,
 *   index = z mod n, a draw equal to an earlier index of the same sample is drawn again).  A sample without a solution counts as an
 *   iteration.
 * Outputs: mask (1 per pair: 1 = inlier of the best model); q_out (4 per frame, wxyz, unit, w >= 0) / p_out (3 per frame):
 * T_WORLD_BASELINK = T_CAMERA_WORLD^-1 T_cam_baselink (visual_odometry.cpp:252-253); T_cam_world (12 per frame, row-major [R|t], may
 * be NULL); n_inliers, n_iters (samples the loop consumed), best_sample (3 per frame: the winning sample's pair indices inside the
 * frame) — each may be NULL; status per frame: BSGPU_RANSAC_OK; BSGPU_RANSAC_TOO_FEW (fewer than 4 pairs — three cannot tell P3P's
 * solutions apart: n_iters 0); BSGPU_RANSAC_NO_MODEL (no solution ever reached 4 inliers).  In both of those the mask is all 0,
 * n_inliers 0, best_sample -1 and every pose output NaN: a frame without a model has no pose (a decision of this library; libbeam's
 * behaviour there is not verifiable here).
 * A frame's results do not depend on the other frames of the call except through its position k.  The context needs cameras only: it
 * need not be finalized and is not changed.  INVALID: a NULL ctx / obs_start / pixels / points / camera / mask / q_out / p_out /
 * status, n_frames < 0, a malformed obs_start, a camera index outside the table, prob outside [0, 1) or NaN, threshold_px <= 0,
 * max_iters <= 0.  UNSUPPORTED: a frame of more than BSGPU_RANSAC_MAX_MATCHES pairs.  Nothing is written on an argument error.   */
int bsgpu_absolute_pose_ransac(bsgpu_ctx* ctx, int32_t n_frames, const int32_t* obs_start, const double* pixels,
                               const double* points, const int32_t* camera, double prob, double threshold_px,
                               int32_t max_iters, uint64_t seed, int32_t truncate_pixels, uint8_t* mask,
                               double* q_out, double* p_out, double* T_cam_world, int32_t* n_inliers,
                               int32_t* n_iters, int32_t* best_sample, int32_t* status);

/* Seven-point RANSAC two-view bootstrap for a batch of match sets — steps 1 and 2 of bs_models::vision::ComputePathWithVision
 * (bs_models/src/lib/vision/utils.cpp:44-94, called from slam_initialization.cpp:216): the relative pose of the last image of the
 * window against the first, beam_cv::RelativePoseEstimator::RANSACEstimator(cam, cam, first, last, SEVENPOINT, 100), the two-view
 * triangulation of every match, Triangulation::TriangulatePoints, and the 10 px / 80 % validity gate.  Together with
 * bsgpu_absolute_pose_ransac (step 3) and bsgpu_solve (step 4) the bootstrap stays on the device; `points` at valid_mask are the
 * world points step 3 takes.
 * [EXT] libbeam is not in the reference checkout: the semantics below are RECALLED and could not be verified (DESIGN.md
 * "Relative-pose RANSAC").  Recalled: a fixed loop of max_iterations, a random 7-subset per iteration, the seven-point solver's one
 * or three matrices, each decomposed into its four poses, every pose scored by triangulating every match and reprojecting it into
 * both images against a pixel threshold (default 5), the best count wins, no refit.  This library's own choices: the sampler, the
 * order of a sample's matrices and of a matrix' four poses, "strictly greater than max(best, 7)", positive depth in both cameras as
 * part of the inlier test, the optional early termination (prob > 0), TOO_FEW below 8 matches, and what a set without a model
 * returns.
 *   set k holds matches [match_start[k], match_start[k+1]) (match_start[0] == 0, non-decreasing); px_first / px_last: 2 per match,
 *   undistorted pixels of the first and the last image, truncated toward zero when truncate_pixels != 0 (the reference's
 *   cast<int>(), utils.cpp:34-36) — for the solve, the scoring, the triangulation and the gate alike; camera: per set, an index into
 *   the bsgpu_set_cameras table; the one pinhole camera serves both images (the reference passes camera_model twice).  Normalised
 *   coordinates are x = ((u - cx) / fx, (v - cy) / fy).
 *   Minimal sample: 7 distinct matches.  Models: every real E of the two-dimensional null space of the 7 x 9 system
 *   x_last^T E x_first = 0 with det E = 0 (one or three), scaled to |E|_F = 1 with its largest-magnitude entry positive, in ascending
 *   order of E[0] (the five-point rule).  Each E = U diag(s) V^T (U, V proper rotations) gives four poses T_last_first = [R|t],
 *   R in {U W V^T, U W^T V^T}, t = +-u3, in the order (R_a, +t), (R_a, -t), (R_b, +t), (R_b, -t): R_a the rotation with the larger
 *   trace, +t the unit left null vector with its largest-magnitude component positive.  All four are hypotheses.
 *   Triangulation: bsgpu_triangulate's definition for the two views [I|0] and [R|t] — unit bearings, four DLT rows, the right
 *   singular vector of the smallest singular value, de-homogenised; homogeneous w == 0 is the point at infinity (its status 5).
 *   Inlier iff the point is finite, its depth is positive in both cameras and the squared reprojection distance is below
 *   threshold_px^2 in BOTH images, every multiply-add of the test a fused one.
 *   Loop: niters = max_iters; for sample s = 0, 1, ... while s < niters, every hypothesis of sample s, in the order above, whose
 *   inlier count is strictly greater than max(best, 7) becomes the best and, when prob lies inside (0, 1), sets
 *   niters = update(prob, (n - good) / n, 7, niters) [bsgpu_absolute_pose_ransac's rule with exponent 7].  prob == 0: no early
 *   termination — the libbeam loop as recalled; max_iters = 100, threshold_px = 5 (libbeam's default as recalled) is the reference's
 *   call.  No refit.  A sample without a model counts as an iteration.
 *   Sampler (part of the contract): state = seed ^ (k * 0x9E3779B97F4A7C15) ^ (s * 0xBF58476D1CE4E5B9) with k the set's position in
 *   THIS call; seven distinct indices by the draw and redraw rule of bsgpu_essential_ransac.
 *   After the loop (utils.cpp:57-94): points (3 per match) in the first camera's frame — the reference's world — triangulated under
 *   the best model, NaN for a point at infinity; valid_mask[i] = 1 iff the point is in front of both cameras and both reprojection
 *   distances are below validate_px (the reference: 10); inlier_ratio = sum(valid_mask) / n in double (the reference's total_size is
 *   decremented but never read); pair_valid = !(inlier_ratio < min_inlier_ratio) (the reference: 0.8; it compares a float ratio —
 *   for n <= 65 536 = BSGPU_RANSAC_MAX_MATCHES the two comparisons agree).
 * Outputs: mask (1 per match: 1 = inlier of the best model); T_last_first (12 per set, row-major [R|t], |t| = 1, may be NULL);
 * q_out (8 per set) / p_out (6 per set): TWO poses per set, T_WORLD_BASELINK of the first and then of the last image with
 * world = first camera (AddCameraPose, utils.cpp:108-109): T_cam_baselink and T_last_first^-1 T_cam_baselink, each wxyz with w >= 0
 * and xyz, as bsgpu_localize_frames takes them; points, valid_mask, inlier_ratio (may be NULL); pair_valid (1 per set); n_inliers,
 * n_iters (samples the loop consumed), best_sample (7 per set) — each may be NULL; status per set: BSGPU_RANSAC_OK;
 * BSGPU_RANSAC_TOO_FEW (fewer than 8 matches — seven always fit their own model: n_iters 0); BSGPU_RANSAC_NO_MODEL (no hypothesis
 * ever reached 8 inliers).  In both of those both masks are 0, the counts 0, best_sample -1, pair_valid 0 and every pose, point and
 * ratio NaN (a decision of this library; libbeam's behaviour there is not verifiable here).
 * A set's results do not depend on the other sets of the call except through its position k.  The context needs cameras only: it
 * need not be finalized and is not changed.  INVALID: a NULL ctx / match_start / px_first / px_last / camera / mask / q_out / p_out /
 * pair_valid / status, n_sets < 0, a malformed match_start, a camera index outside the table, prob outside [0, 1) or NaN,
 * threshold_px <= 0, validate_px <= 0, max_iters <= 0, min_inlier_ratio outside [0, 1].  UNSUPPORTED: a set of more than
 * BSGPU_RANSAC_MAX_MATCHES matches.  Nothing is written on an argument error.                                                       */
int bsgpu_relative_pose_ransac(bsgpu_ctx* ctx, int32_t n_sets, const int32_t* match_start, const double* px_first,
                               const double* px_last, const int32_t* camera, double prob, double threshold_px,
                               int32_t max_iters, uint64_t seed, int32_t truncate_pixels, double validate_px,
                               double min_inlier_ratio, uint8_t* mask, double* T_last_first, double* q_out, double* p_out,
                               double* points, uint8_t* valid_mask, double* inlier_ratio, int32_t* pair_valid,
                               int32_t* n_inliers, int32_t* n_iters, int32_t* best_sample, int32_t* status);

/* ---- measurement helpers (used by bench.py only) --------------------------- */
/* Launches the Jacobian-evaluation kernel of the reprojection factors `reps`
 * times on the context's stream between two HIP events and returns the average
 * milliseconds per launch (<0 on error).                                        */
double bsgpu_time_reproj_jacobian_ms(bsgpu_ctx* ctx, int32_t reps);
/* The same for EVERY factor type of the problem (reprojection, IMU, relative / absolute pose, priors): mean milliseconds of one
 * evaluation of residuals + Jacobians at the current values, and the algorithmic bytes of that evaluation (SURVEY.md 8(d):
 * 196-200 B per reprojection factor, ~990 B per relative-pose factor, ~6.1 KB per IMU factor).  Measurement hooks: what
 * CostFunction::Evaluate costs per LM iteration ([EXT] ceres::Problem::Evaluate inside fixed_lag_smoother.cpp:281).        */
double bsgpu_time_eval_ms(bsgpu_ctx* ctx, int32_t reps);
int64_t bsgpu_eval_bytes(const bsgpu_ctx* ctx);
/* Block rows and non-zero 3x3 blocks of the block-sparse J^T J of the PCG path (both 0 on the dense Schur path).           */
int bsgpu_bsr_info(bsgpu_ctx* ctx, int32_t* block_rows, int32_t* nnz_blocks);
/* Algorithmic bytes one launch of that kernel moves. */
int64_t bsgpu_reproj_jacobian_bytes(const bsgpu_ctx* ctx);
/* Measurement: the phases of a full LM step timed IN SITU — `reps` steps exactly as bsgpu_solve enqueues them for an accepted step
 * (dense Schur path), a HIP event at every phase boundary on the solver's stream.  ms_out[BSGPU_PHASE_NUM]: mean milliseconds
 * per phase; work_out[BSGPU_PHASE_NUM] (may be NULL): the algorithmic work of the phase's dominant kernel — bytes, or FP64 flops
 * for BSGPU_PHASE_FACTOR — 0 where none is defined.  The values return to those of the last finalize. */
enum {
  BSGPU_PHASE_EVAL_REPROJ = 0,    /* reproj_eval_kernel<true>: residuals + Jacobians of the reprojection factors */
  BSGPU_PHASE_EVAL_OTHER = 1,     /* IMU / relative-pose / prior factors */
  BSGPU_PHASE_LANDMARK = 2,       /* clear + landmark_kernel: H_ll, its Cholesky, C and rho per factor */
  BSGPU_PHASE_PAIRS = 3,          /* pairs_kernel: camera-pair blocks of the reduced system */
  BSGPU_PHASE_ASSEMBLE_OTHER = 4, /* pose-only factors, LM diagonal, gradient norms */
  BSGPU_PHASE_FACTOR = 5,         /* Cholesky of the reduced camera system (FP64 MFMA) */
  BSGPU_PHASE_BACKSOLVE = 6,      /* L^T y = y' */
  BSGPU_PHASE_BACKSUB = 7,        /* landmark back-substitution + model-cost terms */
  BSGPU_PHASE_CANDIDATE = 8,      /* x [+] delta, cost at the candidate, end-of-step reduction */
  BSGPU_PHASE_NUM = 9
};
int bsgpu_profile_step(bsgpu_ctx* ctx, const bsgpu_options* options, int32_t reps, double* ms_out, double* work_out);

/* Stand-alone dense SPD solve A x = b (row-major n x n, host pointers) through the kernels the
 * reduced camera system uses after Schur elimination — test and measurement hook for the FP64
 * MFMA Cholesky.  The tile structure is taken from the non-zeros of A; max_chains caps the number
 * of independent sub-chains of the nested-dissection ordering (<= 1: natural order).
 * ms_out: HIP-event time.                                                                       */
int bsgpu_dense_solve(int device, int32_t n, const double* A, const double* b, double* x,
                      int32_t max_chains, double* ms_out);
/* Diagnostics of the tiled-Cholesky plan of the finalized problem. */
int bsgpu_plan_info(const bsgpu_ctx* ctx, int32_t* n_chains, int32_t* n_steps, int32_t* n_tiles);
/* What the elimination order of the reduced camera system is planned for (the [EXT] choice Ceres makes once for everyone in
 * ceres::Solver::Options::linear_solver_ordering_type; the reference's fixed-lag smoother takes the default,
 * bs_optimizers/src/fixed_lag_smoother.cpp:281 through fuse_core::Graph::optimize):
 *   BSGPU_PLAN_LATENCY (default)  one window solved by itself: a small system (<= 2 000 reduced dimensions) is planned under several
 *                                 settings of the dissection's cost model and keeps the one whose task list replays shortest;
 *   BSGPU_PLAN_THROUGHPUT         the window is one of many advanced side by side (bsgpu_solve_batch): the setting with the fewest
 *                                 supernodes — a batch is bound by the number of its factorisation workgroups, not by one window's path.
 * Takes effect at the next bsgpu_finalize() (a finalized context is planned again).                                                       */
enum { BSGPU_PLAN_LATENCY = 0, BSGPU_PLAN_THROUGHPUT = 1 };
int bsgpu_set_plan_preference(bsgpu_ctx* ctx, int32_t preference);

#ifdef __cplusplus
}
#endif
#endif /* BSGPU_H_ */
