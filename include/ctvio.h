/*
 * ctvio.h -- C ABI of libctvio.so: the MI355X (gfx950) sliding-window continuous-time VIO solve.
 *
 * Drop-in boundary for the Ceres build-and-solve behind the reference's
 * `ctrlvio::TrajectoryEstimator` (reference src/estimator/trajectory_estimator.h:61-206).  The reference
 * has no FFI; its seam is that C++ class, driven by TrajectoryManager::UpdateTrajectory
 * (src/estimator/trajectory_manager.cpp:317-483).  Every entry point below cites the reference
 * interface it replaces.  include/ctvio_estimator.hpp is the header-only C++ adaptor with the
 * reference's method names that a maintainer compiles src/estimator against.
 *
 * Conventions: plain C, caller-owned buffers, fp64 at the ABI regardless of device precision,
 * int status codes (no exceptions, like the reference: trajectory_estimator.cpp has no error paths),
 * one solver handle per host thread / HIP stream.  Parameters are addressed by INDEX (knot k,
 * bias state f, landmark l), not by pointer identity as in Ceres.
 *
 * Unknown ordering of every dense quantity:
 *   knot k : rot 6k..6k+2, pos 6k+3..6k+5 ; bias f : bg 6K+6f.., ba 6K+6f+3.. ; line delay 6K+6F ;
 *   P = 6K+6F+1 ; inverse depth l : P+l ; N = P+L.
 */
#ifndef CTVIO_H_
#define CTVIO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctvio_solver ctvio_solver;

enum ctvio_status {
  CTVIO_OK = 0,
  CTVIO_ERR_INVALID = 1,    /* bad argument / inconsistent sizes / time outside the spline */
  CTVIO_ERR_NO_DEVICE = 2,  /* no HIP device: the product path has NO CPU fallback */
  CTVIO_ERR_HIP = 3,        /* a HIP runtime call failed (ctvio_last_error has the text) */
  CTVIO_ERR_STATE = 4,      /* call order violated (e.g. solve before upload) */
  CTVIO_ERR_INTERNAL = 5    /* a device-side consistency check failed (an evaluation left the knot span planned for its landmark): the
                               results of THIS call are not to be trusted; the counter is cleared, the batch stays usable */
};

/* CTVIO_FP64 (the only mode): every residual, Jacobian, product and factorisation in fp64, like the reference (Ceres / Eigen
 * are all double); reproduces the fp64 CPU reference's iterates, final state to ~1e-9.  The mixed fp32 mode of rounds 1-2
 * (CTVIO_FP32 = 0) missed the 1e-4 contract on one window in four and was removed: ctvio_create rejects it. */
enum ctvio_precision { CTVIO_FP32_REMOVED = 0, CTVIO_FP64 = 1 };

/* Kinds of parameter blocks kept by a marginalisation prior (reference
 * marginalization_factor.h:115-129 keep_block_*; sizes 4->local 3, 3, 3, 3, 1). */
enum { CTVIO_PK_ROT = 0, CTVIO_PK_POS = 1, CTVIO_PK_BG = 2, CTVIO_PK_BA = 3, CTVIO_PK_LD = 4 };

/* Replaces TrajectoryEstimatorOptions (trajectory_estimator_options.h:34-68) + the ceres::Solver::Options
 * set in TrajectoryEstimator::Solve (trajectory_estimator.cpp:371-398).  Zero-initialise then call
 * ctvio_default_options.                                                                        */
typedef struct ctvio_options {
  int32_t device;               /* HIP device ordinal */
  int32_t precision;            /* CTVIO_FP64 */
  int32_t use_mfma;             /* 1 (default): products on v_mfma_f64_16x16x4_f64; 2: as 1 with every IMU group evaluated by the
                                   general body (the one groups with knot-to-knot rotations >= 0.5 rad or anisotropic accelerometer
                                   weights take): cross-check of the specialised body.  0 (the vector-ALU cross-check kernels of rounds
                                   1-5) was removed: ctvio_create rejects it */
  int32_t check_every;          /* host polls "all windows terminated" every n LM iterations */
  double function_tolerance;    /* 1e-6  Ceres defaults, see SURVEY.md Appendix A */
  double gradient_tolerance;    /* 1e-10 */
  double parameter_tolerance;   /* 1e-8 */
  double initial_radius;        /* 1e4 */
  double max_radius, min_radius;/* 1e16, 1e-32 */
  double min_relative_decrease; /* 1e-3 */
  double min_lm_diagonal, max_lm_diagonal; /* 1e-6, 1e32 */
  int32_t max_consecutive_invalid_steps;   /* 5 */
  int32_t deterministic;        /* 1: order-fixed accumulation everywhere (no floating-point atomics): two runs of the same batch
                                   are bitwise equal, also when profiling (ctvio_set_profiling) splits the launches differently.
                                   It exists for batches whose every window has K <= 25 (packed Hessian in LDS):
                                   ctvio_upload / ctvio_set_batch return CTVIO_ERR_INVALID for any other batch
                                   instead of silently accumulating with atomics.  -1 (default): on for batches of <= 64 windows
                                   where it applies, the atomic path (run-to-run differences ~1e-13 in the state) otherwise; 0: off.
                                   2: order-fixed accumulation for EVERY batch the solver accepts (windows up to P = 1024, mixed
                                   batches, IMU-only long splines): the windows with K <= 25 run exactly as under 1 (same bits),
                                   the others assemble their pose block with one owner per entry and a summation order fixed by
                                   the upload plan.  Two runs of the same batch are bitwise equal. */
  int32_t host_threads;         /* host threads that validate / pack a batch (ctvio_set_batch, ctvio_upload); 0 = min(cores, 16) */
  int32_t use_graph;            /* 1 (default): the launch sequence of one LM pass is captured into a hipGraph and replayed */
  int32_t line_search;          /* 1 (default): Ceres' projected Armijo line search of bounds-constrained problems
                                   (a free line delay has bounds: trajectory_estimator.cpp:311-318 => Minimizer is_constrained) */
} ctvio_options;

/* One sliding window = what TrajectoryManager::UpdateTrajectory feeds a fresh TrajectoryEstimator
 * (trajectory_manager.cpp:331-451).  All pointers are read during ctvio_add_window only.          */
typedef struct ctvio_window {
  int32_t K, F, L, M, NB, V;    /* knots, bias states (frames), landmarks, IMU, bias-chain, visual blocks */
  int32_t pn, pnb;              /* prior residual dim / kept blocks (0: no prior) */
  int64_t t0_ns, dt_ns;         /* Se3Spline(time_interval_ns, start_time_ns), se3_spline.h:108-111 */
  const double *quat;           /* K*4 (x,y,z,w): getKnotSO3(i).data(), se3_spline.h:271 */
  const double *pos;            /* K*3: getKnotPos(i).data(), se3_spline.h:283 */
  const double *bias;           /* F*6 (bg, ba): para_bg_vec / para_ba_vec, trajectory_manager.cpp:332-342 */
  const double *rho;            /* L: para_Feature[l][0], trajectory_manager.h:96 */
  double ld, ld_lo, ld_hi;      /* trajectory_->line_delay, ld_lower, ld_upper (trajectory.h:55-62,99-103) */
  int32_t fix_ld;               /* trajectory_->fix_ld (trajectory_estimator.cpp:312-318) */
  int32_t lock_bg, lock_ba;     /* options.lock_wb / lock_ab (trajectory_estimator.cpp:236-245) */
  int32_t fixed_upto;           /* SetFixedIndex(idx) / lock_traj (trajectory_estimator.cpp:134-138); -1 none (see also knot_const) */
  double q_CI[4], p_CI[3];      /* ImageFeatureDelayFactor::S_CtoI / p_CinI (image_feature_factor.h:273-274) */
  double gravity[3];            /* AddIMUMeasurementAnalytic gravity argument */
  double imu_w[6];              /* info_vec (opt_weight.h:124-126) */
  double img_w;                 /* ImageFeatureDelayFactor::sqrt_info = img_w*I2 (trajectory_manager.cpp:57) */
  double cauchy_a;              /* ceres::CauchyLoss(a) of every visual block without an entry in v_cauchy; <= 0 : none */
  /* AddIMUMeasurementAnalytic (trajectory_estimator.h:102-106) x M */
  const int64_t *imu_t; const double *imu_gyro, *imu_acc; const int32_t *imu_bias;
  /* AddBiasFactor (trajectory_estimator.h:109-112) x NB : r = w .* (b_j - b_i), dt = 1 */
  const int32_t *bc_i, *bc_j; const double *bc_w;
  /* AddImageFeatureDelayAnalytic (trajectory_estimator.h:128-131) x V */
  const int32_t *v_lm; const int64_t *v_ti, *v_tj; const int32_t *v_rowi, *v_rowj;
  const double *v_pi, *v_pj;    /* V*2 (x, y), z = 1 */
  /* AddMarginalizationFactor (trajectory_estimator.h:146-148): r = r0 + J0*dx over the kept blocks */
  const double *pJ0;            /* pn*pn COLUMN-major (Eigen default of linearized_jacobians) */
  const double *pr0;            /* pn */
  const int32_t *p_kind, *p_index, *p_off; /* pnb: block kind, knot/frame index, column offset (keep_block_idx - m).  The blocks
                                   tile [0, pn) without overlap, and each (kind, index) appears at most once -- a duplicate block
                                   is refused with CTVIO_ERR_INVALID, as Ceres refuses a parameter block listed twice in one
                                   residual block; hence pn <= P */
  const double *p_x0;           /* pnb*4: keep_block_data (quaternion x,y,z,w or 3-vector / scalar, zero padded) */
  /* per residual block: the reference creates one loss per AddImageFeatureDelayAnalytic call, CauchyLoss(marg_this_feature ?
   * 1 : 2) (trajectory_estimator.cpp:320-323).  V entries (<= 0: no loss for that block) or NULL: cauchy_a for every block. */
  const double *v_cauchy;
  /* per knot: constancy is decided per AddControlPoints call (trajectory_estimator.cpp:134-138), so the constant knots need not
   * be a prefix.  K flags (non-zero: SetParameterBlockConstant) or NULL; applied on top of fixed_upto. */
  const uint8_t *knot_const;
} ctvio_window;

/* Replaces ceres::Solver::Summary (callers only print BriefReport(): trajectory_manager.cpp:314,455). */
typedef struct ctvio_summary {
  int32_t iterations;           /* Ceres-style iteration counter at exit */
  int32_t num_successful, num_unsuccessful;
  int32_t termination;          /* 0 max-iterations 1 gradient 2 parameter 3 function 4 min-radius 5 failure */
  double initial_cost, final_cost, final_radius;
  int32_t num_line_search_steps;   /* ceres::Solver::Summary::num_line_search_steps: Armijo iterations beyond the first trial */
  int32_t num_line_search_reduced; /* LM iterations whose step was shortened by the projected line search */
} ctvio_summary;

void ctvio_default_options(ctvio_options *opt);
const char *ctvio_status_string(int32_t status);
const char *ctvio_last_error(void);
int32_t ctvio_device_count(void);

/* new TrajectoryEstimator(trajectory, option) / ~TrajectoryEstimator (trajectory_estimator.h:76-84):
 * one handle owns a HIP stream and the device buffers of a BATCH of independent windows.            */
int32_t ctvio_create(const ctvio_options *opt, ctvio_solver **out);
void ctvio_destroy(ctvio_solver *s);

/* Drop all windows of the batch (a fresh estimator per solve in the reference: trajectory_manager.cpp:350). */
int32_t ctvio_clear(ctvio_solver *s);
/* The Add*Factor calls of one UpdateTrajectory, recorded as one window; returns the window id in *id. */
int32_t ctvio_add_window(ctvio_solver *s, const ctvio_window *w, int32_t *id);
/* Pack (sort IMU samples into (segment,bias) groups, visual blocks landmark by landmark, prior J0^T J0, ...), PLAN THE SPARSITY of the
 * reduced system -- what the reference leaves to Ceres' SPARSE_NORMAL_CHOLESKY (trajectory_estimator.cpp:371-384): every landmark's knot span
 * over the box [ld_lo, ld_hi] of the line delay, the row order of Hpl, the envelope of the Schur complement -- and copy to HBM.
 * Checked here (CTVIO_ERR_INVALID otherwise): P = 6K + 6F + 1 <= 1024; at most 64 visual blocks per landmark; finite observations and line
 * delay; ld_lo <= ld_hi for a free line delay; every row time t + row * ld inside the spline for ld at both ends of the box. */
int32_t ctvio_upload(ctvio_solver *s);
/* ctvio_clear + n x ctvio_add_window + ctvio_upload in one call, without the intermediate host copy: the n windows are
 * validated and packed straight from the caller's buffers (read during this call only) by opt.host_threads threads into a
 * pinned staging arena, which reaches HBM with a single asynchronous copy on the solver's stream.  Window ids = 0..n-1. */
int32_t ctvio_set_batch(ctvio_solver *s, int32_t n, const ctvio_window *wins);
int32_t ctvio_num_windows(const ctvio_solver *s);

/* TrajectoryEstimator::Solve(max_iterations) (trajectory_estimator.cpp:367-408) for every window of the
 * batch, device-resident LM with Ceres 1.14 trust-region semantics.  out: n_windows summaries (may be NULL). */
int32_t ctvio_solve(ctvio_solver *s, int32_t max_iterations, ctvio_summary *out);

/* Results back to the caller's live state (Ceres updates the double* in place; here explicit). */
int32_t ctvio_get_state(ctvio_solver *s, int32_t id, double *quat, double *pos, double *bias, double *rho, double *ld);
/* The state of EVERY window of the batch with one device-to-host copy: quat (sum K x 4), pos (sum K x 3), bias (sum F x 6),
 * rho (sum L), ld (n), each concatenated in window order.  Any pointer may be NULL. */
int32_t ctvio_get_batch_state(ctvio_solver *s, double *quat, double *pos, double *bias, double *rho, double *ld);
/* Overwrite the state of an uploaded window (re-solve the same factors from another initial guess).  A free line delay is projected on
 * [ld_lo, ld_hi]; the line delay of a fix_ld window must equal the uploaded one (the landmarks' knot spans were planned for it). */
int32_t ctvio_set_state(ctvio_solver *s, int32_t id, const double *quat, const double *pos, const double *bias,
                        const double *rho, double ld);

/* Keep / bring back a device-side copy of the whole batch state: re-solve the same windows from the same initial
 * guess without touching the host (the reference rebuilds its estimator from live state every frame instead). */
int32_t ctvio_snapshot_state(ctvio_solver *s);
int32_t ctvio_restore_state(ctvio_solver *s);

/* ---- diagnostics used by the per-kernel parity tests (ResidualSummary analogue,
 *      trajectory_estimator.h:37-59,168-171) ---- */
/* Linearise window id at its current state: Hpp (P*P row-major, symmetric filled), W (P*L row-major,
 * Hpl block), Hll (L), g (N), cost.  Any pointer may be NULL. */
int32_t ctvio_linearize(ctvio_solver *s, int32_t id, double *Hpp, double *W, double *Hll, double *g, double *cost);
/* Cost only (residual kernels). */
int32_t ctvio_cost(ctvio_solver *s, int32_t id, double *cost);
/* ResidualSummary (trajectory_estimator.h:37-59, AddResidualInfo at trajectory_estimator.cpp:36-67): for window id at its
 * current state, the sum over all blocks of |r_i| for every residual component of each factor type (the cost functions' own
 * whitened residuals, before any robust loss) and the block counts.  sums: IMU [6], bias [6], image [2], prior [pn]
 * (14 + pn doubles); counts4 = {M, NB, V, prior present}; err_ave of PrintSummary = sums / count. */
int32_t ctvio_residual_summary(ctvio_solver *s, int32_t id, double *sums, int32_t *counts4);
/* One LM step for radius mu at the current state (Jacobi scaling from this same point): delta (N),
 * model cost change; the state is not modified. */
int32_t ctvio_lm_step(ctvio_solver *s, int32_t id, double mu, double *delta, double *model_cost_change);

/* Marginal covariances of window estimates, from the reduced system of the CURRENT state (the reference includes ceres/covariance.h at its
 * estimator boundary, src/estimator/trajectory_estimator.h:23; Ceres' Covariance::Compute + GetCovarianceBlockInTangentSpace are the
 * counterpart).  H = the normal matrix sum J~^T J~ that the linearise entry returns (prior, bias chain and robust corrector included, NO LM
 * damping).  An unknown is EXCLUDED if it is constant or if no factor touches it (H_jj == 0 exactly, e.g. the spline's last padding knot);
 * Sigma = (H restricted to the other unknowns)^-1; rotations in the tangent space of the Jacobians (q <- q exp(delta)).
 *   n_sel[w] (0 .. 64): trajectory unknowns selected in window w; sel: the selections concatenated, each an index in [0, P_w) in the unknown
 *   order above (any order inside a window, no duplicates); cov: window w owns n_sel[w]^2 doubles, row-major in the order of sel, packed in
 *   window order (may be NULL if every n_sel is 0): cov[i][j] = Sigma[sel_i][sel_j]; a constant selected unknown gives a zero row and
 *   column, an untouched one +inf on its diagonal and 0 elsewhere.  var_rho (sum L doubles, window order, the caller's landmark order; or
 *   NULL): the marginal variance of every inverse depth, +inf for a landmark without information (Hll == 0).  singular (n windows, or NULL):
 *   1 if the window's factorisation met a non-positive or non-finite pivot -- its outputs are NaN then; the call still returns CTVIO_OK.
 * CTVIO_ERR_INVALID: an entry outside [0, P), a duplicate, n_sel > 64; CTVIO_ERR_STATE before the upload; the handle stays usable.  The state,
 * the launch plan and the captured graph of the solve are left as they were; the kernels of the covariance use no atomics: where the linearisation
 * is order-fixed (opt.deterministic) two calls give the same bits, and the single-window entry
 * (n_sel, sel, cov, var_rho (L doubles), singular (1) of window id alone) gives the bits of the batch entry.  Pose-landmark cross terms are
 * not returned as such; ctvio_landmark_points_batch uses them for the covariance of every landmark's world point. */
int32_t ctvio_covariance_batch(ctvio_solver *s, const int32_t *n_sel, const int32_t *sel, double *cov, double *var_rho, int32_t *singular);
int32_t ctvio_covariance(ctvio_solver *s, int32_t id, int32_t n_sel, const int32_t *sel, double *cov, double *var_rho, int32_t *singular);

/* The 6 x 6 covariance of the POSE at a time -- what an odometry message, a gate or a downstream fuser takes -- from the same reduced system:
 * Sigma_pose(t) = J Sigma J^T, with H, the exclusions and Sigma exactly those of ctvio_covariance_batch (no damping) and J the Jacobian of the
 * pose at t against the spline unknowns, evaluated on the device (the cumulative-B-spline rotation Jacobian of the visual factors, reference
 * so3_spline_view.h:136-198).  Query i = (window win[i], absolute time t_ns[i]) at the CURRENT state; any number of queries per window, in any
 * order, from any windows -- no 64-unknown limit.  Segment and u by the integer-ns rule of ctvio_spline_eval; the time must lie in
 * [t0, t0 + (K - 3) dt).  The pose depends on knots s, s + 1, s + 2, and on s + 3 iff u > 0.
 *   Tangent of the result: R(t) <- R(t) exp(dtheta), p(t) <- p(t) + dp, ordered (theta0..2, p0..2) -- rotation first, as in the unknown order;
 *   the knots under the library's own retraction (R_k <- R_k exp(delta_k), p_k <- p_k + dp_k).
 *   q_SI = (x,y,z,w), p_SI (the arguments of ctvio_sensor_pose; both NULL: the body pose): the pose is T_I(t) T_SI, dtheta_S = R_SI^T dtheta_I,
 *   dp_S = dp_I - R_I(t) [p_SI]x dtheta_I.
 *   cov36: n x 36 doubles, row-major 6 x 6 per query, symmetric to the bit.  status (n entries, or NULL) per query:
 *     0 ok;  1 the window's factorisation met a non-positive or non-finite pivot: NaN;  2 a knot the pose depends on is touched by no factor:
 *     +inf on the diagonal, 0 elsewhere;  3 time outside the spline: NaN.
 *   Constant unknowns contribute nothing: a pose that depends on constant knots alone has the exact zero matrix and status 0.
 * The call returns CTVIO_OK for every status.  n == 0 returns CTVIO_OK and launches nothing.  CTVIO_ERR_STATE before the upload;
 * CTVIO_ERR_INVALID for a window id out of range, n < 0, a NULL win / t_ns / cov36 with n > 0, exactly one of q_SI / p_SI NULL (or a zero
 * quaternion); the handle stays usable.  The state, the launch plan and the captured graph of the solve are left as they were; no atomics:
 * where the linearisation is order-fixed (opt.deterministic) the bits of a query's result depend on its window and time alone -- not on the
 * entry (batch or single-window: win is window id for every query), the order of the queries, or which other query shares its tile. */
int32_t ctvio_pose_covariance_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int64_t *t_ns, const double *q_SI, const double *p_SI,
                                    double *cov36, int32_t *status);
int32_t ctvio_pose_covariance(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_ns, const double *q_SI, const double *p_SI, double *cov36,
                              int32_t *status);

/* The landmark cloud of a window with its uncertainty -- what VisualOdometry::GetLandmarksInWindow / GetMarginCloud assemble on the host
 * (visual_odometry.cpp:310-372: Rs[i] * (point * estimated_depth) + Ps[i]) and OdometryManager::PublishCloudAndTrajectory publishes --, at the
 * CURRENT state.  Landmark l is anchored at the observation (t_i, row_i, p_i = (x, y, 1)) that all its visual blocks share, with inverse
 * depth rho; the point as the visual factor models it:
 *   tau = t_i + row_i * (int64)(ld * 1e9)   (the time exactly as the factors take it),   x_c = p_i / rho,
 *   T_C = T_I(tau) (q_CI, p_CI)  (the window's camera extrinsic),   X = R_C x_c + p_C   (world frame, metres).
 * The reference takes the pose at the frame time t_i (per-row poses are expensive on its host): a stated difference, as for triangulateRS;
 * ctvio_sensor_pose gives the frame-time pose to a caller who wants that cloud.
 * cov9 = the first-order covariance of X in the world frame (dX, additive), from the same reduced system as ctvio_covariance_batch: H, the
 * exclusions and Sigma_pp are exactly those (no damping).  With Jp (3 x P) the Jacobian of X against the trajectory unknowns under the library's
 * retraction (R_k <- R_k exp(delta_k), p_k <- p_k + dp_k) -- the knots of tau through the camera-pose Jacobian of ctvio_pose_covariance,
 * [-R_C [x_c]x, I] J_pose, and the line-delay column row_i (R_I(tau) [omega(tau)]x (R_CI x_c + p_CI) + v(tau)), the formal derivative the
 * visual factor itself uses --, j_rho = dX / drho = -R_C p_i / rho^2, w_l the landmark's row of W and h_l = Hll_l:
 *   G = Jp^T - w_l j_rho^T / h_l  (rows of excluded unknowns zero),   Cov(X) = G^T Sigma_pp G + j_rho j_rho^T / h_l,
 * i.e. [Jp | j_rho] over the joint covariance of the trajectory and rho_l, pose-landmark cross terms included.
 *   point3 (3 doubles per landmark), cov9 (9 per landmark, row-major, symmetric to the bit), status (1 per landmark): sum L entries (batch) /
 *   L entries (window id), window order, the caller's landmark order (as ctvio_triangulate_batch); any of the three may be NULL.
 *   status 0: ok;  1: the window's factorisation met a non-positive or non-finite pivot: the point is valid, the covariance NaN;  2: no
 *   information on the inverse depth (Hll == 0 exactly): the point is valid, +inf on the diagonal and 0 elsewhere;  3: not computable -- rho <= 0
 *   or non-finite, no visual block, blocks that name more than one anchor observation, or tau outside the spline (the rules of
 *   ctvio_triangulate_batch): point and covariance NaN.
 * With cov9 == NULL nothing is linearised or factored: one kernel evaluates the points, and statuses 1 and 2 cannot occur; the points have the
 * bits of the covariance call's.  The call returns CTVIO_OK for every status, and for a batch or window with L = 0.  CTVIO_ERR_STATE before the
 * upload; CTVIO_ERR_INVALID for a window id out of range; the handle stays usable.  The state, the launch plan and the captured graph of the
 * solve are left as they were; no atomics: where the linearisation is order-fixed (opt.deterministic) the bits of a landmark's result depend on
 * its window and itself alone -- the single-window entry gives the batch entry's bits, and a second call repeats them. */
int32_t ctvio_landmark_points_batch(ctvio_solver *s, double *point3, double *cov9, int32_t *status);
int32_t ctvio_landmark_points(ctvio_solver *s, int32_t id, double *point3, double *cov9, int32_t *status);

/* The NAVIGATION STATE at a time -- orientation, position, world velocity, gyro bias, accelerometer bias -- with its joint 15 x 15 covariance:
 * what the reference reads after every solve to re-seed its IMU dead-reckoning (VisualOdometry::SlideWindow, visual_odometry.cpp:217-221,
 * Trajectory::GetIMUState, trajectory.cpp:27-37) and what IMU-rate odometry, a velocity / bias gate or a downstream fuser starts from.
 * Query i = (window win[i], absolute time t_ns[i], bias state frame[i] in [0, F)) at the CURRENT state; frame == NULL: F - 1, the newest frame,
 * for every query.  Any number of queries, in any order, from any windows.  Segment and u by the integer-ns rule of ctvio_spline_eval; the
 * time must lie in [t0, t0 + (K - 3) dt).  This is the BODY (IMU) state: there is no sensor extrinsic in this entry.
 *   state16 (n x 16 doubles, or NULL): (px, py, pz, qx, qy, qz, qw) as ctvio_spline_eval's pose7, the world velocity (transVelWorld) in 7..9,
 *   bg of bias state frame[i] in 10..12, ba in 13..15.
 *   cov225 (n x 225 doubles, row-major 15 x 15 per query, symmetric to the bit, or NULL): J Sigma J^T in the tangent (dtheta 0..2, dp 3..5,
 *   dv 6..8, dbg 9..11, dba 12..14), with H, the exclusions and Sigma exactly those of ctvio_covariance_batch (no damping).  R(t) <- R(t)
 *   exp(dtheta); p, v and the biases are additive; the knots under the library's own retraction.  Rows of J: the pose rows of
 *   ctvio_pose_covariance (body); velocity: c'_k(u) / dt I on the position unknowns of knots s .. s + 3 (knot s + 3 iff u > 0: c'_3 = u^2 / 2),
 *   zero against rotations; bias: one-hot on unknowns 6 K + 6 f .. 6 K + 6 f + 5.  Constant unknowns contribute nothing: a locked bias gives
 *   exact zero rows and columns, a state that depends on constant unknowns alone the exact zero matrix and status 0.
 *   With cov225 == NULL nothing is linearised or factored: one kernel evaluates the states, and statuses 1 and 2 cannot occur.
 *   status (n entries, or NULL) per query, in this precedence: 3 time outside the spline: state and covariance NaN;  2 a knot the state depends
 *   on, or the selected bias state, has a non-constant unknown no factor touches: state valid, +inf on the diagonal, 0 elsewhere;  1 the
 *   window's factorisation met a non-positive or non-finite pivot: state valid, covariance NaN;  0 ok.
 * The call returns CTVIO_OK for every status.  n == 0 returns CTVIO_OK and launches nothing.  CTVIO_ERR_STATE before the upload;
 * CTVIO_ERR_INVALID for a window id out of range, a frame outside [0, F), n < 0, a NULL win / t_ns with n > 0, all three outputs NULL with
 * n > 0; the handle stays usable.  The state, the launch plan and the captured graph of the solve are left as they were; no atomics: where the
 * linearisation is order-fixed (opt.deterministic) the bits of a query's result depend on its window, time and frame alone -- not on the entry
 * (batch or single-window: win is window id for every query), the order of the queries, or which other queries are in the call; a second
 * call repeats them. */
int32_t ctvio_nav_state_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int64_t *t_ns, const int32_t *frame, double *state16,
                              double *cov225, int32_t *status);
int32_t ctvio_nav_state(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_ns, const int32_t *frame, double *state16, double *cov225,
                        int32_t *status);

/* The BODY RATES at a time -- angular velocity, specific force, body-frame velocity -- with their joint covariance, and a Mahalanobis gate
 * for an IMU sample: the twist half of an odometry message (child-frame linear and angular velocity with a 6 x 6 covariance), a rate
 * uncertainty for a controller, and the inertial counterpart of ctvio_project_landmarks' gate.  The values are Se3Spline::rotVelBody /
 * transAccelWorld / transVelWorld (se3_spline.h:361-389) and the prediction inside IMUFactor::Evaluate (trajectory_value_factor.h:165-171);
 * the reference has no covariance for any of them.
 * Query i = (window win[i], absolute time t_ns[i], bias state frame[i] in [0, F)) at the CURRENT state; frame == NULL: F - 1 for every query.
 * Any number of queries, in any order, from any windows.  Segment and u by the integer-ns rule of ctvio_spline_eval; the time must lie in
 * [t0, t0 + (K - 3) dt).  This is the BODY (IMU) frame: there is no sensor extrinsic in this entry, as in ctvio_nav_state (a caller maps
 * (omega, v_B) and their joint block to another point of the body with its fixed lever arm).
 *   rates9 (n x 9 doubles, or NULL): omega in 0..2, the body angular velocity;  f = R(t)^T (p''(t) + g) in 3..5, the specific force, g the
 *   window's `gravity`, signed as in the IMU factor;  v_B = R(t)^T v_W(t) in 6..8, the body-frame velocity.
 *   cov225 (n x 225 doubles, row-major 15 x 15 per query, symmetric to the bit, or NULL): J Sigma J^T in the additive tangent (domega 0..2,
 *   df 3..5, dv_B 6..8, dbg 9..11, dba 12..14), with H, the exclusions and Sigma exactly those of ctvio_covariance_batch (no damping).  Rows of
 *   J against the knots s .. s + 3 (knot s + 3 only where u > 0) under the library's retraction: omega and f are the IMU factor's rows
 *   (rotations: Jw[k], Ja[k]; positions: zero, c''_k(u) / dt^2 R(t)^T);  v_B: [v_B]x J_theta,k on the rotations (J_theta,k the rotation rows
 *   of ctvio_pose_covariance), c'_k(u) / dt R(t)^T on the positions;  bias: one-hot on unknowns 6 K + 6 f .. 6 K + 6 f + 5.  The line delay
 *   and the inverse depths do not enter.  Constant unknowns contribute nothing: a locked bias gives exact zero rows and columns, a query that
 *   depends on constant unknowns alone the exact zero matrix and status 0.
 *   chi2 (n doubles, or NULL; requires meas6, n x 6: the gyro sample, then the accelerometer sample, as the IMU factor takes them): with the
 *   predicted reading z = (omega + bg_f, f + ba_f) and e = meas - z, chi2 = e^T S^-1 e, S = A C A^T + diag(sigma_k^2),
 *   A = [[I, 0, 0, I, 0], [0, I, 0, 0, I]], C the 15 x 15 block above: a 6 x 6 Cholesky on the device, from the very cov225 and rates9 bits
 *   that are returned.  noise6: the six standard deviations for the whole call; NULL: sigma_k = 1 / imu_w[k] of the query's window.  The gate
 *   is meant for NEW samples: for a sample that is already a factor of the window, estimate and measurement are correlated and S overstates
 *   the variance of e.  The samples of the window itself are tested by ctvio_imu_gate_batch, below.
 *   status (n entries, or NULL) per query, in this precedence: 3 time outside the spline: everything NaN;  2 a knot the query depends on, or
 *   the bias state, has a non-constant unknown no factor touches: values valid, +inf on the diagonal and 0 elsewhere, chi2 = 0;  1 the
 *   window's factorisation met a non-positive or non-finite pivot: values valid, covariance and chi2 NaN;  0 ok.
 *   With cov225 == NULL and chi2 == NULL nothing is linearised or factored: one kernel evaluates the values, statuses 1 and 2 cannot occur,
 *   and the values have the bits of the covariance call's.
 * The call returns CTVIO_OK for every status.  n == 0 returns CTVIO_OK and launches nothing.  CTVIO_ERR_STATE before the upload;
 * CTVIO_ERR_INVALID for a window id or frame out of range, n < 0, a NULL t_ns (batch entry: win) with n > 0, every output NULL with n > 0,
 * chi2 without meas6, a non-finite meas6, a non-positive or non-finite noise6 entry, noise6 == NULL with chi2 asked for and a queried window
 * whose imu_w has a non-positive entry; the handle stays usable.  The state, the launch plan and the captured graph of the solve are left as
 * they were; no atomics: where the linearisation is order-fixed (opt.deterministic) the bits of a query's outputs depend on its own arguments
 * alone -- not on the entry (batch or single-window: win is window id for every query), the order of the queries, which queries share a
 * call, or which optional outputs were asked for.
 * ctvio_last_timing: ms8[0..2] = k_cov_prepare, k_cov_solve, k_cov_rates_jac, ms8[7] the whole call; values only: ms8[2] and ms8[7]. */
int32_t ctvio_body_rates_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int64_t *t_ns, const int32_t *frame,
                               const double *meas6, const double *noise6,
                               double *rates9, double *cov225, double *chi2, int32_t *status);
int32_t ctvio_body_rates(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_ns, const int32_t *frame,
                         const double *meas6, const double *noise6,
                         double *rates9, double *cov225, double *chi2, int32_t *status);

/* The POSE INCREMENT between two times, T_ab = T(t_a)^-1 T(t_b), with its 6 x 6 covariance: what a pose-graph or loop-closure back end, a
 * keyframe-to-keyframe "between" factor, a lidar or wheel fuser or a drift gate consumes.  The entries above describe one time in the window's
 * own gauge, which the prior on the oldest knots fixes, so their uncertainty grows along the window; the increment carries the
 * cross-covariance of the two times and is the gauge-free quantity.
 * Query i = (window win[i], absolute times t_a_ns[i], t_b_ns[i]) at the CURRENT state.  Any number of queries, in any order, from any windows;
 * t_b may lie before t_a or equal it.  Segment and u of each time by the integer-ns rule of ctvio_spline_eval; each time must lie in
 * [t0, t0 + (K - 3) dt).  q_SI == p_SI == NULL: body poses; otherwise both poses are T_I(t) T_SI, exactly as in ctvio_pose_covariance.
 *   rel7 (n x 7 doubles, or NULL): (p_ab, q_ab as x, y, z, w) with R_ab = R_a^T R_b, p_ab = R_a^T (p_b - p_a); q_ab is a unit quaternion
 *   whose sign is whatever the product gives: compare it as a rotation.
 *   cov36 (n x 36 doubles, row-major 6 x 6 per query, symmetric to the bit, or NULL): J_rel Sigma J_rel^T in the tangent (dtheta 0..2, dp 3..5)
 *   of R_ab <- R_ab exp(dtheta), p_ab <- p_ab + dp (dp in frame a), with H, the exclusions and Sigma exactly those of ctvio_covariance_batch
 *   (no damping).  With J_a, J_b the 6 x P Jacobians of ctvio_pose_covariance at the two times (the knots under the library's own retraction):
 *     dtheta_ab = dtheta_b - R_ab^T dtheta_a,   dp_ab = [p_ab]x dtheta_a + R_a^T (dp_b - dp_a)
 *     J_rel = A_a J_a + A_b J_b,   A_a = [[-R_ab^T, 0], [[p_ab]x, -R_a^T]],   A_b = [[I, 0], [0, R_a^T]].
 *   Constant unknowns contribute nothing: a pair that depends on constant knots alone gives the exact zero matrix and status 0.
 *   With cov36 == NULL nothing is linearised or factored: one kernel evaluates the values, and statuses 1 and 2 cannot occur; the values have
 *   the bits of the covariance call's.
 *   status (n entries, or NULL) per query, in this precedence: 3 either time outside the spline: value and covariance NaN;  2 a knot either
 *   pose depends on (knot s + 3 only where u > 0) has a non-constant unknown no factor touches: value valid, +inf on the diagonal, 0
 *   elsewhere;  1 the window's factorisation met a non-positive or non-finite pivot: value valid, covariance NaN;  0 ok.
 * The call returns CTVIO_OK for every status.  n == 0 returns CTVIO_OK and launches nothing.  CTVIO_ERR_STATE before the upload;
 * CTVIO_ERR_INVALID for a window id out of range, n < 0, a NULL win / t_a_ns / t_b_ns with n > 0, both outputs and status NULL with n > 0,
 * exactly one of q_SI and p_SI NULL, a zero quaternion; the handle stays usable.  The state, the launch plan and the captured graph of the
 * solve are left as they were; no atomics: where the linearisation is order-fixed (opt.deterministic) the bits of a query's result depend on
 * its window and its two times alone -- not on the entry (batch or single-window: win is window id for every query), the order of the
 * queries, or which query shares its tile; a second call repeats them.
 * ctvio_last_timing: ms8[0..2] = k_cov_prepare, k_cov_solve, k_cov_rel_jac, ms8[7] the whole call; values only: ms8[2] and ms8[7]. */
int32_t ctvio_relative_pose_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int64_t *t_a_ns, const int64_t *t_b_ns,
                                  const double *q_SI, const double *p_SI, double *rel7, double *cov36, int32_t *status);
int32_t ctvio_relative_pose(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_a_ns, const int64_t *t_b_ns,
                            const double *q_SI, const double *p_SI, double *rel7, double *cov36, int32_t *status);

/* WHERE A LANDMARK FALLS IN THE CAMERA at a time, and how sure the window is: what a visual front end asks before the next solve -- the
 * prediction seeds the tracker, the 2 x 2 covariance sizes the search window, the Mahalanobis distance of a candidate match gates it.  The
 * value is the visual factor's own prediction (ImageFeatureDelayFactor::Evaluate, image_feature_factor.h:63-269: x_j.xy / x_j.z); the
 * reference has no covariance for it.
 * Query i = (window win[i], landmark lm[i] in the caller's landmark order, frame time t_ns[i], image row row[i]) at the CURRENT state.  Any
 * number of queries, in any order, from any windows; the same landmark may be queried many times.  Landmark l is anchored as in
 * ctvio_landmark_points: anchor observation (t_i, row_i, p_i), x_c = p_i / rho, X = R_C(tau_i) x_c + p_C(tau_i).  With
 * tau_q = t + row * (int64)(ld * 1e9) and the window's camera extrinsic:
 *   y = R_C(tau_q)^T (X - p_C(tau_q)),   proj3 = (y.x / y.z, y.y / y.z, y.z): the normalised image point and the depth in the query camera.
 * For a query that coincides with a visual block (t_j, row_j), img_w (proj.xy - p_j) is that block's residual before the robust loss.
 *   rm == NULL: row[i] is used as given.  rm != NULL (pinhole rows without distortion): row[i] is the first guess and the row is iterated
 *   rm->iterations times (1 .. 8): one iteration evaluates y at the current row, then sets row <- clamp(lrint(fy y.y / y.z + cy), 0, rows - 1).
 *   Value and Jacobian are taken at the final row, which goes to row_out (n entries, or NULL).  The row is treated as GIVEN in the
 *   covariance: its own dependence on the state is of second order in ld |dy/dt|.  A caller with a distorted camera passes rows explicitly.
 *   cov4 (n x 4 doubles, row-major 2 x 2, symmetric to the bit, or NULL): the first-order covariance of proj.xy, with H, the exclusions and
 *   Sigma exactly those of ctvio_covariance_batch (no damping).  With Pi = (1 / y.z) [[1, 0, -z0], [0, 1, -z1]], z = proj.xy, the row Jp of
 *   either coordinate against the trajectory unknowns (the library's retraction) is, on the knots of the anchor time, Pi R_Cq^T Jp_X with Jp_X
 *   the point Jacobian of ctvio_landmark_points; on the knots of the query time Pi ([y]x J_theta - R_Cq^T J_p) with (J_theta, J_p) the
 *   camera-pose Jacobian of ctvio_pose_covariance at tau_q; in the line-delay column the anchor's (Pi R_Cq^T times the line-delay column of
 *   ctvio_landmark_points) plus row_q Pi ([y]x omega_C - R_Cq^T v_C), omega_C = R_CI^T omega_I(tau_q), v_C = v_I(tau_q) + R_I(tau_q)
 *   [omega_I]x p_CI, the formal derivative the factor itself uses.  j = Pi R_Cq^T (-R_Ci p_i / rho^2) is the inverse-depth column.  Then
 *     G = Jp^T - w_l j^T / h_l  (rows of excluded unknowns zero),   Cov = G^T Sigma_pp G + j j^T / h_l,
 *   pose-landmark cross terms included.  Constant unknowns contribute nothing.
 *   chi2 (n doubles, or NULL; requires obs2, n x 2 candidate image points): e^T (Cov + I / img_w^2)^-1 e with e = obs - proj.xy, formed on
 *   the device from the very cov4 and proj3 bits that are returned.  The gate is meant for NEW matches: for an observation that is already a
 *   block of the window, estimate and measurement are correlated and the sum above overstates the variance of e.
 *   status (n entries, or NULL) per query, in this precedence: 3 not computable -- the landmark by the rules of ctvio_landmark_points status 3,
 *   tau_q outside [t0, t0 + (K - 3) dt) at any row visited, y.z <= 0 or non-finite at any row visited: everything NaN, row_out -1;  2
 *   Hll_l == 0, or a knot either time depends on (knot s + 3 only where u > 0) has a non-constant unknown no factor touches: value valid,
 *   +inf on the diagonal, 0 elsewhere, chi2 = 0;  1 the window's factorisation met a bad pivot: value valid, covariance and chi2 NaN;  0 ok.
 *   With cov4 == NULL and chi2 == NULL nothing is linearised or factored: one kernel evaluates the values, statuses 1 and 2 cannot occur, and
 *   the values have the bits of the covariance call's.
 * The call returns CTVIO_OK for every status.  n == 0 returns CTVIO_OK and launches nothing.  CTVIO_ERR_STATE before the upload;
 * CTVIO_ERR_INVALID for a window id or landmark index out of range, n < 0, a NULL lm / t_ns / row (batch entry: win) with n > 0, every output
 * NULL with n > 0, chi2 without obs2, a non-finite obs2, rm with iterations outside 1 .. 8, rows < 1 or non-finite fy / cy; the handle stays
 * usable.  The state, the launch plan and the captured graph of the solve are left as they were; no atomics: where the linearisation is
 * order-fixed (opt.deterministic) the bits of a query's result depend on its own arguments alone -- not on the entry (batch or single-window:
 * win is window id for every query), the order of the queries, which queries share its tile or call, or which optional outputs were asked for.
 * ctvio_last_timing: ms8[0..2] = k_cov_prepare, k_cov_solve, k_cov_proj_jac, ms8[7] the whole call; values only: ms8[2] and ms8[7]. */
typedef struct ctvio_row_model { double fy, cy; int32_t rows, iterations; } ctvio_row_model;   /* 24 bytes */
int32_t ctvio_project_landmarks_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int32_t *lm, const int64_t *t_ns, const int32_t *row,
                                      const ctvio_row_model *rm, const double *obs2,
                                      double *proj3, double *cov4, double *chi2, int32_t *row_out, int32_t *status);
int32_t ctvio_project_landmarks(ctvio_solver *s, int32_t id, int32_t n, const int32_t *lm, const int64_t *t_ns, const int32_t *row,
                                const ctvio_row_model *rm, const double *obs2,
                                double *proj3, double *cov4, double *chi2, int32_t *row_out, int32_t *status);

/* AFTER THE SOLVE, WHICH OBSERVATIONS ARE OUTLIERS: the leave-one-out (deleted) innovation test of every visual block of the windows
 * themselves.  ctvio_project_landmarks' gate is for NEW matches; an observation that is already a block of the window is correlated with the
 * estimate.  Here the block's own information is taken out of the normal matrix, the observation is predicted from everything else, and the
 * residual is gated against that prediction's covariance plus the measurement noise -- a 2 x 2 Woodbury correction per block on top of Sigma
 * of the full system, no second factorisation, and well defined under the Cauchy loss.
 * There are no query inputs: the blocks are the window's own, as uploaded.  Per-block outputs hold sum V entries (batch) or V entries
 * (single window), window after window and in the CALLER'S block order (ctvio_window.v_*); per-landmark outputs sum L or L entries in the
 * caller's landmark order.  Any output may be NULL.  Per block b = (l, t_j, row_j, p_j) at the CURRENT state, a_b = v_cauchy[b] (else
 * cauchy_a; <= 0: no loss):
 *   (proj.xy, depth) = ctvio_project_landmarks' proj3 for the query (l, t_j, row_j) with rm == NULL;
 *   res2 (x 2) = r = img_w (proj.xy - p_j), the factor's whitened residual before the loss; s = |r|^2;
 *   weight = rho'(s) = 1 / (1 + s / a_b^2), 1 without a loss;
 *   corrector S, as the linearisation applies it to the block's Jacobian rows (Ceres' Corrector): S = sqrt(rho') (I - alpha r r^T / s),
 *   alpha = 1 - sqrt(max(0, 1 + 2 s rho'' / rho')), rho'' = -(1 / a_b^2) / (1 + s / a_b^2)^2, with Corrector's rule alpha = 0 where s == 0 or
 *   rho'' <= 0 -- which the Cauchy loss always meets, so that S = sqrt(rho') I; S = I without a loss;
 *   Cw = img_w^2 C with C ctvio_project_landmarks' cov4 of that query (H, the exclusions and Sigma exactly those of ctvio_covariance_batch,
 *   pose-landmark cross terms included, no damping; constant unknowns contribute nothing);
 *   A = S Cw S (A <= I: the block's own J~^T J~ is part of H), redundancy = lambda_min(I - A) in closed form;
 *   cov4 (x 4, row-major 2 x 2, whitened, symmetric to the bit) = C_loo = Cw + Cw S (I - A)^-1 S Cw = J (H - J~_b^T J~_b)^-1 J^T (Woodbury);
 *   chi2 = r^T (C_loo + I)^-1 r, 2 degrees of freedom, formed on the device from the very res2 / cov4 bits that are returned.
 *   status, in this precedence: 3 not computable (ctvio_project_landmarks' status 3): everything NaN;  2 Hll_l == 0 or an untouched
 *   non-constant unknown under either time: values valid, redundancy 0, cov4 +inf on the diagonal and 0 elsewhere, chi2 = 0;  1 bad pivot in
 *   the window's factorisation: values valid, redundancy / cov4 / chi2 NaN;  4 redundancy < opt->min_redundancy -- the rest of the window
 *   cannot predict this observation, e.g. the only block of a landmark with a free depth: values and redundancy valid, cov4 +inf on the
 *   diagonal and 0 elsewhere, chi2 = 0;  0 ok.
 * Per landmark, over its blocks with status other than 3, in the library's packed block order (fixed by the upload): lm_count their number;
 * lm_stats3[0] the mean of |proj.xy - p_j| (unwhitened: what VINS-style outliersRejection thresholds), [1] the largest chi2 over its
 * status-0 blocks (0: none), [2] the smallest redundancy over its blocks of status 0 or 4 (+inf: none).  No blocks: 0 and (NaN, 0, +inf).
 * With redundancy, cov4, chi2 and lm_stats3 all NULL nothing is linearised or factored: statuses 1, 2 and 4 cannot occur and the values have
 * the bits of the covariance call's.
 * Returns CTVIO_OK for every status, and for V = 0 or L = 0 (nothing is launched).  CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for
 * a window id out of range, NULL options, min_redundancy outside (0, 1) or non-finite, every output NULL with V > 0; the handle stays
 * usable.  The state, the launch plan and the captured graph of the solve are left as they were; no atomics: where the linearisation is
 * order-fixed (opt.deterministic) the bits of a block's and a landmark's outputs depend on the window alone -- not on the entry, on which
 * outputs were asked for, or on how the call was sliced (large batches are walked in slices of windows so that the per-block scratch stays
 * bounded; the factorisation happens once) -- and a second call repeats them.
 * ctvio_last_timing: ms8[0..2] = k_cov_prepare, k_cov_solve, k_cov_gate_jac (a call of several slices: the first slice's record kernel; the
 * later ones run between the slices' k_cov_solve and count in ms8[1]), ms8[3] the landmark reduction, ms8[7] the whole call; values only:
 * ms8[2] (both kernels) and ms8[7]. */
typedef struct ctvio_gate_options { double min_redundancy; } ctvio_gate_options;   /* 8 bytes */
void ctvio_default_gate_options(ctvio_gate_options *o);                             /* 0.01 */
int32_t ctvio_visual_gate_batch(ctvio_solver *s, const ctvio_gate_options *o, double *res2, double *weight, double *depth, double *redundancy,
                                double *cov4, double *chi2, int32_t *status, double *lm_stats3, int32_t *lm_count);
int32_t ctvio_visual_gate(ctvio_solver *s, int32_t id, const ctvio_gate_options *o, double *res2, double *weight, double *depth, double *redundancy,
                          double *cov4, double *chi2, int32_t *status, double *lm_stats3, int32_t *lm_count);

/* ACTING ON THE GATE: every visual block of an uploaded batch is ACTIVE or INACTIVE.  ctvio_upload, ctvio_set_batch and ctvio_clear make
 * every block active; ctvio_set_state and ctvio_snapshot_state / ctvio_restore_state leave the flags alone (they are not state).  The flags
 * live in device memory and are read on every pass, so changing them moves neither the launch plan nor the captured graph
 * (ctvio_graph_captures).
 * An inactive block is NOT A FACTOR of the window: it contributes exactly 0.0 to the cost, to Hpp, W, Hll and g and to the block records
 * the assembly reads, on every linearisation path (LDS-resident and wide windows, deterministic 1 and 2, use_mfma 1 and 2, cost-only passes
 * and candidate evaluation, graph replay and profiled launches) -- also where its own projection is not finite (the block is not evaluated
 * at all; its anchor's record still is, which needs no more than a finite non-zero inverse depth).  ctvio_solve, ctvio_linearize,
 * ctvio_cost, ctvio_lm_step, ctvio_marginalize(_batch) and every covariance-family entry see the window without it.  A landmark whose
 * blocks are all inactive has Hll == 0 and gets the existing "no information" statuses; a knot that inactive blocks alone touch is
 * "untouched" by the existing rule.  ctvio_residual_summary's image sums and counts4[2] cover the active blocks.
 * THE STRUCTURE STAYS THE UPLOAD'S: the slot order, the sparsity plan (a superset of any subset of the blocks), the landmark spans, the
 * anchor of a landmark, ctvio_triangulate* and ctvio_shift_anchor_batch do not look at the flags.
 * ctvio_visual_gate(_batch) on an inactive block is the RE-ADMISSION test: its information is not in H, so nothing is taken out (S = 0,
 * weight = 0), and the formulas above give redundancy = 1, cov4 = Cw and chi2 = r^T (Cw + I)^-1 r -- ctvio_project_landmarks' new-match
 * gate, whitened.  Where its status would be 0 it is 5 (inactive); the precedence is 3, 2, 1, 5, 4, 0.  lm_count and lm_stats3 run over the
 * active blocks only.  With every block active the gate computes what it computed before there were flags; one output is formed more
 * strictly than it used to be: lm_stats3[0] now rounds every operation of |proj.xy - p_j| once, as its definition above says (the earlier
 * build fused a product into the sum), and may differ from that build in the last place.
 * active: one byte per block in the CALLER'S block order (ctvio_window.v_*), non-zero = active; sum V entries (batch) / V (window id).
 * set: NULL makes every block active.  get: 1 / 0.  CTVIO_OK also for V = 0; CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a
 * window id out of range or a NULL output. */
int32_t ctvio_set_visual_active_batch(ctvio_solver *s, const uint8_t *active);
int32_t ctvio_set_visual_active(ctvio_solver *s, int32_t id, const uint8_t *active);
int32_t ctvio_get_visual_active_batch(ctvio_solver *s, uint8_t *active);
int32_t ctvio_get_visual_active(ctvio_solver *s, int32_t id, uint8_t *active);

/* CULL: gate + decision + flag update, all on the device, at the CURRENT state and the current flags.  The rules are written in terms of
 * what ctvio_visual_gate_batch with the same min_redundancy returns at this state and these flags, and are applied to those very bits
 * (k_vis_cull reads the gate's device outputs), so that on an order-fixed linearisation the result does not depend on the entry or on how
 * the call was sliced.
 *   block rule: an active block of status 0 with chi2 > chi2_max is switched off; with worst_only only the landmark's worst such block
 *     (largest chi2, first in the packed block order on a tie) -- Baarda-style data snooping, one deletion per re-solve;
 *   landmark rule: every active status-0 block of a landmark with lm_count > 0 and lm_stats3[0] > mean_error_max is switched off;
 *   drop_uncomputable: an active block of status 3 is switched off (the counterpart of setDepth's failure flag + removeFailures).
 * Never touched: blocks of status 1, 2 or 4 (4: the rest of the window cannot check the block) and blocks that are already inactive -- the
 * cull never re-admits; a caller re-admits with ctvio_set_visual_active from the gate's status-5 results.  A window whose factorisation
 * failed is left alone entirely (n_culled = 0).
 * n_culled: blocks switched off by THIS call per window (n windows / 1); active: the flags after the call, as ctvio_get_visual_active*;
 * either may be NULL.  CTVIO_OK also for V = 0 (nothing is launched); CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a window id
 * out of range, NULL options or min_redundancy outside (0, 1); the handle stays usable.  The state, the launch plan and the captured
 * graph are left as they were.  ctvio_last_timing: as after a full ctvio_visual_gate call, and ms8[4] = k_vis_cull. */
typedef struct ctvio_cull_options {
  double min_redundancy;     /* the gate's; 0.01 */
  double chi2_max;           /* 9.21 (99 % point, 2 dof); <= 0: block rule off */
  double mean_error_max;     /* landmark rule on lm_stats3[0] (unwhitened mean |proj - p_j|); <= 0 (default): off */
  int32_t worst_only;        /* 0 (default); 1: the block rule takes at most one block per landmark and call */
  int32_t drop_uncomputable; /* 1 (default) */
} ctvio_cull_options;        /* 32 bytes */
void ctvio_default_cull_options(ctvio_cull_options *o);
int32_t ctvio_cull_visual_batch(ctvio_solver *s, const ctvio_cull_options *o, int32_t *n_culled, uint8_t *active);
int32_t ctvio_cull_visual(ctvio_solver *s, int32_t id, const ctvio_cull_options *o, int32_t *n_culled, uint8_t *active);

/* AFTER THE SOLVE, WHICH IMU SAMPLES ARE OUTLIERS: the leave-one-out (deleted) residual test of every IMU sample of the windows themselves.
 * The IMU factor carries no robust loss, so a saturated, dropped or mis-timed sample pulls the spline at full weight; ctvio_body_rates' gate is
 * for NEW samples.  Here the sample's own information is taken out of the normal matrix -- a 6 x 6 Woodbury correction per sample on top of
 * Sigma of the full system, no second factorisation.
 * There are no query inputs: the samples are the window's own, as uploaded.  Per-sample outputs hold sum M entries (batch) or M entries
 * (single window), window after window and in the CALLER'S sample order (ctvio_window.imu_*); frame_stats4 holds sum F or F entries of four
 * doubles, one per bias state.  Any output may be NULL.  Per sample m = (t, bias state b, gyro, acc) at the CURRENT state, w = imu_w:
 *   z = (omega(t) + bg_b, f(t) + ba_b): ctvio_body_rates' rates9[0..5] at (t, b) plus the bias -- the same segment / u rule and the same code,
 *   so the same bits;
 *   res6 (x 6) = r = w (.) (z - meas), the factor's own whitened residual, every operation rounded once;
 *   J (6 x P) = w (.) the omega and f rows of ctvio_body_rates' Jacobian plus its one-hot bias rows; knot s + 3 enters only where u > 0, rows
 *   of excluded unknowns are zero, constant unknowns contribute nothing;
 *   A = J Sigma J^T (H, the exclusions and Sigma exactly those of ctvio_covariance_batch, no damping).  A <= I: the sample's own J^T J is
 *   part of H.  There is no loss and so no corrector: S = I;
 *   redundancy = lambda_min(I - A);
 *   cov36 (x 36, row-major 6 x 6, whitened, symmetric to the bit) = C_loo = (I - A)^-1 - I = J (H - J^T J)^-1 J^T (Woodbury with S = I);
 *   chi2 = r^T (I - A)^-1 r, 6 degrees of freedom (16.81 is the 99 % point), formed on the device from the very res6 bits that are returned.
 *   It equals r_loo^T (C_loo + I)^-1 r_loo with r_loo = (I - A)^-1 r, the first-order residual of the sample against the estimate re-solved
 *   without it, and is also the test of the post-fit residual against its own covariance Cov(r) = I - A.  Under the model its mean over the
 *   samples of a window is 6: a check of the tuning of imu_w.
 *   THIS IS NOT ctvio_visual_gate's chi2: that one gates the POST-FIT residual r against C_loo + I, which with S = I reads r^T (I - A) r and
 *   is smaller by up to (1 - lambda)^2 (5.67 against 6.23 on the config1 fixture).
 *   status, in this precedence: 2 a non-constant unknown under the sample's knots or its bias state is touched by no factor (possible only
 *   with zero weights): values valid, redundancy 0, cov36 +inf on the diagonal and 0 elsewhere, chi2 = 0;  1 bad pivot in the window's
 *   factorisation: values valid, redundancy / cov36 / chi2 NaN;  4 redundancy < opt->min_redundancy -- the rest of the window cannot predict
 *   this sample: values and redundancy valid, cov36 +inf on the diagonal and 0 elsewhere, chi2 = 0;  0 ok.  Status 3 cannot occur: the upload
 *   refuses IMU times outside the spline.  A sample that depends on constant unknowns alone: A = 0, redundancy 1, a zero cov36,
 *   chi2 = |r|^2, status 0.
 * Per bias state, over the samples naming it, in the library's packed sample order (fixed by the upload): frame_stats4[0] the number of
 * its status-0 samples, [1] their mean chi2 (NaN: none), [2] their largest chi2 (0: none), [3] the smallest redundancy over status 0 or 4
 * (+inf: none).
 * With redundancy, cov36, chi2 and frame_stats4 all NULL nothing is linearised or factored: one kernel writes res6 and status (all 0), with
 * the bits of the full call's.
 * Returns CTVIO_OK for every status, and for M = 0 (nothing is launched).  CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a window
 * id out of range, NULL options, min_redundancy outside (0, 1) or non-finite, every output NULL with M > 0; the handle stays usable.  The
 * state, the launch plan and the captured graph of the solve are left as they were; no atomics: where the linearisation is order-fixed
 * (opt.deterministic) the bits of a sample's and a bias state's outputs depend on the window alone -- not on the entry, on which outputs
 * were asked for, or on how the call was sliced (large batches are walked in slices of windows so that the per-sample scratch stays bounded;
 * the factorisation happens once) -- and a second call repeats them.
 * ctvio_last_timing: ms8[0..2] = k_cov_prepare, k_cov_solve, k_cov_imugate_jac (a call of several slices: the first slice's record kernel;
 * the later ones run between the slices' k_cov_solve and count in ms8[1]), ms8[3] the bias-state reduction, ms8[7] the whole call; values
 * only: ms8[2] and ms8[7]. */
int32_t ctvio_imu_gate_batch(ctvio_solver *s, const ctvio_gate_options *o, double *res6, double *redundancy, double *cov36, double *chi2,
                             int32_t *status, double *frame_stats4);
int32_t ctvio_imu_gate(ctvio_solver *s, int32_t id, const ctvio_gate_options *o, double *res6, double *redundancy, double *cov36, double *chi2,
                       int32_t *status, double *frame_stats4);

/* BETWEEN FRAMES: IMU dead reckoning from the navigation state, with its 15 x 15 covariance -- what VisualOdometry::ProcessIMU
 * (visual_odometry.cpp:137-172) does with the state SlideWindow hands it, and where AddImageToWindow (:188-191) takes the predicted pose of
 * the next frame from; beside the mean, the first-order covariance that IntegrationBase::midPointIntegration (integration_base.h:100-179)
 * carries through the same recurrence (F, G, noise_covariance).
 * Query i = (window win[i], bias state frame[i] in [0, F), m_i = n_imu[i] samples); frame == NULL: F - 1 for every query.  The samples of all
 * queries are concatenated in query order: absolute times imu_t (ns), imu_gyro and imu_acc as 3 doubles each.  Sample 0 of a query is the
 * measurement at the start: the state and covariance at imu_t[0] are exactly those of ctvio_nav_state_batch at (win, imu_t[0], frame) -- the same
 * reduced system, exclusions, tangent (dtheta 0..2, dp 3..5, dv 6..8, dbg 9..11, dba 12..14) and statuses, the same bits.
 * Sample j >= 1 is one midpoint step with dt = (imu_t[j] - imu_t[j - 1]) * 1e-9, the formulas of ProcessIMU:
 *   w  = (w_{j-1} + w_j) / 2 - bg             R' = R Exp(w dt)
 *   A  = ((R (a_{j-1} - ba) - g) + (R' (a_j - ba) - g)) / 2      g = the window's `gravity` (sign as in the IMU factor)
 *   p' = p + dt v + dt^2 A / 2                v' = v + dt A      bg, ba unchanged
 * Exp is the exact exponential; the reference's Utility::deltaQ is its first-order quaternion (1, w dt / 2), normalised later: the two agree
 * to O(|w dt|^3) per step.
 * Covariance: P_j = F P_{j-1} F^T + G Q G^T with F and G the EXACT Jacobians of this step map in the tangent above (R <- R Exp(dtheta), the rest
 * additive) and additive noise per sample (n_g0, n_a0, n_g1, n_a1, n_bg, n_ba), as the reference's 18-column G has it.  With E = Exp(w dt),
 * J = Jr(w dt), [.] the hat map, u0 = a_{j-1} - ba, u1 = a_j - ba, A_th = -(R [u0] + R' [u1] E^T) / 2, A_g = R' [u1] J dt / 2, A_a = -(R + R') / 2:
 *   F = [ E^T          0  0     -J dt        0          ]    G (rows theta, p, v): n_g0 = n_g1 = -F[., bg] / 2;
 *       [ dt^2 A_th/2  I  dt I  dt^2 A_g/2   dt^2 A_a/2 ]      n_a0: p dt^2 R / 4, v dt R / 2;  n_a1: p dt^2 R' / 4, v dt R' / 2;
 *       [ dt A_th      0  I     dt A_g       dt A_a     ]      n_bg: dt I on the bg rows;  n_ba: dt I on the ba rows
 *       [ 0 0 0 I 0 ] [ 0 0 0 0 I ]                          Q = diag(gyr_n^2, acc_n^2, gyr_n^2, acc_n^2, gyr_w^2, acc_w^2) (x) I_3
 * The sigmas are taken as IntegrationBase takes them: per-sample standard deviations, the bias walk enters as sigma dt; the correlation of
 * consecutive steps through their shared sample is neglected, as there.  The reference's F is the first-order form of these blocks (I - [w] dt
 * for E^T, J = I): at 1 rad/s and 5 ms the entries differ by 2.5e-3 relative.
 *   state16 (or NULL): as ctvio_nav_state's; the biases are those of the chosen state for every sample.   cov225 (or NULL): row-major,
 *   symmetric to the bit.  Each holds sum m_i entries in query order, then sample order, sample 0 included; with last_only != 0 each holds n
 *   entries, the last sample of each query.  status (or NULL): one entry per query, the precedence of ctvio_nav_state: 3 imu_t[0] outside
 *   [t0, t0 + (K - 3) dt): states and covariances NaN;  2 an untouched non-constant unknown under the start state: states valid for every
 *   sample, +inf on the diagonal and 0 elsewhere for every sample;  1 bad pivot in the window's factorisation: states valid, covariances NaN;
 *   0 ok.  Constant unknowns contribute nothing to P_0.  With cov225 == NULL nothing is linearised or factored (statuses 1 and 2 cannot
 *   occur) and the states have the bits of the covariance call's.
 * The call returns CTVIO_OK for every status, and for n == 0, where it launches nothing.  CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID
 * for a window id or frame out of range, n < 0, a NULL n_imu / imu_t / imu_gyro / imu_acc / noise (batch: win) with n > 0, all three outputs
 * NULL with n > 0, m_i < 1 or m_i > 4096, sample times of a query that are not strictly increasing, a non-finite measurement, a negative or
 * non-finite sigma; the handle stays usable.  The state, the launch plan and the captured graph of the solve are left as they were; no atomics:
 * where the linearisation is order-fixed (opt.deterministic) the bits of a query's outputs depend on its window, frame, samples and sigmas
 * alone -- not on the entry (batch or single), the order of the queries, which queries share a wave or a call, or last_only. */
typedef struct ctvio_imu_noise { double gyr_n, acc_n, gyr_w, acc_w; } ctvio_imu_noise;  /* GYR_N, ACC_N, GYR_W, ACC_W */
void ctvio_default_imu_noise(ctvio_imu_noise *o);   /* 4.0e-3, 8.0e-2, 2.0e-6, 4.0e-5: reference parameters.cpp:13-16 */
int32_t ctvio_imu_predict_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int32_t *frame, const int32_t *n_imu,
                                const int64_t *imu_t, const double *imu_gyro, const double *imu_acc, const ctvio_imu_noise *noise,
                                int32_t last_only, double *state16, double *cov225, int32_t *status);
/* One query of window id (frame -1: the newest bias state) with m samples: the same bits as the batch entry. */
int32_t ctvio_imu_predict(ctvio_solver *s, int32_t id, int32_t frame, int32_t m, const int64_t *imu_t, const double *imu_gyro,
                          const double *imu_acc, const ctvio_imu_noise *noise, int32_t last_only, double *state16, double *cov225,
                          int32_t *status);

/* WHERE A LANDMARK FALLS IN THE NEXT IMAGE: ctvio_project_landmarks at an IMU-PREDICTED pose beyond the end of the spline.  A window's spline
 * ends shortly after its newest frame, so the one frame a tracker needs seeding for -- the next one -- lies outside ctvio_project_landmarks'
 * range; ctvio_imu_predict carries the state there but stops at the state, and the covariance of an image point needs the cross-covariance
 * of the propagated pose and the landmark (shared anchor knots, line delay, inverse depth), which no entry returns.  This entry composes
 * the two on the device.  The reference predicts the pose the same way (VisualOdometry::ProcessIMU) and has no covariance for the point.
 * PREDICTIONS (n_pred) are exactly the queries of ctvio_imu_predict_batch: prediction k = (window win[k], bias state frame[k], frame == NULL:
 * F - 1, n_imu[k] samples), the samples concatenated in prediction order, the same refusals.  POINTS (n_pts): point i = (prediction pred[i],
 * landmark lm[i] in the caller's landmark order of that prediction's window, image row row[i]); many points normally share a prediction.
 * End state: (R, p, v, bg, ba) at t_e = imu_t[m - 1] is ctvio_imu_predict's with last_only, the same bits; state16 (n_pred x 16, or NULL)
 * returns it (NaN where imu_t[0] is outside the spline).  w_e = the last sample's gyro reading - bg (m = 1: sample 0).
 * Pose at the row time -- a STATED MODEL, a constant-rate extrapolation over the read-out, the acceleration term a delta^2 / 2 neglected:
 *   delta = (double)(row * (int64)(ld * 1e9)) * 1e-9,   R_I(tau) = R Exp(w_e delta),   p_I(tau) = p + delta v,   T_C = T_I(tau) (q_CI, p_CI).
 * Value: X the world point of ctvio_landmark_points (same anchor rules), y = R_C^T (X - p_C), proj3 = (y.x / y.z, y.y / y.z, y.z).
 *   rm: the row iteration of ctvio_project_landmarks (1 .. 8 iterations; value and Jacobian at the final row, returned in row_out).
 *   cov4 (n_pts x 4, row-major 2 x 2, symmetric to the bit, or NULL): with Pi as in ctvio_project_landmarks, E = Exp(w_e delta),
 *     B (6 x 15) = [[E^T, 0, 0, -delta Jr(w_e delta), 0], [0, I, delta I, 0, 0]]   (the body pose at tau against the tangent of ctvio_imu_predict),
 *     C_ext = the body -> camera tangent map of ctvio_pose_covariance (dtheta_C = R_CI^T dtheta_I, dp_C = dp_I - R_I(tau) [p_CI]x dtheta_I),
 *     A (2 x 15) = Pi [[y]x, -R_C^T] C_ext B,   Phi = F_{m-1} ... F_1 the product of ctvio_imu_predict's exact step Jacobians (m = 1: I),
 *     J_nav = the 15 rows of ctvio_nav_state at (imu_t[0], frame),   Jp = A Phi J_nav + Pi R_C^T Jp_X,
 *   Jp_X the point Jacobian of ctvio_landmark_points with its line-delay column; the line-delay column additionally gets
 *   row Pi ([y]x R_CI^T w_e - R_C^T (v + R_I(tau) [w_e]x p_CI)), the formal derivative of the read-out;  j = Pi R_C^T (-R_Ci p_i / rho^2).  Then
 *     G = Jp^T - w_l j^T / h_l  (rows of excluded unknowns zero),   Cov = G^T Sigma_pp G + j j^T / h_l + A N A^T,
 *   H, the exclusions and Sigma_pp exactly those of ctvio_covariance_batch; N the process noise of the propagation, N_j = F N_{j-1} F^T +
 *   G Q G^T from N_0 = 0 (ctvio_imu_predict's recurrence with a zero start).  Cross terms between the propagated pose and the landmark are
 *   included; the row is treated as given; constant unknowns contribute nothing.
 *   chi2 (n_pts doubles, or NULL; requires obs2, n_pts x 2): e^T (Cov + I / img_w^2)^-1 e, e = obs - proj.xy, formed on the device from the
 *   very bits that are returned, as in ctvio_project_landmarks.
 *   status (n_pts entries, or NULL) per point, in this precedence: 3 imu_t[0] of its prediction outside [t0, t0 + (K - 3) dt), the landmark
 *   not computable (ctvio_landmark_points status 3), y.z <= 0 or non-finite at any row visited: everything NaN, row_out -1;  2 Hll_l == 0, or
 *   a non-constant unknown no factor touches under the anchor knots, the knots of imu_t[0] (knot s + 3 only where u > 0) or the chosen bias
 *   state: value valid, +inf on the diagonal, 0 elsewhere, chi2 = 0;  1 bad pivot in the window's factorisation: value valid, covariance and
 *   chi2 NaN;  0 ok.  With cov4 == NULL and chi2 == NULL nothing is linearised or factored, statuses 1 and 2 cannot occur, and the values
 *   have the bits of the covariance call's.
 * The single-window entry is one prediction of window id (frame -1: the newest bias state) with every point under it: the batch entry's bits.
 * The call returns CTVIO_OK for every status, and for n_pred == 0 or n_pts == 0, where it launches nothing.  CTVIO_ERR_STATE before the
 * upload; CTVIO_ERR_INVALID for every refusal of ctvio_imu_predict_batch (window id or frame out of range, a count < 0, NULL sample arrays or
 * noise, m outside 1 .. 4096, sample times not strictly increasing, a non-finite measurement, a negative or non-finite sigma), pred[i] outside
 * [0, n_pred), a landmark index out of range for its prediction's window, a NULL pred / lm / row, all of proj3 / cov4 / chi2 / state16 NULL,
 * chi2 without obs2, a non-finite obs2, a bad rm; the handle stays usable.  The state, the launch plan and the captured graph of the solve are
 * left as they were; no atomics: where the linearisation is order-fixed (opt.deterministic) the bits of a point depend on its own arguments
 * and its prediction's samples alone -- not on the entry, the order of points or predictions, which points share a tile or call, or which
 * optional outputs were asked for.
 * ctvio_last_timing: ms8[0..2] = k_cov_prepare, k_cov_solve, k_cov_pred_jac, ms8[3] = k_imu_transition, ms8[7] the whole call; values only:
 * ms8[2], ms8[3] and ms8[7]. */
int32_t ctvio_predict_landmarks_batch(ctvio_solver *s, int64_t n_pred, const int32_t *win, const int32_t *frame, const int32_t *n_imu,
                                      const int64_t *imu_t, const double *imu_gyro, const double *imu_acc, const ctvio_imu_noise *noise,
                                      int64_t n_pts, const int32_t *pred, const int32_t *lm, const int32_t *row, const ctvio_row_model *rm,
                                      const double *obs2, double *state16, double *proj3, double *cov4, double *chi2, int32_t *row_out,
                                      int32_t *status);
int32_t ctvio_predict_landmarks(ctvio_solver *s, int32_t id, int32_t frame, int32_t m, const int64_t *imu_t, const double *imu_gyro,
                                const double *imu_acc, const ctvio_imu_noise *noise, int32_t n_pts, const int32_t *lm, const int32_t *row,
                                const ctvio_row_model *rm, const double *obs2, double *state16, double *proj3, double *cov4, double *chi2,
                                int32_t *row_out, int32_t *status);

/* Landmark depths on the device, at the CURRENT state: what FeatureManager::triangulate gives a window to start from (called from
 * VisualOdometry::AddImageToWindow, visual_odometry.cpp:174-193; feature_manager.cpp:226-274) and what removeBackShiftDepth does to them after
 * a slide (feature_manager.cpp:341-381, visual_odometry.cpp:299-308). */
typedef struct ctvio_triangulate_options {
  int32_t row_times;   /* 1 (default): every observation at t + row * line delay of the CURRENT state, the time computed exactly as the factors
                          compute it (truncated integer-ns line delay) -- the reference's triangulateRS (feature_manager.cpp:276-339, `#if 0`
                          there: per-row poses are expensive on the host); 0: at its frame time t -- the reference's live triangulate(Ps, Rs) */
  int32_t only_unset;  /* 1 (default): only landmarks whose current rho <= 0 (reference: `if (estimated_depth > 0) continue`); 0: every landmark */
  int32_t apply;       /* 1 (default): rho = 1 / depth is written into the device state for every landmark flagged 1 or 2 (triangulation only) */
  double min_depth;    /* 0.1 (feature_manager.cpp:218) */
  double init_depth;   /* 5.0 (parameters.cpp:44 INIT_DEPTH) */
} ctvio_triangulate_options;
void ctvio_default_triangulate_options(ctvio_triangulate_options *o);
/* Triangulation of every landmark of the batch / of window id.  Observation 0 of a landmark is the anchor (t_i, row_i, p_i) of its visual
 * blocks, observations 1..n the (t_j, row_j, p_j) of the blocks (n <= 64).  Camera pose of an observation: the spline pose times (q_CI, p_CI)
 * (Trajectory::GetSensorPose); relative to the anchor camera R = R0^T Rk, t = R0^T (tk - t0), P = [R^T | -R^T t], f = (x, y, 1) / |.|; every
 * observation, the anchor included, gives the rows f0 P.row(2) - f2 P.row(0) and f1 P.row(2) - f2 P.row(1); depth = v[2] / v[3] for the right
 * singular vector v of the smallest singular value of that 2 (n + 1) x 4 matrix (feature_manager.cpp:236-266).  The singular vector comes from
 * one-sided Jacobi on the matrix itself (not from its normal matrix), rows summed in a fixed order: two calls give the same bits, and the
 * single-window entry the bits of the batch entry.  The blocks enter in the library's packed order, not the caller's: v does not depend on
 * the order of the rows beyond rounding.
 *   depth, flag: sum L entries (batch) / L entries (window id), window order, the caller's landmark order; either may be NULL.
 *   flag 0: skipped by only_unset, depth = 1 / rho;  1: triangulated;  2: the depth came out below min_depth or non-finite and init_depth is
 *   returned (the reference's `depth < 0.1` lets NaN through: a stated difference);  3: not triangulable -- no block, blocks that name more
 *   than one anchor observation, or an observation time outside the spline -- depth = 1 / rho, never applied.
 * CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a bad id or NULL options (the handle stays usable).  The launch plan and the captured
 * graph of the solve are untouched; with apply = 0 the state is bitwise unchanged.  A window may be uploaded with rho <= 0 on its new landmarks
 * for this purpose; solving such a state is the caller's error. */
int32_t ctvio_triangulate_batch(ctvio_solver *s, const ctvio_triangulate_options *o, double *depth, int32_t *flag);
int32_t ctvio_triangulate(ctvio_solver *s, int32_t id, const ctvio_triangulate_options *o, double *depth, int32_t *flag);
/* Depths in the frame of a new anchor observation: query i is landmark lm[i] of window win[i]; with p_i its current anchor point and camera
 * poses (row_times as above), depth_new[i] = z(R_new^T (R_old (p_i / rho) + P_old - P_new)) for the new anchor observation at absolute time
 * t_new[i], row row_new[i] (row_new may be NULL when row_times = 0) -- removeBackShiftDepth (feature_manager.cpp:370-377).
 *   flag 1: shifted;  2: the result was <= 0 and init_depth is returned;  3: not computable (rho <= 0, no single anchor, a time outside the
 *   spline), depth_new = NaN.  depth_new, flag: n entries, either may be NULL.  The state is never modified (only row_times and init_depth of the
 *   options are read).  CTVIO_ERR_INVALID for a window id or landmark index out of range, NULL options, NULL row_new with row_times = 1. */
int32_t ctvio_shift_anchor_batch(ctvio_solver *s, const ctvio_triangulate_options *o, int64_t n, const int32_t *win, const int32_t *lm,
                                 const int64_t *t_new, const int32_t *row_new, double *depth_new, int32_t *flag);

/* Batched trajectory query on the device: Se3Spline::poseNs / transVelWorld / rotVelBody / transAccelWorld
 * (se3_spline.h:361-399).  pose7 = (px,py,pz,qx,qy,qz,qw).  Any output may be NULL. */
int32_t ctvio_spline_eval(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_ns, double *pose7, double *vel3,
                          double *omega3, double *acc3);

/* The same queries for ANY windows of the batch in ONE launch (the per-row poses of rolling-shutter frames,
 * 11 x 640 row times per window, for a whole batch): query i belongs to window win[i] (0 .. ctvio_num_windows - 1) at absolute time
 * t_ns[i]; outputs in query order, laid out as in ctvio_spline_eval, any may be NULL.  Reference consumers: Se3Spline::poseNs /
 * transVelWorld / rotVelBody (se3_spline.h:361-399), Trajectory::GetSensorPose (trajectory.cpp:39-56) called once per time.
 * kernel_ms (may be NULL) receives the device time of the evaluation kernel alone (HIP events on the solver's stream); the call itself
 * also pays for the H2D copy of the queries and the D2H copy of the results. */
int32_t ctvio_spline_eval_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int64_t *t_ns, double *pose7, double *vel3,
                                double *omega3, double *acc3, double *kernel_ms);

/* Sensor pose on the device: Trajectory::GetSensorPose (src/spline/trajectory.cpp:39-56; used for the camera by
 * visual_odometry.cpp:197-221): pose_S_to_G(t) = poseNs(t) * T_StoI with T_StoI = (q_SI = (x,y,z,w), p_SI).  pose7 as above.
 * A query outside [minTimeNs, maxTimeNs) is an error (the reference asserts). */
int32_t ctvio_sensor_pose(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_ns, const double *q_SI, const double *p_SI, double *pose7);

/* Prior construction for the next window (reference MarginalizationInfo::preMarginalize / marginalize,
 * src/estimator/factor/analytic_diff/marginalization_factor.cpp:106-265, driven by TrajectoryEstimator::
 * PrepareMarginalizationInfo / SaveMarginalizationInfo, trajectory_estimator.cpp:143-204).  Window `id` holds the factors
 * to be dropped (IMU samples, visual blocks with cauchy_a = 1 as in the reference, bias chain, the previous prior) at the
 * linearisation point; its normal equations A = sum J~^T J~, b = sum J~^T r~ are assembled on the device by the linearise
 * kernels.  role[N] (N = 6K + 6F + 1 + L, the library's unknown order): 1 = marginalise, 0 = keep, -1 = not involved.
 * Output: n_keep, kept[n_keep] (unknown indices, ascending), J0 (n_keep x n_keep row-major) and r0 (n_keep) such that the
 * prior residual of the next window is r0 + J0 dx (ctvio_window.pJ0 / pr0, column j of J0 = unknown kept[j]).
 * kept / J0 / r0 must have room for N, N*N and N entries.  eps = 1e-8 in the reference (:26).  Use a CTVIO_FP64 solver when
 * the prior has to match an fp64 reference tightly: the elimination amplifies the fp32 noise of the default path. */
int32_t ctvio_marginalize(ctvio_solver *s, int32_t id, const int8_t *role, double eps, int32_t *n_keep, int32_t *kept, double *J0, double *r0);

/* The same for EVERY window of the batch, all on the device.  Windows with <= 180 marginalised and <= 180 kept unknowns share one
 * launch (one workgroup per window: Schur elimination + two parallel-Jacobi eigendecompositions in LDS); larger windows, up to 1024
 * marginalised and 1024 kept unknowns, take the blocked path one after the other (csrc/marg_blocked.hpp: block two-sided Jacobi, the
 * same convergence rule, deterministic).  Both may share a batch.  role: the windows' role arrays concatenated (sum of N_i entries,
 * window order); outputs: n_keep[n_windows]; kept: window i's kept unknowns at offset sum_{k<i} N_k; J0 / r0 packed tightly in window
 * order (offsets sum_{k<i} n_keep_k^2 / sum_{k<i} n_keep_k).  A window beyond 1024 is refused with CTVIO_ERR_INVALID (the handle stays
 * usable). */
int32_t ctvio_marginalize_batch(ctvio_solver *s, const int8_t *role, double eps, int32_t *n_keep, int32_t *kept, double *J0, double *r0);
/* Where the LAST ctvio_marginalize / ctvio_marginalize_batch call of this handle factored: 0 = on the device (the product path), 1 = the
 * eigen-decompositions ran on the HOST cores (csrc/marginalize.hpp: a window with more than 180 marginalised or kept unknowns, or one whose
 * in-LDS Jacobi sweeps stalled; ctvio_marginalize only -- the batch entry factors such windows on the device (blocked path) and never
 * sets it).  The normal equations come from the device kernels
 * either way.  Reference counterpart of the host leg: MarginalizationInfo::marginalize, marginalization_factor.cpp:178-265. */
int32_t ctvio_marginalize_ran_on_host(const ctvio_solver *s);

/* 4-DoF gauge restore after a solve, on the device, for n windows of the batch at once (reference
 * TrajectoryManager::double2vector, src/estimator/trajectory_manager.cpp:485-516, called at :467 right after Solve):
 * for window ids[i], the rigid transform that puts the yaw (full rotation near the Euler singularity) and the position
 * of knot knot[i] back to the pre-solve pose q0[i] = (x,y,z,w), t0[i] is applied to knots knot[i] .. K-1.
 * knot[i] = computeTIndexNs(timestamps[0]).second - index of the window's first knot (reference :324-329). */
int32_t ctvio_gauge_restore(ctvio_solver *s, int32_t n, const int32_t *ids, const int32_t *knot, const double *q0, const double *t0);

/* ---- every GPU of the node from one C / C++ process (windows are independent units; device g owns the windows
 * {w : w mod G = g}, one host thread + one solver handle / HIP stream per device, no inter-GPU traffic during the solves) ----
 * ctvio_solve_sharded: ctvio_set_batch + ctvio_solve + ctvio_get_batch_state of the n windows spread over n_devices devices
 * (0: all visible ones; device ordinals 0 .. n_devices - 1; opt->device is ignored).  out (n summaries) and the state arrays are in
 * the caller's WINDOW order, laid out like ctvio_get_batch_state (quat: sum K x 4, pos: sum K x 3, bias: sum F x 6, rho: sum L,
 * ld: n); any of them may be NULL.  The per-device handles and one persistent host thread per shard are created on first use and kept
 * for the next call (grow-only arenas, no thread creation per call); ctvio_sharded_release frees them.  One sharded solve at a time
 * per process (concurrent callers serialise on a mutex: use one solver handle per thread for concurrent batches).  Python ranks use torch.distributed + ctrl-vio_amd/sharding.py for the same rule. */
int32_t ctvio_solve_sharded(const ctvio_options *opt, int32_t n_devices, int32_t n, const ctvio_window *wins, int32_t max_iterations,
                            ctvio_summary *out, double *quat, double *pos, double *bias, double *rho, double *ld);
void ctvio_sharded_release(void);
/* The partition itself (no device needed): owner of window w, and how many of n windows device g gets -- for G shards.  The G a
 * call of ctvio_solve_sharded really uses is ctvio_shards_used(n_devices, n) = min(n_devices or all, devices present, n): pass THAT
 * to ctvio_shard_of / ctvio_shard_count when predicting owners.  Options: a call whose *opt differs from the one a kept handle was
 * created with gets a fresh handle (tolerances, deterministic, use_mfma, line_search ... take effect immediately).  Failures inside a
 * shard's host thread (HIP errors, std::bad_alloc) come back as that shard's status; nothing is thrown across the ABI. */
int32_t ctvio_shard_of(int32_t window_id, int32_t n_devices);
int32_t ctvio_shard_count(int32_t n, int32_t device, int32_t n_devices);
int32_t ctvio_shards_used(int32_t n_devices, int32_t n);

/* Kernel timing of the next ctvio_solve calls with HIP events recorded on the solver's stream around every
 * launch group (adds a few microseconds per launch: use a dedicated profiling solve, not the timed one). */
int32_t ctvio_set_profiling(ctvio_solver *s, int32_t on);
/* Timing of the last ctvio_solve.  ms8: accumulated device time [ms] per launch group
 *   0 k_imu_linearize  1 k_vis_eval (linearise)  2 k_assemble_vis  3 zero + k_assemble_imu + k_misc + k_post_linearize
 *   4 Schur SYRK (k_schur_window / k_schur_mfma)  5 k_cholesky_solve  6 everything else (damping, rhs, backsub, update, cost, control)
 *   7 whole solve (always measured).  launches8: number of launches of each group, [7] = LM passes launched.
 * Groups 0..6 are zero unless profiling was on.
 * After a covariance call instead: ms8[0..2] = device time of k_cov_prepare, k_cov_solve, k_cov_gram, ms8[7] = the whole call on the device
 * (linearisation, Schur complement and Cholesky included), the rest zero.
 * After a pose-covariance call: ms8[0..2] = device time of k_cov_prepare, k_cov_solve (substitution and the 6 x 6 blocks), k_cov_pose_jac,
 * ms8[7] = the whole call on the device, the rest zero.
 * After a landmark-points call: ms8[0..2] = device time of k_cov_prepare, k_cov_solve (substitution and the 3 x 3 blocks), k_cov_point_jac,
 * ms8[7] = the whole call on the device, the rest zero; points only (cov9 == NULL): ms8[0] = device time of k_cov_point_jac, ms8[7] = the whole
 * call on the device (its copy included), the rest zero.
 * After a navigation-state call: ms8[0..2] = device time of k_cov_prepare, k_cov_solve (substitution and the 15 x 15 blocks), k_cov_nav_jac,
 * ms8[7] = the whole call on the device, the rest zero; states only (cov225 == NULL): ms8[2] = device time of k_cov_nav_jac, ms8[7] = the
 * whole call on the device (its copies included), the rest zero.
 * After an IMU-prediction call: ms8[0..2] as after a navigation-state call, ms8[3] = device time of k_imu_propagate, ms8[7] = the whole call on
 * the device, the rest zero; states only (cov225 == NULL): ms8[2], ms8[3] and ms8[7].
 * After a landmark-projection call: ms8[0..2] = device time of k_cov_prepare, k_cov_solve (substitution, the 2 x 2 blocks and the gates),
 * k_cov_proj_jac, ms8[7] = the whole call on the device, the rest zero; values only (cov4 == NULL and chi2 == NULL): ms8[2] = device time of
 * k_cov_proj_jac, ms8[7] = the whole call on the device (its copies included), the rest zero.
 * After a body-rates call: ms8[0..2] = device time of k_cov_prepare, k_cov_solve (substitution, the 15 x 15 blocks and the gates),
 * k_cov_rates_jac, ms8[7] = the whole call on the device, the rest zero; values only (cov225 == NULL and chi2 == NULL): ms8[2] = device time
 * of k_cov_rates_jac, ms8[7] = the whole call on the device (its copies included), the rest zero.
 * After a landmark-prediction call: ms8[0..2] = device time of k_cov_prepare, k_cov_solve (substitution, the 2 x 2 blocks and the gates),
 * k_cov_pred_jac, ms8[3] = device time of k_imu_transition, ms8[7] = the whole call on the device, the rest zero; values only (cov4 == NULL
 * and chi2 == NULL): ms8[2], ms8[3] and ms8[7].
 * After a triangulation or anchor-shift call: ms8[0] = device time of k_triangulate / k_shift_anchor, ms8[7] = the whole call on the device
 * (its copies included), the rest zero. */
int32_t ctvio_last_timing(ctvio_solver *s, double *ms8, int32_t *launches8);
/* The HIP stream every kernel of this solver is launched on (hipStream_t), for external event timing. */
void *ctvio_stream(ctvio_solver *s);
/* How many times this handle captured its LM pass into a hipGraph so far (diagnostic: a stream of equally shaped batches captures
 * once; the launch sequence the reference replaces is ceres::Solve's per-iteration Evaluate loop, trajectory_estimator.cpp:399). */
int32_t ctvio_graph_captures(const ctvio_solver *s);

/* ---- Diagnostic switches.  libctvio.so reads a fixed set of environment variables ONCE per handle, inside ctvio_create (csrc/ctvio.hip:
 * DebugSwitches, the only getenv of the library), and never again: kernel selection cannot change between ctvio_upload and ctvio_solve.
 * They exist for A/B measurements and for the tests' cross-checks; production callers set none of them.
 *   CTVIO_DENSE=1 (dense sparsity plan)   CTVIO_CHOL_TILES=0|1|3   CTVIO_SCHUR_TILE2=0|1   CTVIO_SCHUR_COPY_PLAIN=1
 *   CTVIO_SPLIT_LINEARIZE=1   CTVIO_MARG_HOST=1   CTVIO_MARG_DEBUG=1   CTVIO_DEBUG_STAMPS=1
 *   CTVIO_MARG_BLOCKED=1 (ctvio_marginalize_batch: small windows through the blocked path too)
 *   CTVIO_SHARD_OVERSUBSCRIBE=1 (test only; read by ctvio_shards_used / ctvio_solve_sharded at call time)
 *   CTVIO_POISON=1|2 (test only: reused double scratch starts as quiet NaN / 2.6e151 at every upload and call, and ctvio_upload /
 *     ctvio_set_batch fail with CTVIO_ERR_INTERNAL if the packer leaves a staged input byte unwritten)
 *   CTVIO_CHOL_COMPACT=1|n (test only: every batch the panel Cholesky factors takes its slot-indexed variant, which otherwise runs only for
 *     windows beyond 591 unknowns; 1 = as many LDS slots as the batch needs, n >= 2 = at most n, the tiles beyond overflow to S)
 *   CTVIO_GATE_SLICE=n (test only: ctvio_visual_gate_batch walks its windows in slices of at most n block slots instead of 65536, and
 *     ctvio_imu_gate_batch in slices of at most n IMU samples instead of 49152) */

#ifdef __cplusplus
}
#endif
#endif /* CTVIO_H_ */
