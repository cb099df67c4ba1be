// kernels_cov.hpp -- covariances from the reduced system.  k_cov_prepare (per-call activity mask, zero damping), then one record kernel per
// entry and k_cov_solve (block forward substitution against 16 right-hand sides per workgroup, and the tile's covariance blocks):
//   ctvio_covariance_batch          selected block, var(rho)           k_cov_solve<COV_BASE> on TILE_SEL / TILE_RHO, k_cov_gram
//   ctvio_pose_covariance_batch     6 x 6 at query times               k_cov_pose_jac, k_cov_solve<COV_BASE> on TILE_POSE
//   ctvio_landmark_points_batch     world points, 3 x 3                k_cov_point_jac, k_cov_solve<COV_BASE> on TILE_POINT
//   ctvio_nav_state_batch           pose, velocity, biases, 15 x 15    k_cov_nav_jac, k_cov_solve<COV_BASE> on TILE_NAV (also ctvio_imu_predict_batch)
//   ctvio_relative_pose_batch       pose increments, 6 x 6             k_cov_rel_jac, k_cov_solve<COV_REL>
//   ctvio_project_landmarks_batch   image points, 2 x 2, gates         k_cov_proj_jac, k_cov_solve<COV_PROJ>
//   ctvio_body_rates_batch          body rates, 15 x 15, IMU gates     k_cov_rates_jac, k_cov_solve<COV_RATES>
//   ctvio_predict_landmarks_batch   points from IMU-predicted poses    k_cov_nav_jac, k_imu_transition (kernels_prop.hpp), k_cov_pred_jac, k_cov_solve<COV_PRED>
//   ctvio_visual_gate_batch         leave-one-out test of the blocks   k_cov_gate_jac, k_cov_solve<COV_GATE>, k_cov_gate_reduce
//   ctvio_imu_gate_batch            leave-one-out test of the samples  k_cov_imugate_jac, k_cov_solve<COV_IMUGATE>, k_cov_imugate_reduce
// Part of kernels.hpp (included from there, in order; not a stand-alone header).  With H the normal matrix of the window at its current
// state (no LM damping) and the excluded unknowns -- constant ones, and those no factor touches (H_jj == 0) -- removed, the reduced system
// S = Hpp - W Hll^-1 W^T = L L^T is factored by the panel kernel (k_cholesky_solve: L21 in S, the inverses of the 32 x 32 diagonal blocks in
// Dev::chol_inv).  Then
//   Sigma[i][j]     = (L^-1 e_i)^T (L^-1 e_j)                    for trajectory unknowns i, j,
//   Sigma[P+l][P+l] = 1 / Hll_l + | L^-1 (w_l / Hll_l) |^2        for the inverse depth of landmark l (w_l: its row of W),
//   Sigma_pose(t)   = J Sigma J^T = (L^-1 J^T)^T (L^-1 J^T)        for the 6 x P Jacobian J of the pose at time t (factors.hpp: pose_jac_T),
//   Cov(X_l)        = (L^-1 G)^T (L^-1 G) + j_rho j_rho^T / Hll_l   for the world point X_l of landmark l: G = Jp^T - w_l j_rho^T / Hll_l (P x 3), Jp
//                     the Jacobian of X_l against the trajectory unknowns, j_rho = dX_l / drho_l (the joint covariance of the trajectory and
//                     rho_l is Sigma_pp, Sigma_pl = -Sigma_pp w_l / Hll_l, Sigma_ll = 1 / Hll_l + w_l^T Sigma_pp w_l / Hll_l^2),
//   Sigma_nav(t, f) = (L^-1 J^T)^T (L^-1 J^T)                      for the 15 x P Jacobian J of (pose, world velocity, bias state f) at t (nav_jac_T),
//   Sigma_rel(a, b) = (L^-1 J^T)^T (L^-1 J^T)                      for the 6 x P Jacobian J = A_a J_a + A_b J_b of the increment T(t_a)^-1 T(t_b)
//                     (factors.hpp: rel_pose_jac_T; J_a, J_b the pose Jacobians at the two times),
//   Cov(proj)       = (L^-1 G)^T (L^-1 G) + j j^T / Hll_l           for the predicted image point of landmark l at a query time: Cov(X_l)'s identity
//                     with two columns, G = Jp^T - w_l j^T / Hll_l, Jp over the knots of the anchor time and of the query time and the line
//                     delay (factors.hpp: proj_jac_T, proj_cols), j = d(proj) / drho_l,
//   Sigma_rates(t, f) = (L^-1 J^T)^T (L^-1 J^T)   for the 15 x P Jacobian J of (omega, specific force, body-frame velocity, bias state f) at t (rates_jac_T),
//   Cov(pred)       = (L^-1 G)^T (L^-1 G) + j j^T / Hll_l + A N A^T  for the image point of landmark l seen from an IMU-predicted pose beyond the
//                     spline: Cov(proj)'s identity with Jp over the knots of the anchor time, the knots of the prediction's start time and its
//                     bias state (A Phi J_nav: the image point's row A pulled back through the propagation's transition Phi) and the line
//                     delay (factors.hpp: pred_A), plus the propagation's process noise N through A,
// so everything is a forward substitution Y = L^-1 B against many right-hand sides, 16 per workgroup, with Y resident in LDS.
#pragma once

namespace ctv {

// One right-hand-side tile: 16 columns of one window.
enum CovKind : int32_t {
  TILE_SEL = 0,     // one-hot columns of selected unknowns
  TILE_RHO = 1,     // rows of W (sorted landmark order) scaled by 1 / Hll
  TILE_POSE = 2,    // the six columns of J^T of one or two pose queries of the window (columns 6 q .. 6 q + 5)
  TILE_POINT = 3,   // the three columns of G of up to five landmarks (sorted landmark order, columns 3 q .. 3 q + 2, column 15 unused)
  TILE_NAV = 4,     // the fifteen columns of J^T of one navigation-state query (pose 0..5, velocity 6..8, gyro bias 9..11, accelerometer bias
                    // 12..14, column 15 unused)
  TILE_REL = 5,     // the six columns of J_rel^T of one or two relative-pose queries of the window (columns 6 q .. 6 q + 5)
  TILE_PROJ = 6,    // the two columns of G of up to eight projection queries of the window (columns 2 q, 2 q + 1)
  TILE_RATES = 7,   // the fifteen columns of J^T of one body-rates query (omega 0..2, specific force 3..5, body-frame velocity 6..8, gyro bias
                    // 9..11, accelerometer bias 12..14, column 15 unused)
  TILE_PRED = 8,    // the two columns of G of up to eight points of ctvio_predict_landmarks_batch (columns 2 q, 2 q + 1)
  TILE_GATE = 9,    // TILE_PROJ's columns for eight consecutive block slots of the window (ctvio_visual_gate_batch; built in the kernel, not listed)
  TILE_IMUGATE = 10 // the six columns of imu_w (.) J^T of one or two consecutive packed IMU samples of the window (columns 6 q .. 6 q + 5;
                    // ctvio_imu_gate_batch; built in the kernel from one descriptor per window, not listed)
};
struct CovTile {
  int32_t win;
  CovKind kind;
  int32_t first;    // SEL: offset of the tile's first entry in the concatenated selection; RHO and POINT: first row of W (window-local);
                    // POSE, REL, PROJ, PRED, GATE and IMUGATE: the tile's first query record; NAV and RATES: its query record
  int32_t count;    // columns in use (<= 16); POSE, REL and IMUGATE: queries (1 or 2); POINT: landmarks (<= 5); NAV and RATES: 1; PROJ, PRED and GATE: queries (<= 8)
  long long yoff;   // SEL: where the tile's Y ([P][16] doubles) goes in the scratch
};
// One window with a selection (k_cov_gram).
struct CovWin {
  int32_t win, nsel, sel0, pad;   // sel0: offset of its selection in the concatenated list
  long long y0, cov0;             // its first Y tile (tile t at y0 + 16 P t); its n_sel^2 block of the output
};

// Why a trajectory unknown is left out of the covariance's system (k_cov_prepare -> k_cov_gram).  Dev::active is 0 both for constant unknowns
// and for those no factor touches (host_pack.hpp: active_mask), so the two are told apart here: constant by the window's flags (fixed_upto,
// lock_bg / lock_ba, fix_ld), or inactive with H_jj != 0 (a per-knot constant that factors touch); untouched: H_jj == 0 exactly.
enum { COV_IN = 0, COV_CONSTANT = 1, COV_UNTOUCHED = 2 };

// Per call: the activity mask of the covariance (mask[j] = 1: unknown j is in the system) and the reason of every exclusion, zero damping,
// 1 / Hll by row of W.
__global__ __launch_bounds__(256) void k_cov_prepare(Dev d, uint8_t *mask, uint8_t *excl) {
  const int w = blockIdx.x;
  const WinMeta &m = d.wins[w];
  const int cur = d.lm[w].cur, K6 = 6 * m.K;
  const double *Hd = d.HppS[cur] + m.H0, *Hl = d.HllS[cur] + m.lm0;
  for (int j = threadIdx.x; j < m.N; j += blockDim.x) {
    const bool act = d.active[m.u0 + j] != 0;
    const double h = (j < m.P) ? Hd[(long long)j * m.ldh + j] : Hl[j - m.P];
    int why = COV_IN;
    if (j < m.P) {
      const bool flagged = j < K6 ? j / 6 <= m.fixed_upto : (j == m.P - 1 ? m.fix_ld != 0 : ((j - K6) % 6 < 3 ? m.lock_bg != 0 : m.lock_ba != 0));
      why = flagged ? COV_CONSTANT : (h == 0.0 ? COV_UNTOUCHED : (act ? COV_IN : COV_CONSTANT));
    }
    mask[m.u0 + j] = why == COV_IN ? 1 : 0;
    excl[m.u0 + j] = (uint8_t)why;
    d.dd[m.u0 + j] = 0.0;
    if (j >= m.P) {
      const int row = m.lm0 + d.lm_pos[m.lm0 + j - m.P];
      d.dinv[row] = h > 0.0 ? 1.0 / h : 0.0;   // (a landmark without observations: Hll = 0, its row of W is zero)
      d.grs[row] = 0.0;   // (the reduced right-hand side rides through the factorisation; nothing here reads it)
    }
  }
}

// ---- what the record kernels (k_cov_*_jac) share
// The segment of a time t_rel (relative to the window's t0) by the integer-ns rule of k_spline_eval (reference spline_segment.h:83-85):
// first knot s = t_rel / dt_ns, u = (t_rel % dt_ns) / dt_ns from one remainder and one division, and nk, the knots a value at t_rel depends
// on: 3 at u = 0 (the last blending weights are multiples of u), else 4.  Outside the spline (t_rel < 0 or s + 3 >= K) s = 0 and u = 0: the
// loads stay in range and the value is not used.
struct CovSeg { int s, nk; double u; bool outside; };
__device__ __forceinline__ CovSeg cov_segment(const WinMeta &m, long long t_rel) {
  const long long sl = t_rel / m.dt_ns;
  CovSeg g;
  g.outside = t_rel < 0 || sl + 3 >= m.K;
  g.s = g.outside ? 0 : (int)sl;
  g.u = g.outside ? 0.0 : (double)(t_rel % m.dt_ns) / (double)m.dt_ns;
  g.nk = g.u > 0.0 ? 4 : 3;
  return g;
}
// Whether one of the knots s .. s + nk - 1, or the bias state `frame`, has an unknown that no factor touches (k_cov_prepare: COV_UNTOUCHED
// on any of its six unknowns).  Decided on the exclusion flags and on u > 0 (nk), never on a Jacobian entry.  The caller names the status:
// POSE_UNTOUCHED, IMUG_NO_INFO or PRJ_NO_INFO.  Several tests are joined with |, not ||: every flag is loaded, no load waits for a result.
__device__ __forceinline__ bool cov_untouched(const uint8_t *excl, const WinMeta &m, int j0, int n) {
  bool hit = false;
  for (int j = j0; j < j0 + n; ++j)
    if (excl[m.u0 + j] == COV_UNTOUCHED) hit = true;
  return hit;
}
__device__ __forceinline__ bool cov_untouched_knots(const uint8_t *excl, const WinMeta &m, int s, int nk) { return cov_untouched(excl, m, 6 * s, 6 * nk); }
__device__ __forceinline__ bool cov_untouched_bias(const uint8_t *excl, const WinMeta &m, int frame) { return cov_untouched(excl, m, 6 * (m.K + frame), 6); }
// What the records of the one-sided entries begin with (k_cov_solve reads it under these names): first knot, knots the value depends on
// (cov_segment), the bias state -- 0 where the entry has none (PoseRec, PointRec).  The two-sided records (RelRec, ProjRec, GateRec,
// PredRec) have headers of their own.  CTV_REC_LAYOUT: a record is laid out as k_cov_solve reads it -- the header at offset 0, jt where it
// has always been (offsetof through the base is well defined for these plain structs; the compiler's remark about it is silenced).
struct CovRecHead { int32_t status, s, nk, frame; };
__device__ __forceinline__ void cov_rec_head(CovRecHead &r, int status, int s, int nk, int frame) { r.status = status; r.s = s; r.nk = nk; r.frame = frame; }
#define CTV_REC_LAYOUT(Rec, jt_off, bytes)                                                                                                            \
  _Pragma("clang diagnostic push") _Pragma("clang diagnostic ignored \"-Winvalid-offsetof\"")                                                         \
  static_assert(sizeof(CovRecHead) == 16 && sizeof(Rec) == (bytes) && __builtin_offsetof(Rec, status) == 0 && __builtin_offsetof(Rec, frame) == 12 && \
                __builtin_offsetof(Rec, jt) == (jt_off), #Rec ": the layout k_cov_solve reads");                                                      \
  _Pragma("clang diagnostic pop") static_assert(true, "")

// One pose query (ctvio_pose_covariance_batch), grouped by window on the host, and what k_cov_pose_jac makes of it.
enum { POSE_OK = 0, POSE_SINGULAR = 1, POSE_UNTOUCHED = 2, POSE_OUTSIDE = 3 };   // the statuses of ctvio.h (1 is the host's: Lm::chol_fail)
struct PoseQuery {
  int32_t win, pad;
  long long t_rel;   // relative to the window's t0
};
struct PoseRec : CovRecHead {
  double jt[144];   // J^T, rows of knots s .. s + 3 (pose_jac_T; written for POSE_OK only)
};
CTV_REC_LAYOUT(PoseRec, 16, 16 + 8 * 144);

// One lane per query: the segment (cov_segment), the status, and J^T at the current state.  A knot the pose depends on that no factor
// touches gives POSE_UNTOUCHED (cov_untouched_knots).
__global__ __launch_bounds__(64) void k_cov_pose_jac(Dev d, int n, const PoseQuery *qs, const uint8_t *excl, SensorExt ext, PoseRec *recs, int32_t *status_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PoseQuery q = qs[i];
  const WinMeta &m = d.wins[q.win];
  const CovSeg g = cov_segment(m, q.t_rel);
  int status = g.outside ? POSE_OUTSIDE : POSE_OK;
  if (!g.outside && cov_untouched_knots(excl, m, g.s, g.nk)) status = POSE_UNTOUCHED;
  PoseRec &r = recs[i];
  cov_rec_head(r, status, g.s, g.nk, 0);
  status_out[i] = status;
  if (status != POSE_OK) return;
  const double zero3[3] = {0, 0, 0};
  Knots4 k;
  load_knots(d.quat, d.pos, m.knot0 + g.s, zero3, k);
  SegConst sc;
  seg_const(k, sc, true);
  pose_jac_T(k.q, sc, g.u, ext.on != 0, qmk(ext.q[0], ext.q[1], ext.q[2], ext.q[3]), mk(ext.p[0], ext.p[1], ext.p[2]), r.jt);
}

// One navigation-state query (ctvio_nav_state_batch), grouped by window on the host, and what k_cov_nav_jac makes of it.  The statuses are
// the pose entry's (POSE_*).
struct NavQuery {
  int32_t win, frame;   // frame: the bias state, in [0, F) (the host has resolved "the newest")
  long long t_rel;      // relative to the window's t0
};
struct NavRec : CovRecHead {
  double cv[4];     // c'_k(u) / dt: the velocity rows against the position unknowns of knots s .. s + 3
  double jt[144];   // the pose block of J^T, rows of knots s .. s + 3 (nav_jac_T; with cv written for POSE_OK only)
};
CTV_REC_LAYOUT(NavRec, 48, 48 + 8 * 144);

// One lane per query: the segment (cov_segment), the state -- position and orientation, world velocity (the device functions of
// k_spline_eval), the six biases of state `frame` -- into state16 (NaN outside the spline), and with excl (after k_cov_prepare; null: values
// only, recs is not touched) the status and the record.  A knot the state depends on, or the bias state, that no factor touches gives
// POSE_UNTOUCHED (cov_untouched_knots, cov_untouched_bias).  The values are formed before excl is looked at: both calls give them the same bits.
__global__ __launch_bounds__(64) void k_cov_nav_jac(Dev d, int n, const NavQuery *qs, const uint8_t *excl, NavRec *recs, double *state16, int32_t *status_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const NavQuery q = qs[i];
  const WinMeta &m = d.wins[q.win];
  const CovSeg g = cov_segment(m, q.t_rel);
  const double u = g.u;
  const bool outside = g.outside;
  int status = outside ? POSE_OUTSIDE : POSE_OK;
  const double zero3[3] = {0, 0, 0};
  Knots4 k;
  load_knots(d.quat, d.pos, m.knot0 + g.s, zero3, k);
  SegConst sc;
  seg_const(k, sc, excl != nullptr);
  {
    const double nan = qnan();
    double c[4], dc[4];
    basis<false, 0>(u, 1.0, c);
    basis<false, 1>(u, m.inv_dt, dc);
    V3 p = mk(0, 0, 0), v = mk(0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) { p = p + c[j] * k.p[j]; v = v + dc[j] * k.p[j]; }
    const Q4 qq = eval_R(k.q, sc, u);
    const double *bp = d.bias + 6 * (size_t)(m.bias0 + q.frame);
    double *o = state16 + 16 * (size_t)i;
    const double val[10] = {p.x, p.y, p.z, qq.x, qq.y, qq.z, qq.w, v.x, v.y, v.z};
#pragma unroll
    for (int j = 0; j < 10; ++j) o[j] = outside ? nan : val[j];
#pragma unroll
    for (int j = 0; j < 6; ++j) o[10 + j] = outside ? nan : bp[j];
  }
  if (!excl) {
    status_out[i] = status;
    return;
  }
  if (!outside && (cov_untouched_knots(excl, m, g.s, g.nk) | cov_untouched_bias(excl, m, q.frame))) status = POSE_UNTOUCHED;
  NavRec &r = recs[i];
  cov_rec_head(r, status, g.s, g.nk, q.frame);
  status_out[i] = status;
  if (status != POSE_OK) return;
  nav_jac_T(k.q, sc, u, m.inv_dt, r.jt, r.cv);
}

// One body-rates query (ctvio_body_rates_batch), grouped by window on the host, and what k_cov_rates_jac makes of it.  The statuses are the
// pose entry's (POSE_*).
struct RatesQuery {
  int32_t win, frame;   // frame: the bias state, in [0, F) (the host has resolved "the newest")
  long long t_rel;      // relative to the window's t0
  double meas[6];       // the candidate IMU sample of the gate, gyro then accelerometer (zeros without one)
  double sig[6];        // its six standard deviations (the host has resolved noise6 == NULL to 1 / imu_w; ones without a gate)
};
struct RatesRec : CovRecHead {
  double z[6];              // the predicted reading (omega + bg_f, f + ba_f), from the bits that go to rates9
  double meas[6], sig[6];   // the query's
  double jt[216];           // J^T over the knots s .. s + 3, 24 x 9 (rates_jac_T; written for POSE_OK only)
};
CTV_REC_LAYOUT(RatesRec, 160, 160 + 8 * 216);

// One lane per query: the segment (cov_segment), the values -- omega (eval_omega), f = R(t)^T (p''(t) + g), v_B = R(t)^T v_W(t) -- into
// rates9 (NaN outside the spline), and with excl (after k_cov_prepare; null: values only, recs is not touched) the status and the record.
// A knot the rates depend on, or the bias state, that no factor touches gives POSE_UNTOUCHED (cov_untouched_knots, cov_untouched_bias).
// The values are formed before excl is looked at, by code the Jacobians do not share: both calls give them the same bits.
// (The values are rates_values, shared with k_cov_imugate_jac: segment s and u in, the knots relative to knot s, the segment's constants --
// with want_jac those the Jacobian needs as well --, gravity and val = (omega, f, v_B) out.)
__device__ __forceinline__ void rates_values(const Dev &d, const WinMeta &m, int s, double u, bool want_jac, Knots4 &k, SegConst &sc, V3 &grav, double *val) {
  load_knots(d.quat, d.pos, m.knot0 + s, d.pos + 3 * (size_t)(m.knot0 + s), k);   // relative to knot s: the rates are translation invariant
  seg_const(k, sc, want_jac);
  grav = mk(m.gravity[0], m.gravity[1], m.gravity[2]);
  double dc[4], ddc[4];
  basis<false, 1>(u, m.inv_dt, dc);
  basis<false, 2>(u, m.inv_dt * m.inv_dt, ddc);
  V3 v = mk(0, 0, 0), a = mk(0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) { v = v + dc[j] * k.p[j]; a = a + ddc[j] * k.p[j]; }
  const Q4 qinv = qconj(eval_R(k.q, sc, u));
  const V3 om = eval_omega<SegConst>(sc, u, m.inv_dt), f = qrot(qinv, a + grav), vb = qrot(qinv, v);
  val[0] = om.x; val[1] = om.y; val[2] = om.z; val[3] = f.x; val[4] = f.y; val[5] = f.z; val[6] = vb.x; val[7] = vb.y; val[8] = vb.z;
}
__global__ __launch_bounds__(64) void k_cov_rates_jac(Dev d, int n, const RatesQuery *qs, const uint8_t *excl, RatesRec *recs, double *rates9, int32_t *status_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const RatesQuery &q = qs[i];
  const int frame = q.frame;
  const WinMeta &m = d.wins[q.win];
  const CovSeg g = cov_segment(m, q.t_rel);
  const double u = g.u;
  const bool outside = g.outside;
  int status = outside ? POSE_OUTSIDE : POSE_OK;
  Knots4 k;
  SegConst sc;
  V3 grav;
  double val[9];
  rates_values(d, m, g.s, u, excl != nullptr, k, sc, grav, val);
  {
    const double nan = qnan();
    double *o = rates9 + 9 * (size_t)i;
#pragma unroll
    for (int j = 0; j < 9; ++j) o[j] = outside ? nan : val[j];
  }
  if (!excl) {
    status_out[i] = status;
    return;
  }
  if (!outside && (cov_untouched_knots(excl, m, g.s, g.nk) | cov_untouched_bias(excl, m, frame))) status = POSE_UNTOUCHED;
  RatesRec &r = recs[i];
  cov_rec_head(r, status, g.s, g.nk, frame);
  status_out[i] = status;
  if (status != POSE_OK) return;
  const double *bp = d.bias + 6 * (size_t)(m.bias0 + frame);
#pragma unroll
  for (int j = 0; j < 6; ++j) { r.z[j] = val[j] + bp[j]; r.meas[j] = q.meas[j]; r.sig[j] = q.sig[j]; }
  rates_jac_T(k, sc, u, m.inv_dt, grav, r.jt);
}

// One IMU sample of the window itself (ctvio_imu_gate_batch) and what k_cov_imugate_jac makes of it.  The statuses: 2 as POSE_UNTOUCHED,
// 4 the epilogue's (redundancy < min_redundancy); 3 cannot occur, the upload refuses IMU times outside the spline.
enum { IMUG_OK = 0, IMUG_SINGULAR = 1, IMUG_NO_INFO = 2, IMUG_WEAK = 4 };   // the statuses of ctvio.h (1 is the host's: Lm::chol_fail)
constexpr int IMUG_PER_TILE = 2;
struct ImuGateRec : CovRecHead {
  double r[6];      // the whitened residual, the bits that go to res6
  double jt[144];   // the omega and f columns of J^T over the knots s .. s + 3, 24 x 6, unweighted (rates_jac_T<.., 6>; IMUG_OK only)
};
CTV_REC_LAYOUT(ImuGateRec, 64, 64 + 8 * 144);
// What the gate's kernels write per packed sample slot (absolute slot - slot0; null: not asked for) and the threshold of IMUG_WEAK.
struct ImuGateOut {
  double *res6, *red, *cov36, *chi2;
  int32_t *status;
  int32_t slot0, pad;
  double min_red;
};
// One lane per packed sample slot e = first + i of the slice (records by i, outputs by e - slot0): segment and bias state of the sample's
// group, u = imu_u (the host's integer-ns rule, the one k_cov_rates_jac applies to a query time), z = rates_values + bias, and
// r = imu_w (z - meas), every operation rounded once, so that the residual can be re-derived from ctvio_body_rates' values to the bit.
// With excl (after k_cov_prepare; null: values only, recs is not touched) the status -- a knot the sample depends on, or its bias state,
// that no factor touches gives IMUG_NO_INFO (cov_untouched_knots, cov_untouched_bias) -- and the record.  The values are formed before
// excl is looked at: both calls give them the same bits.
__global__ __launch_bounds__(64) void k_cov_imugate_jac(Dev d, int first, int n, const uint8_t *excl, ImuGateRec *recs, ImuGateOut o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int e = first + i;
  const ImuGroup &g = d.groups[d.imu_grp[e]];
  const WinMeta &m = d.wins[g.win];
  const int s = g.s, frame = g.bias;
  const double u = d.imu_u[e];
  const int nk = u > 0.0 ? 4 : 3;
  Knots4 k;
  SegConst sc;
  V3 grav;
  double val[9], r[6];
  rates_values(d, m, s, u, excl != nullptr, k, sc, grav, val);
  const double *bp = d.bias + 6 * (size_t)(m.bias0 + frame);
#pragma unroll
  for (int j = 0; j < 6; ++j) r[j] = __dmul_rn(m.imu_w[j], __dsub_rn(__dadd_rn(val[j], bp[j]), d.imu_meas[(size_t)j * d.Mtot + e]));
  const size_t ko = (size_t)(e - o.slot0);
  if (o.res6) {
#pragma unroll
    for (int j = 0; j < 6; ++j) o.res6[6 * ko + j] = r[j];
  }
  int status = IMUG_OK;
  if (excl && (cov_untouched_knots(excl, m, s, nk) | cov_untouched_bias(excl, m, frame))) status = IMUG_NO_INFO;
  o.status[ko] = status;
  if (!excl) return;
  ImuGateRec &rc = recs[i];
  cov_rec_head(rc, status, s, nk, frame);
#pragma unroll
  for (int j = 0; j < 6; ++j) rc.r[j] = r[j];
  if (status != IMUG_OK) return;
  rates_jac_T<SegConst, 6>(k, sc, u, m.inv_dt, grav, rc.jt);
}

// One lane per bias state f_base + i (absolute; outputs by i): over the IMU groups that name it (Dev::bgl, group order) and their samples in
// slot order -- the upload's packed order, so the bits are the window's -- the number of status-0 samples, the mean of their chi2 (NaN:
// none), the largest chi2 (0: none) and the smallest redundancy over status 0 or 4 (+inf: none).  A window whose factorisation failed
// (chol_fail) has none of them.
__global__ __launch_bounds__(64) void k_cov_imugate_reduce(Dev d, int f_base, int n, ImuGateOut o, double *stats4) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int fa = f_base + i, w = d.bias_win[fa];
  const bool bad = d.lm[w].chol_fail != 0;
  const int32_t *off = d.bgl_off + fa + w;   // (window w's F + 1 offsets start at bias0 + w)
  int c = 0;
  double sum = 0.0, cmax = 0.0, rmin = __builtin_inf();
  for (int gi = off[0]; gi < off[1] && !bad; ++gi) {
    const ImuGroup &g = d.groups[d.bgl[gi]];
    for (int j = 0; j < g.count; ++j) {
      const size_t k = (size_t)(g.iabs + j - o.slot0);
      const int st = o.status[k];
      if (st == IMUG_OK) { ++c; sum = __dadd_rn(sum, o.chi2[k]); cmax = fmax(cmax, o.chi2[k]); }
      if (st == IMUG_OK || st == IMUG_WEAK) rmin = fmin(rmin, o.red[k]);
    }
  }
  stats4[4 * (size_t)i] = (double)c;
  stats4[4 * (size_t)i + 1] = c ? sum / (double)c : qnan();
  stats4[4 * (size_t)i + 2] = cmax;
  stats4[4 * (size_t)i + 3] = rmin;
}

// One relative-pose query (ctvio_relative_pose_batch), grouped by window on the host, and what k_cov_rel_jac makes of it.  The statuses are
// the pose entry's (POSE_*).
struct RelQuery {
  int32_t win, pad;
  long long ta_rel, tb_rel;   // relative to the window's t0
};
struct RelRec {
  int32_t status, s_a, nk_a, s_b, nk_b, pad;   // per time: first knot; knots the pose depends on (3 at u = 0, else 4)
  double jt_a[144], jt_b[144];                 // the two blocks of J_rel^T: (A_a J_a)^T over knots s_a .. s_a + 3, (A_b J_b)^T over knots s_b .. s_b + 3
                                               // (rel_pose_jac_T; written for POSE_OK only)
};

// The pose of one time of a relative-pose query: the segment (cov_segment), T_I(t), or T_I(t) T_SI with the extrinsic; with jt the 24 x 6
// block of pose_jac_T as well.
__device__ inline void rel_side(const Dev &d, const WinMeta &m, long long t_rel, const SensorExt &ext, double *jt, int &s, int &nk, bool &outside, Q4 &qo, V3 &po) {
  const CovSeg g = cov_segment(m, t_rel);
  s = g.s; nk = g.nk; outside = g.outside;
  const double u = g.u;
  const double zero3[3] = {0, 0, 0};
  Knots4 k;
  load_knots(d.quat, d.pos, m.knot0 + s, zero3, k);
  SegConst sc;
  seg_const(k, sc, jt != nullptr);
  double c[4];
  basis<false, 0>(u, 1.0, c);
  V3 p = mk(0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) p = p + c[j] * k.p[j];
  const Q4 q = eval_R(k.q, sc, u);
  const Q4 q_SI = qmk(ext.q[0], ext.q[1], ext.q[2], ext.q[3]);
  const V3 p_SI = mk(ext.p[0], ext.p[1], ext.p[2]);
  qo = ext.on ? qmul(q, q_SI) : q;
  po = ext.on ? p + qrot(q, p_SI) : p;
  if (jt) pose_jac_T(k.q, sc, u, ext.on != 0, q_SI, p_SI, jt);
}

// One lane per query: the two poses, the increment (p_ab, q_ab) into rel7 (NaN where either time is outside the spline), and with excl
// (after k_cov_prepare; null: values only, recs is not touched) the status and the record.  A knot either pose depends on that no factor
// touches gives POSE_UNTOUCHED (cov_untouched_knots).  The values are formed before excl is looked at, by code the Jacobians do not
// share: both calls give them the same bits.
__global__ __launch_bounds__(64) void k_cov_rel_jac(Dev d, int n, const RelQuery *qs, const uint8_t *excl, SensorExt ext, RelRec *recs, double *rel7, int32_t *status_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const RelQuery q = qs[i];
  const WinMeta &m = d.wins[q.win];
  int s_a, nk_a, s_b, nk_b;
  bool out_a, out_b;
  Q4 q_a, q_b, q_ab;
  V3 p_a, p_b, p_ab;
  rel_side(d, m, q.ta_rel, ext, nullptr, s_a, nk_a, out_a, q_a, p_a);
  rel_side(d, m, q.tb_rel, ext, nullptr, s_b, nk_b, out_b, q_b, p_b);
  const bool outside = out_a || out_b;
  int status = outside ? POSE_OUTSIDE : POSE_OK;
  rel_pose_jac_T(q_a, p_a, q_b, p_b, nullptr, nullptr, q_ab, p_ab);
  if (rel7) {
    const double nan = qnan();
    const double val[7] = {p_ab.x, p_ab.y, p_ab.z, q_ab.x, q_ab.y, q_ab.z, q_ab.w};
#pragma unroll
    for (int j = 0; j < 7; ++j) rel7[7 * (size_t)i + j] = outside ? nan : val[j];
  }
  if (!excl) {
    status_out[i] = status;
    return;
  }
  if (!outside && (cov_untouched_knots(excl, m, s_a, nk_a) | cov_untouched_knots(excl, m, s_b, nk_b))) status = POSE_UNTOUCHED;
  RelRec &r = recs[i];
  r.status = status; r.s_a = s_a; r.nk_a = nk_a; r.s_b = s_b; r.nk_b = nk_b; r.pad = 0;
  status_out[i] = status;
  if (status != POSE_OK) return;
  rel_side(d, m, q.ta_rel, ext, r.jt_a, s_a, nk_a, out_a, q_a, p_a);
  rel_side(d, m, q.tb_rel, ext, r.jt_b, s_b, nk_b, out_b, q_b, p_b);
  rel_pose_jac_T(q_a, p_a, q_b, p_b, r.jt_a, r.jt_b, q_ab, p_ab);
}

// One landmark's world point (ctvio_landmark_points_batch) and what k_cov_point_jac makes of it.  Records are indexed by landmark through the
// batch (lm0 + l, the caller's order).
enum { LMP_OK = 0, LMP_SINGULAR = 1, LMP_NO_INFO = 2, LMP_NONE = 3 };   // the statuses of ctvio.h (1 is the host's: Lm::chol_fail)
constexpr int LMP_PER_TILE = 5;
struct PointRec : CovRecHead {    // (s, nk: of the anchor time)
  double X[3], jrho[3], jld[3];   // the point, dX / drho, dX / d(line delay)
  double jt[72];                  // Jp^T, rows of knots s .. s + 3: jt[3 r + a] = dX_a / d(unknown 6 s + r) (written with the Jacobians, LMP_OK only)
};
CTV_REC_LAYOUT(PointRec, 88, 88 + 8 * 72);

// One lane per landmark l_begin + i < l_begin + l_count: the anchor observation (t_i, row_i, p_i) its blocks share -- read as k_triangulate
// reads it --, the camera pose T_I(tau) (q_CI, p_CI) at tau = t_i + row_i * line delay (vis_times), X = R_C (p_i / rho) + p_C.  LMP_NONE
// by the rules of k_shift_anchor: rho <= 0 or non-finite, no block, blocks naming several anchors, tau outside the spline.  With want_jac
// (after k_cov_prepare: d.dinv holds 1 / Hll by row of W, 0 where Hll == 0 -> LMP_NO_INFO) the record takes j_rho = -R_C p_i / rho^2, the
// line-delay column row_i (R_I [omega]x p_I + v) -- the formal derivative the visual factor uses (factors.hpp: vis_anchor_eval, h) -- and
// Jp^T = ([-R_C [x_c]x, I] J_pose)^T from pose_jac_T with the extrinsic on.  The point is formed before the flag is looked at: both calls
// give it the same bits.  point3 / status_out: [l_count], either may be null.
__global__ __launch_bounds__(64) void k_cov_point_jac(Dev d, int l_begin, int l_count, int want_jac, PointRec *recs, double *point3, int32_t *status_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= l_count) return;
  const int l = l_begin + i, w = d.lm_win[l];
  const WinMeta &m = d.wins[w];
  const double rho = d.rho[l];
  const int first = d.lm_vfirst[l], cnt = d.lm_vcnt[l];
  bool ok = rho > 0.0 && isfinite(rho) && cnt > 0;
  int a0 = m.anc0;
  if (cnt > 0) {
    a0 = d.v_anc[first];
    for (int j = 1; j < cnt; ++j) ok = ok && d.v_anc[first + j] == a0;
  }
  const int row = cnt > 0 ? d.a_row[a0] : 0;
  int s = 0;
  double u = 0.0;
  if (cnt > 0) vis_times(m, d.a_t[a0], row, d.ld[w], s, u);
  ok = ok && s >= 0 && u >= 0.0 && s <= m.K - 4;   // (a negative time truncates towards zero: s <= 0 and u <= 0)
  s = max(0, min(s, m.K - 4));                     // the loads stay in range either way
  const int nk = u > 0.0 ? 4 : 3;
  int status = ok ? LMP_OK : LMP_NONE;
  if (ok && want_jac && d.dinv[m.lm0 + d.lm_pos[l]] == 0.0) status = LMP_NO_INFO;
  const double zero3[3] = {0, 0, 0};
  Knots4 k;
  load_knots(d.quat, d.pos, m.knot0 + s, zero3, k);
  SegConst sc;
  seg_const(k, sc, want_jac != 0);
  const Q4 q_CI = qmk(m.q_CI[0], m.q_CI[1], m.q_CI[2], m.q_CI[3]);
  const V3 p_CI = mk(m.p_CI[0], m.p_CI[1], m.p_CI[2]);
  const double px = cnt > 0 ? d.a_obs[a0] : 0.0, py = cnt > 0 ? d.a_obs[(size_t)d.Atot + a0] : 0.0, z = 1.0 / rho;
  const V3 x_c = mk(px * z, py * z, z);
  double c[4];
  basis<false, 0>(u, 1.0, c);
  V3 pI = mk(0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) pI = pI + c[j] * k.p[j];
  const Q4 qI = eval_R(k.q, sc, u);
  const M3 RI = q2R(qI), RC = q2R(qmul(qI, q_CI));
  const V3 X = mul(RC, x_c) + (pI + qrot(qI, p_CI));
  const double nan = qnan();
  if (point3) { point3[3 * i] = ok ? X.x : nan; point3[3 * i + 1] = ok ? X.y : nan; point3[3 * i + 2] = ok ? X.z : nan; }
  if (status_out) status_out[i] = status;
  if (!want_jac) return;
  PointRec &r = recs[l];
  cov_rec_head(r, status, s, nk, 0);
  r.X[0] = X.x; r.X[1] = X.y; r.X[2] = X.z;
  if (status != LMP_OK) return;
  const V3 jr = (-z * z) * mul(RC, mk(px, py, 1.0));
  r.jrho[0] = jr.x; r.jrho[1] = jr.y; r.jrho[2] = jr.z;
  {   // the line-delay column
    double dc[4];
    basis<false, 1>(u, m.inv_dt, dc);
    V3 v = mk(0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) v = v + dc[j] * k.p[j];
    const V3 p_I = qrot(q_CI, x_c) + p_CI;
    const V3 jl = (double)row * (mul(RI, cross(eval_omega<SegConst>(sc, u, m.inv_dt), p_I)) + v);
    r.jld[0] = jl.x; r.jld[1] = jl.y; r.jld[2] = jl.z;
  }
  double jp[144];
  pose_jac_T(k.q, sc, u, true, q_CI, p_CI, jp);
  const M3 Mx = scale(mul_hat(RC, x_c), -1.0);   // -R_C [x_c]x
  for (int rr = 0; rr < 24; ++rr)
#pragma unroll
    for (int a = 0; a < 3; ++a)
      r.jt[3 * rr + a] = Mx.m[3 * a] * jp[6 * rr] + Mx.m[3 * a + 1] * jp[6 * rr + 1] + Mx.m[3 * a + 2] * jp[6 * rr + 2] + jp[6 * rr + 3 + a];
}

// One projection query (ctvio_project_landmarks_batch), grouped by window on the host, and what k_cov_proj_jac makes of it.
enum { PRJ_OK = 0, PRJ_SINGULAR = 1, PRJ_NO_INFO = 2, PRJ_NONE = 3 };   // the statuses of ctvio.h (1 is the host's: Lm::chol_fail)
constexpr int PRJ_PER_TILE = 8;
struct ProjQuery {
  int32_t win, lm, row, pad;   // lm: the caller's landmark index in the window; row: the image row, or the first guess of the row iteration
  long long t_rel;             // the frame time relative to the window's t0
  double obs[2];               // the candidate point of the gate (zeros without one)
};
struct ProjRowModel { double fy, cy; int32_t rows, iterations; };   // ctvio_row_model; iterations == 0: the rows are used as given
struct ProjRec {
  int32_t status, s_a, nk_a, s_q, nk_q, wrow;   // per time (anchor, query): first knot; knots the pose depends on (3 at u = 0, else 4); wrow: the
                                                // landmark's sorted row of W (window-local)
  double proj[2], obs[2];                       // the prediction as returned in proj3, the candidate point
  double j[2], jld[2];                          // d(proj) / drho; d(proj) / d(line delay), both times summed (proj_cols)
  double jt_a[48], jt_q[48];                    // the two 24 x 2 blocks of Jp^T over knots s_a .. s_a + 3 and s_q .. s_q + 3 (proj_jac_T)
                                                // (j, jld, jt_a, jt_q: written for PRJ_OK only)
};

// The body pose at tau (inside the spline, as the caller has established: of cov_segment only s and u are used), the body rate and world
// velocity there, and the 24 x 6 block of pose_jac_T for the camera pose.
__device__ inline void proj_side(const Dev &d, const WinMeta &m, long long tau, Q4 q_CI, V3 p_CI, double *jp, Q4 &q_I, V3 &om, V3 &v) {
  const CovSeg g = cov_segment(m, tau);
  const double u = g.u;
  const double zero3[3] = {0, 0, 0};
  Knots4 k;
  load_knots(d.quat, d.pos, m.knot0 + g.s, zero3, k);
  SegConst sc;
  seg_const(k, sc, true);
  q_I = eval_R(k.q, sc, u);
  double dc[4];
  basis<false, 1>(u, m.inv_dt, dc);
  v = mk(0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) v = v + dc[j] * k.p[j];
  om = eval_omega<SegConst>(sc, u, m.inv_dt);
  pose_jac_T(k.q, sc, u, true, q_CI, p_CI, jp);
}

// One lane per query: the anchor observation of the landmark as k_cov_point_jac reads it and the camera pose at its row time; the camera pose
// at tau_q = t + row * line delay (integer ns, vis_times' rule) and y = R_Cq^T (X - p_Cq).  With a row model (rm.iterations > 0) the row is
// first iterated: y at the current row, then row <- clamp(rint(fy y.y / y.z + cy), 0, rows - 1); value and Jacobian are taken at the final row.
// PRJ_NONE: the landmark is not computable (k_cov_point_jac's rules), or at any row visited tau_q is outside the spline or y.z <= 0 or y is
// not finite; the iteration stops there, the loads stay in range (rel_side: s = 0 outside the spline), proj3 is NaN and row_out -1.  The value
// is formed before excl is looked at, by code the Jacobians do not share: the values-only call (excl null; recs is not touched) gives it the
// same bits.  With excl (after k_cov_prepare) the status and the record: PRJ_NO_INFO where 1 / Hll == 0 (d.dinv) or a knot either time
// depends on is one no factor touches (cov_untouched_knots).  The anchor block is formed in the 144-double pose buffer and stored, then
// the buffer is reused for the query block.
// (The lane's work is proj_query, shared with k_cov_gate_jac: out3 = the query's proj3, the return value its status; r is written with excl only.)
__device__ __forceinline__ int proj_query(const Dev &d, const ProjQuery &q, const uint8_t *excl, const ProjRowModel &rm, ProjRec *rp, double *out3, int &row_o) {
  const int w = q.win;
  const WinMeta &m = d.wins[w];
  const int l = m.lm0 + q.lm;
  const double rho = d.rho[l];
  const int first = d.lm_vfirst[l], cnt = d.lm_vcnt[l];
  bool ok = rho > 0.0 && isfinite(rho) && cnt > 0;
  int a0 = m.anc0;
  if (cnt > 0) {
    a0 = d.v_anc[first];
    for (int j = 1; j < cnt; ++j) ok = ok && d.v_anc[first + j] == a0;
  }
  const int row_i = cnt > 0 ? d.a_row[a0] : 0;
  const long long ld_ns = (long long)(d.ld[w] * 1e9);
  const long long tau_i = cnt > 0 ? d.a_t[a0] + (long long)row_i * ld_ns : 0;
  const double px = cnt > 0 ? d.a_obs[a0] : 0.0, py = cnt > 0 ? d.a_obs[(size_t)d.Atot + a0] : 0.0;
  const Q4 q_CI = qmk(m.q_CI[0], m.q_CI[1], m.q_CI[2], m.q_CI[3]);
  const V3 p_CI = mk(m.p_CI[0], m.p_CI[1], m.p_CI[2]);
  SensorExt cam;
#pragma unroll
  for (int j = 0; j < 4; ++j) cam.q[j] = m.q_CI[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) cam.p[j] = m.p_CI[j];
  cam.on = 1;
  int s_a, nk_a, s_q, nk_q;
  bool out_a, out_q;
  Q4 q_Ci, q_Cq;
  V3 p_Ci, p_Cq, y;
  rel_side(d, m, tau_i, cam, nullptr, s_a, nk_a, out_a, q_Ci, p_Ci);
  ok = ok && !out_a;
  int row = q.row;
  long long tau_q;
  for (int it = 0;; ++it) {
    tau_q = q.t_rel + (long long)row * ld_ns;
    rel_side(d, m, tau_q, cam, nullptr, s_q, nk_q, out_q, q_Cq, p_Cq);
    y = proj_point(q_Ci, p_Ci, q_Cq, p_Cq, px, py, rho);
    ok = ok && !out_q && y.z > 0.0 && isfinite(y.x) && isfinite(y.y) && isfinite(y.z);
    if (it >= rm.iterations || !ok) break;
    row = (int)fmin(fmax(rint(rm.fy * y.y / y.z + rm.cy), 0.0), (double)(rm.rows - 1));
  }
  const double nan = qnan();
  const double zx = y.x / y.z, zy = y.y / y.z;
  out3[0] = ok ? zx : nan; out3[1] = ok ? zy : nan; out3[2] = ok ? y.z : nan;
  row_o = ok ? row : -1;
  int status = ok ? PRJ_OK : PRJ_NONE;
  if (!excl) return status;
  const int wrow = d.lm_pos[l];
  if (ok) {
    if ((d.dinv[m.lm0 + wrow] == 0.0) | cov_untouched_knots(excl, m, s_a, nk_a) | cov_untouched_knots(excl, m, s_q, nk_q)) status = PRJ_NO_INFO;
  }
  ProjRec &r = *rp;
  r.status = status; r.s_a = s_a; r.nk_a = nk_a; r.s_q = s_q; r.nk_q = nk_q; r.wrow = wrow;
  r.proj[0] = zx; r.proj[1] = zy; r.obs[0] = q.obs[0]; r.obs[1] = q.obs[1];
  if (status != PRJ_OK) return status;
  const double z = 1.0 / rho;
  const V3 x_c = mk(px * z, py * z, z);
  const M3 R_Ci = q2R(q_Ci);
  const ProjLin L = proj_lin(q_Cq, y);
  double jp[144];
  Q4 q_Ii, q_Iq;
  V3 om_i, v_i, om_q, v_q;
  proj_side(d, m, tau_i, q_CI, p_CI, jp, q_Ii, om_i, v_i);
  proj_jac_T(L, false, R_Ci, x_c, y, jp, r.jt_a);
  proj_side(d, m, tau_q, q_CI, p_CI, jp, q_Iq, om_q, v_q);
  proj_jac_T(L, true, R_Ci, x_c, y, jp, r.jt_q);
  proj_cols(L, R_Ci, px, py, rho, y, q_CI, p_CI, (double)row_i, q2R(q_Ii), om_i, v_i, (double)row, q_Iq, om_q, v_q, r.j, r.jld);
  return status;
}
__global__ __launch_bounds__(64) void k_cov_proj_jac(Dev d, int n, const ProjQuery *qs, const uint8_t *excl, ProjRowModel rm, ProjRec *recs, double *proj3,
                                                     int32_t *row_out, int32_t *status_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double o[3];
  int row;
  const int status = proj_query(d, qs[i], excl, rm, excl ? recs + i : nullptr, o, row);
  proj3[3 * (size_t)i] = o[0]; proj3[3 * (size_t)i + 1] = o[1]; proj3[3 * (size_t)i + 2] = o[2];
  row_out[i] = row;
  status_out[i] = status;
}

// One visual block of the window itself (ctvio_visual_gate_batch) and what k_cov_gate_jac makes of it: the projection record of the query
// (landmark, t_j, row_j) with obs = p_j, the whitened residual before the loss r = img_w (proj - p_j), the loss weight rho'(|r|^2) and the
// corrector S (symmetric 2 x 2: entries (0,0), (0,1), (1,1)) as vis_block_eval (factors.hpp) applies it to the block's Jacobian rows:
// S = sqrt(rho') (I - alpha r r^T / s) with Ceres' rule alpha = 0 where s == 0 or rho'' <= 0 -- which the Cauchy loss always meets, so that
// S = sqrt(rho') I here; the general form is kept so that the epilogue does not depend on the loss.
enum { GATE_WEAK = 4, GATE_INACTIVE = 5 };   // ctvio.h: redundancy < min_redundancy; an inactive block that is otherwise ok (the statuses below them are PRJ_*)
struct GateRec : ProjRec {
  double r[2], weight, S[3];
};
// What the gate's kernels write per block slot (absolute slot - slot0; null: not asked for) and the threshold of GATE_WEAK.
struct GateOut {
  double *res2, *weight, *depth, *enorm;   // enorm: |res2| / img_w = |proj - p_j|, the unwhitened reprojection error (for the landmark mean)
  double *red, *cov4, *chi2;
  int32_t *status;
  int32_t slot0, nslot;   // the outputs' first slot; the slots of the slice k_cov_solve runs over (from CovSolveIO::slot_base on)
  double min_red;
};
// |r| / img_w with every operation rounded once.  (The __d*_rn intrinsics are plain operators here and contract into an fma like any
// others: a landmark with a single counted block then missed "re-derivable from res2" by an ulp.  The pragma is what keeps them apart.)
__device__ __forceinline__ double gate_enorm(double r0, double r1, double img_w) {
#pragma clang fp contract(off)
  const double a = r0 * r0, b = r1 * r1, s = a + b;
  return sqrt(s) / img_w;
}
// One lane per block slot e = first + i of the slice (records by i, outputs by e - slot0).  A padding slot (v_win < 0) gets a PRJ_NONE
// record and nothing else.  The value comes from proj_query, so it has the bits of the values-only call (excl null: no records).
__global__ __launch_bounds__(64) void k_cov_gate_jac(Dev d, int first, int n, const uint8_t *excl, GateRec *recs, GateOut o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int e = first + i, w = d.v_win[e];
  if (w < 0) {
    if (excl) { recs[i].status = PRJ_NONE; recs[i].wrow = 0; }
    return;
  }
  const WinMeta &m = d.wins[w];
  const double pjx = d.v_obs[e], pjy = d.v_obs[(size_t)d.Vtot + e], ca = d.v_cauchy[e];
  const ProjQuery q{w, d.v_lm[e], d.v_rowj[e], 0, (long long)d.v_tj[e], {pjx, pjy}};
  const ProjRowModel rm{0.0, 0.0, 1, 0};
  double p3[3];
  int row;
  const int status = proj_query(d, q, excl, rm, excl ? recs + i : nullptr, p3, row);
  // (a status-3 block: p3 is NaN and so is everything below)
  const double ex = p3[0] - pjx, ey = p3[1] - pjy, r0 = m.img_w * ex, r1 = m.img_w * ey;
  const double s = r0 * r0 + r1 * r1;
  double wgt = 1.0, sq = 1.0, asq = 0.0;
  if (ca > 0.0) {
    const double cc = 1.0 / (ca * ca), inv = 1.0 / (1.0 + s * cc), rho2 = -cc * inv * inv;
    wgt = inv;
    sq = sqrt(inv);
    if (!(s == 0.0 || rho2 <= 0.0)) asq = (1.0 - sqrt(fmax(0.0, 1.0 + 2.0 * s * rho2 / inv))) / s;
  }
  if (status == PRJ_NONE) wgt = p3[0];   // (NaN, also without a loss)
  // An inactive block (Dev::v_on) is not in H: nothing is taken out -- weight 0 and S = 0, with which the epilogue's formulas give
  // redundancy 1, C_loo = Cw and chi2 = r^T (Cw + I)^-1 r -- and GATE_INACTIVE stands where PRJ_OK would.
  const bool act = d.v_on[e] != 0;
  if (!act) {
    if (status != PRJ_NONE) wgt = 0.0;
    sq = 0.0;
  }
  const size_t k = (size_t)(e - o.slot0);
  if (o.res2) { o.res2[2 * k] = r0; o.res2[2 * k + 1] = r1; }
  if (o.weight) o.weight[k] = wgt;
  if (o.depth) o.depth[k] = p3[2];
  // (from the residual as returned, every operation rounded once: the landmark mean can be re-derived from res2 to the summation order)
  if (o.enorm) o.enorm[k] = gate_enorm(r0, r1, m.img_w);
  o.status[k] = !act && status == PRJ_OK ? GATE_INACTIVE : status;
  if (!excl) return;
  GateRec &g = recs[i];
  g.r[0] = r0; g.r[1] = r1; g.weight = wgt;
  g.S[0] = sq * (1.0 - asq * r0 * r0); g.S[1] = sq * (-asq * r0 * r1); g.S[2] = sq * (1.0 - asq * r1 * r1);
}

// One lane per landmark of windows wbeg .. (the caller's order; outputs by landmark - lm_base): over its blocks lm_vfirst .. + lm_vcnt in
// slot order -- the upload's packed order, so the bits are the window's -- the count of the blocks whose status is not 3, the mean of their
// |proj - p_j|, the largest chi2 of its status-0 blocks (0: none) and the smallest redundancy of its blocks of status 0 or 4 (+inf: none).
// A window whose factorisation failed (chol_fail; full: the call factored) has neither.  stats3 null: the count alone.
__global__ __launch_bounds__(64) void k_cov_gate_reduce(Dev d, int lm_base, int n, GateOut o, int full, double *stats3, int32_t *count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int l = lm_base + i, first = d.lm_vfirst[l], cnt = d.lm_vcnt[l];
  const bool bad = full && d.lm[d.lm_win[l]].chol_fail != 0;
  int c = 0;
  double sum = 0.0, cmax = 0.0, rmin = __builtin_inf();
  for (int j = 0; j < cnt; ++j) {
    const size_t k = (size_t)(first + j - o.slot0);
    const int st = o.status[k];
    if (st == PRJ_NONE || !d.v_on[first + j]) continue;   // (the landmark's statistics run over its ACTIVE blocks)
    ++c;
    if (!stats3) continue;
    sum = __dadd_rn(sum, o.enorm[k]);
    if (bad) continue;
    if (st == PRJ_OK) cmax = fmax(cmax, o.chi2[k]);
    if (st == PRJ_OK || st == GATE_WEAK) rmin = fmin(rmin, o.red[k]);
  }
  count[i] = c;
  if (stats3) {
    stats3[3 * (size_t)i] = c ? sum / (double)c : qnan();
    stats3[3 * (size_t)i + 1] = cmax;
    stats3[3 * (size_t)i + 2] = rmin;
  }
}

// ctvio_cull_visual_batch: the decision on the gate's device outputs and the flag update.  One lane per landmark (as k_cov_gate_reduce, after
// it and after the last slice's k_cov_solve), over its slots in slot order; no atomics.  A window whose factorisation failed (chol_fail)
// is left alone.  Rules (ctvio.h): an active PRJ_OK block with chi2 > chi2_max goes (worst_only: the landmark's largest such chi2 alone,
// the first in slot order on a tie); every active PRJ_OK block of a landmark with count > 0 and mean error > mean_max goes; an active
// PRJ_NONE block goes with drop_unc.  Singular / no-information / weak blocks and inactive ones are never touched.  Per slot (absolute
// slot - o.slot0): culled = switched off by this launch, flags = Dev::v_on after it.
struct CullRules { double chi2_max, mean_max; int32_t worst_only, drop_unc; };
__global__ __launch_bounds__(64) void k_vis_cull(Dev d, int lm_base, int n, GateOut o, CullRules a, const double *stats3, const int32_t *count, uint8_t *culled,
                                                 uint8_t *flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int l = lm_base + i, first = d.lm_vfirst[l], cnt = d.lm_vcnt[l];
  const bool bad = d.lm[d.lm_win[l]].chol_fail != 0;
  const bool by_chi2 = !bad && a.chi2_max > 0.0, by_mean = !bad && a.mean_max > 0.0 && count[i] > 0 && stats3[3 * (size_t)i] > a.mean_max;
  int worst = -1;
  double cw = 0.0;
  if (by_chi2 && a.worst_only)
    for (int j = 0; j < cnt; ++j) {
      const size_t k = (size_t)(first + j - o.slot0);
      if (!d.v_on[first + j] || o.status[k] != PRJ_OK) continue;
      const double c = o.chi2[k];
      if (c > a.chi2_max && (worst < 0 || c > cw)) { worst = j; cw = c; }
    }
  for (int j = 0; j < cnt; ++j) {
    const int e = first + j;
    const size_t k = (size_t)(e - o.slot0);
    const bool on = d.v_on[e] != 0;
    const int st = o.status[k];
    bool off = false;
    if (on && !bad) {
      if (st == PRJ_OK) off = by_mean || (by_chi2 && o.chi2[k] > a.chi2_max && (!a.worst_only || j == worst));
      else if (st == PRJ_NONE) off = a.drop_unc != 0;
    }
    if (off) d.v_on[e] = 0;
    culled[k] = off ? 1 : 0;
    flags[k] = on && !off ? 1 : 0;
  }
}

// One point of ctvio_predict_landmarks_batch -- a landmark seen from an IMU-predicted pose beyond the spline --, grouped by window on the host,
// and what k_cov_pred_jac makes of it.  The statuses are the projection entry's (PRJ_*).
struct PredPoint {
  int32_t win, pred, lm, row;   // pred: the point's prediction, in the sorted order of the predictions; lm: the caller's landmark index in the window;
                                // row: the image row, or the first guess of the row iteration
  long long last;               // the last sample of the prediction in the concatenated sample arrays (its gyro reading gives w_e)
  double obs[2];                // the candidate point of the gate (zeros without one)
};
constexpr int TRN_OUT = 450;   // doubles k_imu_transition (kernels_prop.hpp) leaves per prediction: Phi (225, row-major) | N (225)
struct PredRec {
  int32_t status, s_a, nk_a, s_q, nk_q, wrow;   // ProjRec's, the "query time" being the prediction's start time imu_t[0]
  int32_t frame, pad;                           // the prediction's bias state
  double proj[2], obs[2];                       // the prediction as returned in proj3, the candidate point
  double j[2], jld[2];                          // d(proj) / drho; d(proj) / d(line delay): the anchor's term + the read-out term (proj_cols)
  double jt_a[48], jt_q[48];                    // Jp^T: the anchor block (proj_jac_T) over knots s_a .. s_a + 3; (A Phi J_nav)^T over knots s_q .. s_q + 3
  double jb[12];                                // (A Phi)[:, 9:15]^T: the rows of the six bias unknowns of state `frame`
  double ana[3];                                // A N A^T: entries (0,0), (0,1), (1,1)
                                                // (j .. ana: written for PRJ_OK only)
};

// One lane per point.  pstat / xe / nrec / trans: per prediction, the status k_cov_nav_jac gave its start time, the end state k_imu_transition
// left (untouched for POSE_OUTSIDE), the start state's record and Phi | N.  The anchor is read as k_cov_proj_jac reads it; the body pose at
// the row time is pred_row_pose(end state, w_e = gyro[last] - bg, delta = (double)(row * ld_ns) * 1e-9), the camera pose that times (q_CI, p_CI),
// y = R_C^T (X - p_C); with a row model the row is iterated first, exactly as there.  PRJ_NONE: the start time is outside the spline, the
// landmark is not computable, or y.z <= 0 or y is not finite at any row visited: proj3 NaN, row_out -1.  The value is formed before excl is
// looked at, by code the Jacobians do not share: the values-only call (excl null; recs, nrec, trans are not touched) gives it the same bits.
// With excl (after k_cov_prepare): PRJ_NO_INFO where 1 / Hll == 0, an anchor knot is one no factor touches (cov_untouched_knots), or the
// start state's record says so (POSE_UNTOUCHED: its knots, knot s + 3 only where u > 0, and the bias state); otherwise the record: the anchor block and the
// columns j, jld as k_cov_proj_jac forms them (the read-out term of jld with omega = w_e, v = the end velocity, R_I(tau)), A (pred_A),
// M = A Phi, the start block M[:, 0:9] J_nav^T from the NavRec (pose rows jt, velocity rows cv), the bias rows M[:, 9:15] and A N A^T.
__global__ __launch_bounds__(64) void k_cov_pred_jac(Dev d, int n, const PredPoint *qs, const uint8_t *excl, ProjRowModel rm, const int32_t *pstat, const double *xe,
                                                     const double *gyro, const NavRec *nrec, const double *trans, PredRec *recs, double *proj3,
                                                     int32_t *row_out, int32_t *status_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PredPoint q = qs[i];
  const int w = q.win;
  const WinMeta &m = d.wins[w];
  const int l = m.lm0 + q.lm;
  const double rho = d.rho[l];
  const int first = d.lm_vfirst[l], cnt = d.lm_vcnt[l];
  bool ok = rho > 0.0 && isfinite(rho) && cnt > 0 && pstat[q.pred] != POSE_OUTSIDE;
  int a0 = m.anc0;
  if (cnt > 0) {
    a0 = d.v_anc[first];
    for (int j = 1; j < cnt; ++j) ok = ok && d.v_anc[first + j] == a0;
  }
  const int row_i = cnt > 0 ? d.a_row[a0] : 0;
  const long long ld_ns = (long long)(d.ld[w] * 1e9);
  const long long tau_i = cnt > 0 ? d.a_t[a0] + (long long)row_i * ld_ns : 0;
  const double px = cnt > 0 ? d.a_obs[a0] : 0.0, py = cnt > 0 ? d.a_obs[(size_t)d.Atot + a0] : 0.0;
  const Q4 q_CI = qmk(m.q_CI[0], m.q_CI[1], m.q_CI[2], m.q_CI[3]);
  const V3 p_CI = mk(m.p_CI[0], m.p_CI[1], m.p_CI[2]);
  SensorExt cam;
#pragma unroll
  for (int j = 0; j < 4; ++j) cam.q[j] = m.q_CI[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) cam.p[j] = m.p_CI[j];
  cam.on = 1;
  int s_a, nk_a;
  bool out_a;
  Q4 q_Ci;
  V3 p_Ci;
  rel_side(d, m, tau_i, cam, nullptr, s_a, nk_a, out_a, q_Ci, p_Ci);
  ok = ok && !out_a;
  // the end state and the last body rate
  const double *x = xe + 16 * (size_t)q.pred, *gl = gyro + 3 * q.last;
  const V3 p_e = mk(x[0], x[1], x[2]), v_e = mk(x[7], x[8], x[9]);
  const Q4 q_e = qmk(x[3], x[4], x[5], x[6]);
  const V3 w_e = mk(gl[0] - x[10], gl[1] - x[11], gl[2] - x[12]);
  int row = q.row;
  double delta;
  Q4 q_I, q_C;
  V3 p_I, p_C, y;
  for (int it = 0;; ++it) {
    delta = (double)((long long)row * ld_ns) * 1e-9;
    pred_row_pose(q_e, p_e, v_e, w_e, delta, q_I, p_I);
    q_C = qmul(q_I, q_CI);
    p_C = p_I + qrot(q_I, p_CI);
    y = proj_point(q_Ci, p_Ci, q_C, p_C, px, py, rho);
    ok = ok && y.z > 0.0 && isfinite(y.x) && isfinite(y.y) && isfinite(y.z);
    if (it >= rm.iterations || !ok) break;
    row = (int)fmin(fmax(rint(rm.fy * y.y / y.z + rm.cy), 0.0), (double)(rm.rows - 1));
  }
  const double nan = qnan();
  const double zx = y.x / y.z, zy = y.y / y.z;
  proj3[3 * (size_t)i] = ok ? zx : nan; proj3[3 * (size_t)i + 1] = ok ? zy : nan; proj3[3 * (size_t)i + 2] = ok ? y.z : nan;
  row_out[i] = ok ? row : -1;
  int status = ok ? PRJ_OK : PRJ_NONE;
  if (!excl) {
    status_out[i] = status;
    return;
  }
  const int wrow = d.lm_pos[l];
  const NavRec &nr = nrec[q.pred];
  if (ok) {
    if ((d.dinv[m.lm0 + wrow] == 0.0) | cov_untouched_knots(excl, m, s_a, nk_a) | (nr.status != POSE_OK)) status = PRJ_NO_INFO;
  }
  PredRec &r = recs[i];
  r.status = status; r.s_a = s_a; r.nk_a = nk_a; r.s_q = ok ? nr.s : 0; r.nk_q = ok ? nr.nk : 3; r.wrow = wrow; r.frame = ok ? nr.frame : 0; r.pad = 0;
  r.proj[0] = zx; r.proj[1] = zy; r.obs[0] = q.obs[0]; r.obs[1] = q.obs[1];
  status_out[i] = status;
  if (status != PRJ_OK) return;
  const double z = 1.0 / rho;
  const V3 x_c = mk(px * z, py * z, z);
  const M3 R_Ci = q2R(q_Ci);
  const ProjLin L = proj_lin(q_C, y);
  {   // the anchor block and the two columns
    double jp[144];
    Q4 q_Ii;
    V3 om_i, v_i;
    proj_side(d, m, tau_i, q_CI, p_CI, jp, q_Ii, om_i, v_i);
    proj_jac_T(L, false, R_Ci, x_c, y, jp, r.jt_a);
    proj_cols(L, R_Ci, px, py, rho, y, q_CI, p_CI, (double)row_i, q2R(q_Ii), om_i, v_i, (double)row, q_I, w_e, v_e, r.j, r.jld);
  }
  double A[30], M[30];
  {
    M3 Et, Bg, Rt, X;
    pred_B(w_e, delta, Et, Bg);
    pred_Cext(q_CI, p_CI, q_I, Rt, X);
    pred_A(L, y, Rt, X, Et, Bg, delta, A);
  }
  const double *Phi = trans + (size_t)TRN_OUT * q.pred, *N = Phi + 225;
  double T[30];   // A N, then A N A^T
#pragma unroll
  for (int c = 0; c < 15; ++c) {
    double m0 = 0.0, m1 = 0.0, t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int k = 0; k < 15; ++k) {
      const double ph = Phi[15 * k + c], nn = N[15 * k + c];
      m0 += A[k] * ph; m1 += A[15 + k] * ph;
      t0 += A[k] * nn; t1 += A[15 + k] * nn;
    }
    M[c] = m0; M[15 + c] = m1; T[c] = t0; T[15 + c] = t1;
  }
  double a00 = 0.0, a01 = 0.0, a11 = 0.0;
#pragma unroll
  for (int c = 0; c < 15; ++c) { a00 += T[c] * A[c]; a01 += T[c] * A[15 + c]; a11 += T[15 + c] * A[15 + c]; }
  r.ana[0] = a00; r.ana[1] = a01; r.ana[2] = a11;
  for (int rr = 0; rr < 24; ++rr) {   // (A Phi J_nav)^T over the knots of the start time: the pose rows, and on position unknowns the velocity rows
    const double *jr = nr.jt + 6 * rr;
    const int b = rr % 6 - 3;
    const double cvk = nr.cv[rr / 6];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      double s = ((M[15 * a] * jr[0] + M[15 * a + 1] * jr[1]) + M[15 * a + 2] * jr[2]) + ((M[15 * a + 3] * jr[3] + M[15 * a + 4] * jr[4]) + M[15 * a + 5] * jr[5]);
      if (b >= 0) s += (b == 0 ? M[15 * a + 6] : b == 1 ? M[15 * a + 7] : M[15 * a + 8]) * cvk;
      r.jt_q[2 * rr + a] = s;
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) { r.jb[2 * c] = M[9 + c]; r.jb[2 * c + 1] = M[24 + c]; }
}

// ---- k_cov_solve<I>: one workgroup per tile fills the tile's 16 right-hand sides in LDS (cov_prologue), substitutes Y = L^-1 B in place
// (cov_forward_subst) and reduces Y to the tile's outputs (cov_epilogue); COV_BASE's two stages stand in the kernel itself.  d is the call's
// copy of Dev (d.active = the per-call mask).  Records whose status is not OK keep zero columns and write nothing.  The substitution: wave
// (h, kp) of four owns the 16-row half h of the current 32-row block and every second 16-column tile of its products; the two partial sums of
// a half are added in a fixed order.  L_bc is read from S inside the envelope only (columns >= 16 env_first of the tile row), L_bb^-1 from
// Dev::chol_inv.  It starts at the first block in which the tile is non-zero (the prologue leaves that row in LDS); the tiles of the products
// go to the two partial sums by their parity, so where the tile starts moves no product from one sum to the other: a column's bits do not
// depend on its tile partners.  Every epilogue sums over the rows from that block on: strided partial sums, added in sequence.
// kind: records | columns, in the order they are written | epilogue -> outputs
// TILE_SEL: io.sel from t.first | one-hot, one per selected unknown (an excluded one: zero) | Y -> io.Y + t.yoff, for k_cov_gram
// TILE_RHO: rows t.first .. of W | its row of W over the planned span, then the line-delay column, times 1 / Hll | 16 partial sums, + 1 / Hll -> io.var_rho
// TILE_POSE: io.rec (PoseRec) from t.first | 6 q + a: J^T over the rows of knots s .. s + nk - 1 | cov_gram6: 3 partial sums -> io.blocks by io.slot
// TILE_POINT: io.lrec by landmark | 3 q + a: TILE_RHO's times -j_rho[a]; barrier; + Jp^T, line-delay row | 3 x 3 Gram, + j_rho j_rho^T / Hll -> io.lm_cov
// TILE_NAV: io.nrec[t.first] | 0..5 pose, 6..8 velocity (c' / dt on positions), 9..14 one-hot bias | cov_gram15 -> io.nav_cov by io.slot
// TILE_REL: io.rec (RelRec) from t.first | 6 q + a: the a-rows; barrier; + the b-rows (overlap: a-term + b-term, elsewhere the one term) | TILE_POSE's
// TILE_PROJ: io.rec (ProjRec) from t.first | 2 q + a: TILE_RHO's column times -j[a]; barrier; + anchor rows; barrier; + query rows and the line-delay
//   row (overlap: anchor term + query term) | cov_gram2: 4 partial sums, + j j^T / Hll, mirrored -> io.blocks by record; cov_gate2(I / img_w^2) on
//   obs - proj from the block just written -> io.chi2 by record
// TILE_RATES: io.rec[t.first] (RatesRec) | 0..8 J^T over the knot rows, 9..14 one-hot bias | cov_gram15 -> io.blocks by io.slot; S = A C A^T +
//   diag(sigma^2), every entry ((C[a][b] + C[a][9 + b]) + C[9 + a][b]) + C[9 + a][9 + b], 6 x 6 Cholesky by one lane -> io.chi2 by io.slot
// TILE_PRED: io.rec (PredRec) from t.first | TILE_PROJ's, the query rows being (A Phi J_nav)^T over the knots of the start time, then the six rows
//   (A Phi)[:, 9:15]^T of the bias state | TILE_PROJ's, + A N A^T (the record's) before mirroring
// TILE_GATE: io.rec (GateRec) by slot of the slice; no tile list: tile b is the slots io.slot_base + 8 b .. + 7 (one window: a window's slots
//   start on a group of 64) | TILE_PROJ's | Cw = img_w^2 (cov_gram2); T = Cw S, A = S T, redundancy = lambda_min(I - A) -> gate.red; below
//   gate.min_red GATE_WEAK, else C_loo = Cw + T (I - A)^-1 T^T -> gate.cov4, cov_gate2(I) on r -> gate.chi2; all by absolute slot - gate.slot0
// TILE_IMUGATE: io.rec (ImuGateRec) by packed sample slot of the slice; no tile list: io.wtile holds the first tile of every window of the
//   slice (one more entry: the tile count), tile b belongs to the last window whose first tile is <= b and is that window's samples
//   2 (b - first tile), + 1 | 6 q + a: imu_w[a] times column a of J^T over the knot rows, imu_w[a] at the bias unknown a of state `frame` |
//   the 21 unique entries of A per sample: four partial sums over the rows k = p mod 4, added in sequence; then lane 0 of wave q runs
//   imugate6 (imugate6.hpp) for sample q in LDS: redundancy -> igate.red; below igate.min_red IMUG_WEAK, else chi2 and M^-1 - I -> igate.chi2,
//   igate.cov36; all by absolute slot - igate.slot0
constexpr int COV_NT = 256;
enum CovInst { COV_BASE, COV_REL, COV_PROJ, COV_RATES, COV_PRED, COV_GATE, COV_IMUGATE };   // COV_BASE: TILE_SEL .. TILE_NAV by t.kind; the others: their one kind
template <CovInst I> struct CovQueryRec { typedef PoseRec type; };
template <> struct CovQueryRec<COV_REL> { typedef RelRec type; };     template <> struct CovQueryRec<COV_PROJ> { typedef ProjRec type; };
template <> struct CovQueryRec<COV_RATES> { typedef RatesRec type; }; template <> struct CovQueryRec<COV_PRED> { typedef PredRec type; };
template <> struct CovQueryRec<COV_GATE> { typedef GateRec type; };   template <> struct CovQueryRec<COV_IMUGATE> { typedef ImuGateRec type; };
// k_cov_solve's arguments; what a call does not use stays null.
template <CovInst I> struct CovSolveIO {
  const CovTile *tiles = nullptr;
  const int32_t *sel = nullptr;                          // TILE_SEL: the concatenated selections
  const int32_t *slot = nullptr;                         // the caller's slot of every query record
  const typename CovQueryRec<I>::type *rec = nullptr;    // the query records
  double *blocks = nullptr;                              // their 6 x 6, 2 x 2 or 15 x 15 covariances
  double *chi2 = nullptr;                                // their gates (null: not asked for)
  double *Y = nullptr, *var_rho = nullptr;               // TILE_SEL, TILE_RHO
  const PointRec *lrec = nullptr;                        // TILE_POINT: the records by landmark through the batch,
  double *lm_cov = nullptr; int lm_base = 0;             // the 3 x 3 blocks from landmark lm_base on
  const NavRec *nrec = nullptr; double *nav_cov = nullptr;   // TILE_NAV
  GateOut gate{}; int slot_base = 0;                     // TILE_GATE: the outputs, and the slice's first slot (TILE_IMUGATE: its first sample slot)
  ImuGateOut igate{};                                    // TILE_IMUGATE: the outputs,
  const int32_t *wtile = nullptr; int wt_n = 0, wt_w0 = 0;   // the first tile of the slice's windows wt_w0 .. wt_w0 + wt_n - 1, then the tile count
};
// TILE_IMUGATE's tile b: the window by bisection over the slice's descriptors (wtile[lo] <= b < wtile[hi] throughout; a window without
// samples shares its first tile with its successor and is never chosen), then the window's samples 2 lt, 2 lt + 1.
template <CovInst I> __device__ __forceinline__ CovTile cov_imugate_tile(const Dev &d, const CovSolveIO<I> &io, int b) {
  int lo = 0, hi = io.wt_n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (io.wtile[mid] <= b) lo = mid; else hi = mid;
  }
  const WinMeta &m = d.wins[io.wt_w0 + lo];
  const int lt = b - io.wtile[lo];
  return CovTile{io.wt_w0 + lo, TILE_IMUGATE, m.imu0 + IMUG_PER_TILE * lt - io.slot_base, min(IMUG_PER_TILE, m.M - IMUG_PER_TILE * lt), 0};
}
// What the stages of one workgroup share.  (The dynamic LDS is named, not carried: a pointer through the struct costs two VGPRs.)
extern __shared__ __attribute__((aligned(16))) double cov_lds[];   // Ys | part (the launch's cov_solve_lds bytes)
struct CovCtx {
  const Dev &d; const CovTile t; const WinMeta &m;   // (t: a copy made field by field; a reference to the kernel's tile costs COV_BASE two VGPRs)
  int P, ldh, cur, tid, wave;   // wave: uniform (read from the first lane)
  int *first;                   // LDS: the first row in which the tile is non-zero (PP: a tile of zero columns)
  __device__ double *Ys() const { return cov_lds; }                                  // [PP][16] the right-hand sides, block by block replaced by Y
  __device__ double *part() const { return cov_lds + 16 * 32 * ((P + 31) / 32); }   // [512] partial sums handed between waves
};

// Columns col0, col0 + 1 of one landmark of a TILE_PROJ / TILE_PRED / TILE_GATE record, sixteen lanes (sub) each: its row wrow of W over the
// planned span, then the line-delay column, times 1 / Hll and -mult[a].  live: the record is OK (mult is read only then).  (COV_BASE's
// ladders keep their own one- and three-column loops.)
__device__ __forceinline__ void cov_wrow_cols(const CovCtx &x, int wrow, int col0, int sub, bool live, const double *mult) {
  const Dev &d = x.d; const WinMeta &m = x.m;
  const int P = x.P, row = m.lm0 + wrow, klo = d.lm_klo[row], khi = d.lm_khi[row];
  const double dv = d.dinv[row];
  const double *Wr = d.WS[x.cur] + m.W0 + (long long)wrow * m.ldw;
  if (!(live && khi >= klo && dv != 0.0)) return;
  const double j0 = -mult[0], j1 = -mult[1];
  const int cend = min(6 * khi + 6, P);
  auto put = [&](int c) {
    if (!d.active[m.u0 + c]) return;
    const double v = Wr[c] * dv;
    x.Ys()[c * 16 + col0] = v * j0; x.Ys()[c * 16 + col0 + 1] = v * j1;
  };
  for (int c = 6 * klo + sub; c < cend; c += 16) put(c);
  if (sub == 0 && cend <= P - 1) put(P - 1);
}
// One lane's scan over the tile's OK records: a record that starts at knot s and whose landmark is row `row` of W.
__device__ __forceinline__ void cov_span_first(const CovCtx &x, int row, int s) {
  *x.first = min(*x.first, 6 * s);
  if (x.d.lm_khi[row] >= x.d.lm_klo[row]) *x.first = min(*x.first, 6 * x.d.lm_klo[row]);
}

// ---- TILE_POSE and TILE_REL (ctvio_pose_covariance_batch, ctvio_relative_pose_batch)
__device__ __forceinline__ void cov_rel_prologue(const CovCtx &x, const RelRec *rec) {
  const CovTile &t = x.t;
  for (int e = x.tid; e < 144 * t.count; e += COV_NT) {
    const int qi = e / 144, r = (e % 144) / 6, a = e % 6;
    const RelRec &rr = rec[t.first + qi];
    if (rr.status == POSE_OK && r < 6 * rr.nk_a && x.d.active[x.m.u0 + 6 * rr.s_a + r]) x.Ys()[(6 * rr.s_a + r) * 16 + 6 * qi + a] = rr.jt_a[6 * r + a];
  }
  __syncthreads();
  for (int e = x.tid; e < 144 * t.count; e += COV_NT) {
    const int qi = e / 144, r = (e % 144) / 6, a = e % 6;
    const RelRec &rr = rec[t.first + qi];
    if (rr.status == POSE_OK && r < 6 * rr.nk_b && x.d.active[x.m.u0 + 6 * rr.s_b + r]) x.Ys()[(6 * rr.s_b + r) * 16 + 6 * qi + a] += rr.jt_b[6 * r + a];
  }
  if (x.tid == 0)
    for (int qi = 0; qi < t.count; ++qi) {
      const RelRec &rr = rec[t.first + qi];
      if (rr.status == POSE_OK) *x.first = min(*x.first, 6 * min(rr.s_a, rr.s_b));
    }
}
// the two 6 x 6 Gram blocks straight from Ys; every entry three partial sums over the rows k = p mod 3, added in sequence
__device__ __forceinline__ void cov_gram6(const CovCtx &x, int b0, const int32_t *slot, double *blocks) {
  const int P = x.P, tid = x.tid, k0 = min(32 * b0, P) / 3 * 3;
  if (tid < 216) {
    const int p = tid / 72, e = tid % 72, ci = 6 * (e / 36) + (e % 36) / 6, cj = 6 * (e / 36) + e % 6;
    double s = 0.0;
    for (int k = k0 + p; k < P; k += 3) s += x.Ys()[k * 16 + ci] * x.Ys()[k * 16 + cj];
    x.part()[p * 72 + e] = s;
  }
  __syncthreads();
  if (tid < 36 * x.t.count) blocks[(long long)36 * slot[x.t.first + tid / 36] + tid % 36] = (x.part()[tid] + x.part()[72 + tid]) + x.part()[144 + tid];
}

// ---- TILE_NAV and TILE_RATES (ctvio_nav_state_batch, ctvio_imu_predict_batch, ctvio_body_rates_batch): one query per tile.  The 120 unique
// entries of the 15 x 15 Gram block of columns 0..14 over the rows k0 .. P - 1: four partial sums over the rows k = p mod 4 each, added in
// sequence, mirrored into cov + 225 slot[0].  keep: lane tid < 120 leaves its entry (i >= j) in part[i (i + 1) / 2 + j] (it alone has read it).
__device__ __forceinline__ void cov_gram15(const double *Ys, double *part, int k0, int P, int tid, double *cov, const int32_t *slot, bool keep) {
  for (int x = tid; x < 480; x += COV_NT) {
    const int p = x / 120;
    int ci, cj;
    tile_decode(x % 120, ci, cj);
    double s = 0.0;
    for (int k = k0 + p; k < P; k += 4) s += Ys[k * 16 + ci] * Ys[k * 16 + cj];
    part[x] = s;
  }
  __syncthreads();
  if (tid < 120) {
    int ci, cj;
    tile_decode(tid, ci, cj);
    const double v = ((part[tid] + part[120 + tid]) + part[240 + tid]) + part[360 + tid];
    double *o = cov + (long long)225 * slot[0];
    o[15 * ci + cj] = v;
    o[15 * cj + ci] = v;
    if (keep) part[tid] = v;
  }
}
__device__ __forceinline__ void cov_rates_prologue(const CovCtx &x, const RatesRec &rr) {
  const Dev &d = x.d; const WinMeta &m = x.m;
  const int tid = x.tid;
  if (rr.status == POSE_OK) {
    if (tid < 216) {
      const int r = tid / 9, a = tid % 9;
      if (r < 6 * rr.nk && d.active[m.u0 + 6 * rr.s + r]) x.Ys()[(6 * rr.s + r) * 16 + a] = rr.jt[tid];
    } else if (tid < 222) {
      const int a = tid - 216, j = 6 * m.K + 6 * rr.frame + a;
      if (d.active[m.u0 + j]) x.Ys()[j * 16 + 9 + a] = 1.0;
    }
    if (tid == 0) *x.first = 6 * rr.s;
  }
}
// TILE_NAV's Gram block, then the gate of the IMU sample: 21 lanes form S from the block just written, one lane factors it in LDS
__device__ __forceinline__ void cov_rates_epilogue(const CovCtx &x, int b0, const RatesRec &rr, const int32_t *slot, double *blocks, double *chi2) {
  const int tid = x.tid;
  double *part = x.part();
  if (rr.status != POSE_OK) return;
  cov_gram15(x.Ys(), part, min(32 * b0, x.P), x.P, tid, blocks, slot, true);
  if (!chi2) return;
  __syncthreads();
  double *Sm = part + 128, *zv = Sm + 36;   // S = A C A^T + diag(sigma^2), A = [[I, 0, 0, I, 0], [0, I, 0, 0, I]]: rows a and 9 + a of C; then
                                            // its Cholesky factor in place (lower triangle); z = L^-1 e
  if (tid < 21) {
    int a, b;
    tile_decode(tid, a, b);
    const double c = ((part[a * (a + 1) / 2 + b] + part[(9 + b) * (10 + b) / 2 + a]) + part[(9 + a) * (10 + a) / 2 + b]) + part[(9 + a) * (10 + a) / 2 + 9 + b];
    Sm[6 * a + b] = a == b ? c + rr.sig[a] * rr.sig[a] : c;
  }
  __syncthreads();
  if (tid == 0) {
    double chi = 0.0;
    for (int j = 0; j < 6; ++j) {   // column j of L, then z_j of L z = e
      double dj = Sm[7 * j], ej = rr.meas[j] - rr.z[j];
      for (int k = 0; k < j; ++k) { dj -= Sm[6 * j + k] * Sm[6 * j + k]; ej -= Sm[6 * j + k] * zv[k]; }
      const double ljj = sqrt(dj);
      for (int i = j + 1; i < 6; ++i) {
        double v = Sm[6 * i + j];
        for (int k = 0; k < j; ++k) v -= Sm[6 * i + k] * Sm[6 * j + k];
        Sm[6 * i + j] = v / ljj;
      }
      const double zj = ej / ljj;
      zv[j] = zj;
      chi += zj * zj;
    }
    chi2[slot[0]] = chi;
  }
}

// ---- TILE_IMUGATE (ctvio_imu_gate_batch): one or two samples per tile, six columns each
__device__ __forceinline__ void cov_imugate_prologue(const CovCtx &x, const ImuGateRec *rec) {
  const Dev &d = x.d; const WinMeta &m = x.m; const CovTile &t = x.t;
  for (int e = x.tid; e < 150 * t.count; e += COV_NT) {   // the knot rows (f < 144), then the six bias rows
    const int qi = e / 150, f = e % 150;
    const ImuGateRec &rr = rec[t.first + qi];
    if (rr.status != IMUG_OK) continue;
    if (f < 144) {
      const int r = f / 6, a = f % 6;
      if (r < 6 * rr.nk && d.active[m.u0 + 6 * rr.s + r]) x.Ys()[(6 * rr.s + r) * 16 + 6 * qi + a] = m.imu_w[a] * rr.jt[f];
    } else {
      const int a = f - 144, j = 6 * m.K + 6 * rr.frame + a;
      if (d.active[m.u0 + j]) x.Ys()[j * 16 + 6 * qi + a] = m.imu_w[a];
    }
  }
  if (x.tid == 0)
    for (int qi = 0; qi < t.count; ++qi)
      if (rec[t.first + qi].status == IMUG_OK) *x.first = min(*x.first, 6 * rec[t.first + qi].s);
}
// part: [4][42] partial sums | [2][21] A | [2][IMUGATE6_WORK] the work areas of the two lanes.  The two samples' 6 x 6 steps run in lane 0
// of waves 0 and 1: two wave instructions never share an LDS cycle, so the layout of the work areas needs no padding against each other,
// and the rest of the part buffer is free by then.
static_assert(168 + 42 + IMUG_PER_TILE * IMUGATE6_WORK <= 512, "cov_imugate_epilogue: the part buffer");
__device__ __forceinline__ void cov_imugate_epilogue(const CovCtx &x, int b0, const ImuGateRec *rec, const ImuGateOut &g, int slot_base) {
  const CovTile &t = x.t;
  const int P = x.P, tid = x.tid, k0 = min(32 * b0, P);
  double *part = x.part();
  if (tid < 168) {
    const int p = tid / 42, e = tid % 42, c0 = 6 * (e / 21);
    int ci, cj;
    tile_decode(e % 21, ci, cj);
    double s = 0.0;
    for (int k = k0 + p; k < P; k += 4) s += x.Ys()[k * 16 + c0 + ci] * x.Ys()[k * 16 + c0 + cj];
    part[p * 42 + e] = s;
  }
  __syncthreads();
  if (tid < 42) part[168 + tid] = ((part[tid] + part[42 + tid]) + part[84 + tid]) + part[126 + tid];
  __syncthreads();
  const int q = x.wave;
  if ((tid & 63) == 0 && q < t.count) {
    const ImuGateRec &rr = rec[t.first + q];
    if (rr.status == IMUG_OK) {
      const size_t k = (size_t)(slot_base + t.first + q - g.slot0);
      double red, chi;
      imugate6(part + 168 + 21 * q, rr.r, g.cov36 != nullptr, part + 210 + IMUGATE6_WORK * q, red, chi, g.cov36 ? g.cov36 + 36 * k : nullptr);
      if (g.red) g.red[k] = red;
      if (!(red >= g.min_red)) g.status[k] = IMUG_WEAK;   // (cov36 and chi2 are the host's fill)
      else if (g.chi2) g.chi2[k] = chi;
    }
  }
}

// ---- TILE_PROJ, TILE_PRED and TILE_GATE (ctvio_project_landmarks_batch, ctvio_predict_landmarks_batch, ctvio_visual_gate_batch)
// + the anchor rows 6 s_a .. 6 (s_a + nk_a) - 1 of every query's two columns
template <class Rec> __device__ __forceinline__ void cov_anchor_rows(const CovCtx &x, const Rec *rec) {
  for (int e = x.tid; e < 48 * x.t.count; e += COV_NT) {
    const int qi = e / 48, r = (e % 48) / 2, a = e % 2;
    const Rec &pr = rec[x.t.first + qi];
    if (pr.status == PRJ_OK && r < 6 * pr.nk_a && x.d.active[x.m.u0 + 6 * pr.s_a + r]) x.Ys()[(6 * pr.s_a + r) * 16 + 2 * qi + a] += pr.jt_a[2 * r + a];
  }
}
template <CovInst I, class Rec> __device__ __forceinline__ void cov_proj_prologue(const CovCtx &x, const Rec *rec) {
  const Dev &d = x.d; const WinMeta &m = x.m; const CovTile &t = x.t;
  const int P = x.P, tid = x.tid, q = tid >> 4, sub = tid & 15;
  if (q < t.count) {
    const Rec &pr = rec[t.first + q];
    cov_wrow_cols(x, pr.wrow, 2 * q, sub, pr.status == PRJ_OK, pr.j);
  }
  __syncthreads();
  cov_anchor_rows(x, rec);
  __syncthreads();
  if constexpr (I == COV_PRED) {
    for (int e = tid; e < 62 * t.count; e += COV_NT) {   // + the rows of the start time 6 s_q .. 6 (s_q + nk_q) - 1 (r < 24), the line-delay row (r = 24),
                                                         // the six rows of bias state `frame` (r = 25 .. 30)
      const int qi = e / 62, r = (e % 62) / 2, a = e % 2;
      const Rec &pr = rec[t.first + qi];
      if (pr.status != PRJ_OK) continue;
      const int c = r < 24 ? 6 * pr.s_q + r : (r == 24 ? P - 1 : 6 * m.K + 6 * pr.frame + (r - 25));
      if ((r < 6 * pr.nk_q || r >= 24) && d.active[m.u0 + c]) x.Ys()[c * 16 + 2 * qi + a] += r < 24 ? pr.jt_q[2 * r + a] : (r == 24 ? pr.jld[a] : pr.jb[2 * (r - 25) + a]);
    }
  } else {
    for (int e = tid; e < 50 * t.count; e += COV_NT) {   // + the query rows 6 s_q .. 6 (s_q + nk_q) - 1 (r < 24), then the line-delay row (r = 24)
      const int qi = e / 50, r = (e % 50) / 2, a = e % 2;
      const Rec &pr = rec[t.first + qi];
      if (pr.status != PRJ_OK) continue;
      const int c = r < 24 ? 6 * pr.s_q + r : P - 1;
      if ((r < 6 * pr.nk_q || r == 24) && d.active[m.u0 + c]) x.Ys()[c * 16 + 2 * qi + a] += r < 24 ? pr.jt_q[2 * r + a] : pr.jld[a];
    }
  }
  if (tid == 0)
    for (int qi = 0; qi < t.count; ++qi) {
      const Rec &pr = rec[t.first + qi];
      if (pr.status == PRJ_OK) cov_span_first(x, m.lm0 + pr.wrow, min(pr.s_a, pr.s_q));
    }
}
// Entries (0,0), (0,1), (1,1) of the eight 2 x 2 Gram blocks into part: four partial sums over the rows k = p mod 4 each (cov_gram2 adds them).
__device__ __forceinline__ void cov_gram2_partials(const CovCtx &x, int b0) {
  const int P = x.P, tid = x.tid, k0 = min(32 * b0, P);
  constexpr int NE = 3 * PRJ_PER_TILE;
  if (tid < 4 * NE) {
    const int p = tid / NE, e = tid % NE, v = e % 3, ci = 2 * (e / 3) + (v == 2), cj = 2 * (e / 3) + (v != 0);
    double s = 0.0;
    for (int k = k0 + p; k < P; k += 4) s += x.Ys()[k * 16 + ci] * x.Ys()[k * 16 + cj];
    x.part()[p * NE + e] = s;
  }
  __syncthreads();
}
// entry v of query q: the partial sums in sequence, + j j^T / Hll
__device__ __forceinline__ double cov_gram2(const double *part, int q, int v, const double *j, double dv) {
  constexpr int NE = 3 * PRJ_PER_TILE;
  return (((part[3 * q + v] + part[NE + 3 * q + v]) + part[2 * NE + 3 * q + v]) + part[3 * NE + 3 * q + v]) + (j[v == 2] * j[v != 0]) * dv;
}
// e^T (C + s I)^-1 e by the 2 x 2 Cholesky factor; c: entries (0,0), (0,1), (1,1)
__device__ __forceinline__ double cov_gate2(double c0, double c1, double c2, double s, double e0, double e1) {
  const double l00 = sqrt(c0 + s), l10 = c1 / l00, l11 = sqrt((c2 + s) - l10 * l10);
  const double z0 = e0 / l00, z1 = (e1 - l10 * z0) / l11;
  return z0 * z0 + z1 * z1;
}
// TILE_PROJ and TILE_PRED: the blocks by record, then the gate from the block just written and the record's prediction
template <CovInst I, class Rec> __device__ __forceinline__ void cov_proj_epilogue(const CovCtx &x, int b0, const Rec *rec, double *blocks, double *chi2) {
  const WinMeta &m = x.m; const CovTile &t = x.t;
  const int tid = x.tid;
  cov_gram2_partials(x, b0);
  if (tid < t.count) {
    const Rec &pr = rec[t.first + tid];
    if (pr.status == PRJ_OK) {
      const double dv = x.d.dinv[m.lm0 + pr.wrow];
      double c[3];
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        c[v] = cov_gram2(x.part(), tid, v, pr.j, dv);
        if constexpr (I == COV_PRED) c[v] = c[v] + pr.ana[v];
      }
      double *o = blocks + (long long)4 * (t.first + tid);
      o[0] = c[0]; o[1] = c[1]; o[2] = c[1]; o[3] = c[2];
      if (chi2) chi2[t.first + tid] = cov_gate2(c[0], c[1], c[2], 1.0 / (m.img_w * m.img_w), pr.obs[0] - pr.proj[0], pr.obs[1] - pr.proj[1]);
    }
  }
}
// TILE_GATE: the leave-one-out epilogue, one lane per block
__device__ __forceinline__ void cov_gate_epilogue(const CovCtx &x, int b0, const GateRec *rec, const GateOut &gate, int slot_base) {
  const WinMeta &m = x.m; const CovTile &t = x.t;
  const int tid = x.tid;
  cov_gram2_partials(x, b0);
  if (tid < t.count) {
    const GateRec &pr = rec[t.first + tid];
    if (pr.status == PRJ_OK) {
      const double dv = x.d.dinv[m.lm0 + pr.wrow], w2 = m.img_w * m.img_w;
      double c[3];   // Cw = img_w^2 C
#pragma unroll
      for (int v = 0; v < 3; ++v) c[v] = w2 * cov_gram2(x.part(), tid, v, pr.j, dv);
      const double s00 = pr.S[0], s01 = pr.S[1], s11 = pr.S[2];
      // T = Cw S, A = S T, M = I - A
      const double t00 = c[0] * s00 + c[1] * s01, t01 = c[0] * s01 + c[1] * s11, t10 = c[1] * s00 + c[2] * s01, t11 = c[1] * s01 + c[2] * s11;
      const double m00 = 1.0 - (s00 * t00 + s01 * t10), m01 = -(s00 * t01 + s01 * t11), m11 = 1.0 - (s01 * t01 + s11 * t11);
      const double hd = 0.5 * (m00 - m11), red = 0.5 * (m00 + m11) - sqrt(hd * hd + m01 * m01);
      const size_t k = (size_t)(slot_base + t.first + tid - gate.slot0);
      if (gate.red) gate.red[k] = red;
      if (!(red >= gate.min_red)) {
        gate.status[k] = GATE_WEAK;   // (cov4 and chi2 are the host's fill)
      } else {
        // C_loo = Cw + T M^-1 T^T: U = T M^-1, the three unique entries of U T^T
        const double idet = 1.0 / (m00 * m11 - m01 * m01);
        const double u00 = (t00 * m11 - t01 * m01) * idet, u01 = (t01 * m00 - t00 * m01) * idet, u10 = (t10 * m11 - t11 * m01) * idet, u11 = (t11 * m00 - t10 * m01) * idet;
        const double l0 = c[0] + (u00 * t00 + u01 * t01), l1 = c[1] + (u00 * t10 + u01 * t11), l2 = c[2] + (u10 * t10 + u11 * t11);
        if (gate.cov4) { double *o = gate.cov4 + 4 * k; o[0] = l0; o[1] = l1; o[2] = l1; o[3] = l2; }
        if (gate.chi2) gate.chi2[k] = cov_gate2(l0, l1, l2, 1.0, pr.r[0], pr.r[1]);   // from the values just written
      }
    }
  }
}

// ---- the three stages
template <CovInst I> __device__ __forceinline__ void cov_prologue(const CovCtx &x, const CovSolveIO<I> &io) {
  if constexpr (I == COV_REL) cov_rel_prologue(x, io.rec);
  else if constexpr (I == COV_RATES) cov_rates_prologue(x, io.rec[x.t.first]);
  else if constexpr (I == COV_IMUGATE) cov_imugate_prologue(x, io.rec);
  else cov_proj_prologue<I>(x, io.rec);   // COV_PROJ, COV_PRED, COV_GATE
}
// Y = L^-1 B in place, from the block of the tile's first non-zero row on; returns that block (nblk for a tile of zero columns).
__device__ __forceinline__ int cov_forward_subst(const CovCtx &x) {
  const Dev &d = x.d; const WinMeta &m = x.m;
  const int w = x.t.win, P = x.P, ldh = x.ldh, nblk = (P + 31) / 32, wave = x.wave, lane = x.tid & 63, q4 = lane >> 4, l15 = lane & 15;
  double *Ys = x.Ys(), *part = x.part();
  __syncthreads();
  const int b0 = *x.first / 32;
  const double *S = d.S + m.H0;
  const int32_t *ef = d.env_first + m.tr0;
  const int h = wave & 1, kp = wave >> 1;
  for (int b = b0; b < nblk; ++b) {
    double li[8];
    if (kp == 0) {   // L_bb^-1, rows of this wave's half (row-major; rows beyond the last unknown are identity rows)
      const double *gi = d.chol_inv + ((size_t)w * d.chol_nblk + b) * 1024 + (16 * h + l15) * 32;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) li[kk] = (kk < 4 * (h + 1)) ? gi[4 * kk + q4] : 0.0;
    }
    // ---- products with the blocks left of the diagonal: rows 16 R .. 16 R + 15, columns [kbeg, 32 b)
    const int R = 2 * b + h, rrow = 16 * R + l15;
    const bool rlive = rrow < P;
    const double *arow = S + (long long)min(rrow, P - 1) * ldh;
    const int kbeg = max(16 * ef[min(R, P / 16)], 32 * b0);
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    if (16 * R < P) {
      for (int kt = kbeg / 16 + ((kbeg / 16 + kp) & 1); 16 * kt < 32 * b; kt += 2) {   // (tiles kt = kp mod 2)
        double av[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) av[kk] = rlive ? arow[16 * kt + 4 * kk + q4] : 0.0;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], Ys[(16 * kt + 4 * kk + q4) * 16 + l15], acc, 0, 0, 0);
      }
    }
    if (kp == 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) part[h * 256 + r * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (kp == 0) {   // T_b = B_b - (sum of the two partial products), in place
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double *y = Ys + (32 * b + 16 * h + q4 + 4 * r) * 16 + l15;
        *y = *y - (acc[r] + part[h * 256 + r * 64 + lane]);
      }
    }
    __syncthreads();
    f64x4 yv = {0.0, 0.0, 0.0, 0.0};
    if (kp == 0) {   // Y_b = L_bb^-1 T_b (lower triangular: the upper half needs k < 16 only)
#pragma unroll
      for (int kk = 0; kk < 8; ++kk)
        if (kk < 4 * (h + 1)) yv = __builtin_amdgcn_mfma_f64_16x16x4f64(li[kk], Ys[(32 * b + 4 * kk + q4) * 16 + l15], yv, 0, 0, 0);
    }
    __syncthreads();
    if (kp == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) Ys[(32 * b + 16 * h + q4 + 4 * r) * 16 + l15] = yv[r];
    }
    __syncthreads();
  }
  return b0;
}
template <CovInst I> __device__ __forceinline__ void cov_epilogue(const CovCtx &x, const CovSolveIO<I> &io, int b0) {
  if constexpr (I == COV_PRED || I == COV_PROJ) cov_proj_epilogue<I>(x, b0, io.rec, io.blocks, io.chi2);
  else if constexpr (I == COV_RATES) cov_rates_epilogue(x, b0, io.rec[x.t.first], io.slot + x.t.first, io.blocks, io.chi2);
  else if constexpr (I == COV_GATE) cov_gate_epilogue(x, b0, io.rec, io.gate, io.slot_base);
  else if constexpr (I == COV_IMUGATE) cov_imugate_epilogue(x, b0, io.rec, io.igate, io.slot_base);
  else cov_gram6(x, b0, io.slot, io.blocks);   // COV_REL
}
// amdgpu_waves_per_eu: with the stages of five kinds in it COV_BASE otherwise settles at 58 VGPRs + 8 AGPRs, one wave per SIMD short of the eight
// that the LDS of a tile allows up to P = 128; held to eight it uses 60 VGPRs, no AGPRs, no spill.
template <CovInst I>
__global__ __launch_bounds__(COV_NT) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_cov_solve(Dev d, CovSolveIO<I> io) {
  const int g0 = PRJ_PER_TILE * (int)blockIdx.x;   // (COV_GATE: the tile's first slot in the slice)
  const CovTile t = I == COV_GATE      ? CovTile{d.vb_win[(io.slot_base + g0) / 64], TILE_GATE, g0, min(PRJ_PER_TILE, io.gate.nslot - g0), 0}
                    : I == COV_IMUGATE ? cov_imugate_tile(d, io, (int)blockIdx.x)
                                       : io.tiles[blockIdx.x];
  const WinMeta &m = d.wins[t.win];
  const int P = m.P, tid = threadIdx.x, PP = 32 * ((P + 31) / 32);
  __shared__ int s_first;
  const CovCtx x{d, CovTile{t.win, t.kind, t.first, t.count, t.yoff}, m, P, m.ldh, d.lm[t.win].cur, tid, __builtin_amdgcn_readfirstlane(tid >> 6), &s_first};
  for (int e = tid; e < 16 * PP; e += COV_NT) cov_lds[e] = 0.0;
  if (tid == 0) s_first = PP;
  __syncthreads();
  const int cur = x.cur;   // (COV_BASE's stages stand here, in the kernel: see DESIGN.md on their register count.  Ys and part are x's: the helpers the
                           // ladders call -- cov_forward_subst, cov_gram6, cov_gram15 -- read the same LDS through x)
  double *Ys = x.Ys(), *part = x.part();
  if constexpr (I == COV_BASE) {   // the five kinds of ctvio_covariance, pose_covariance, nav_state and landmark_points, by t.kind
    if (t.kind == TILE_SEL) {
      if (tid < t.count) {
        const int j = io.sel[t.first + tid];
        if (d.active[m.u0 + j]) { Ys[j * 16 + tid] = 1.0; atomicMin(&s_first, j); }   // (an excluded unknown: a zero column, finished by k_cov_gram)
      }
    } else if (t.kind == TILE_POSE) {   // rows 6 s .. 6 (s + nk) - 1 of every query's six columns, where the unknown is in the system
      for (int e = tid; e < 144 * t.count; e += COV_NT) {
        const int qi = e / 144, r = (e % 144) / 6, a = e % 6;
        const PoseRec &pr = io.rec[t.first + qi];
        if (pr.status == POSE_OK && r < 6 * pr.nk && d.active[m.u0 + 6 * pr.s + r]) Ys[(6 * pr.s + r) * 16 + 6 * qi + a] = pr.jt[6 * r + a];
      }
      if (tid == 0)
        for (int qi = 0; qi < t.count; ++qi)
          if (io.rec[t.first + qi].status == POSE_OK) s_first = min(s_first, 6 * io.rec[t.first + qi].s);
    } else if (t.kind == TILE_NAV) {   // pose columns 0..5 and velocity columns 6..8 over rows 6 s .. 6 (s + nk) - 1, one-hot bias columns 9..14 over the
                                // rows of bias state f, each where the unknown is in the system
      const NavRec &nr = io.nrec[t.first];
      if (nr.status == POSE_OK) {
        if (tid < 144) {
          const int r = tid / 6, a = tid % 6;
          if (r < 6 * nr.nk && d.active[m.u0 + 6 * nr.s + r]) Ys[(6 * nr.s + r) * 16 + a] = nr.jt[tid];
        } else if (tid < 156) {   // d(dv_a) / d(position a of knot s + kk) = c'_kk / dt
          const int kk = (tid - 144) / 3, a = (tid - 144) % 3, j = 6 * (nr.s + kk) + 3 + a;
          if (kk < nr.nk && d.active[m.u0 + j]) Ys[j * 16 + 6 + a] = nr.cv[kk];
        } else if (tid < 162) {
          const int a = tid - 156, j = 6 * m.K + 6 * nr.frame + a;
          if (d.active[m.u0 + j]) Ys[j * 16 + 9 + a] = 1.0;
        }
        if (tid == 0) s_first = 6 * nr.s;
      }
    } else if (t.kind == TILE_POINT) {
      const int q = tid >> 4, sub = tid & 15;
      if (q < t.count) {   // -(w_l / Hll) j_rho^T: the row's planned span, then the line-delay column
        const int row = m.lm0 + t.first + q, klo = d.lm_klo[row], khi = d.lm_khi[row];
        const PointRec &pr = io.lrec[m.lm0 + d.lm_at[row]];
        const double dv = d.dinv[row];
        const double *Wr = d.WS[cur] + m.W0 + (long long)(t.first + q) * m.ldw;
        if (pr.status == LMP_OK && khi >= klo && dv != 0.0) {
          const double j0 = -pr.jrho[0], j1 = -pr.jrho[1], j2 = -pr.jrho[2];
          const int cend = min(6 * khi + 6, P);
          for (int c = 6 * klo + sub; c < cend; c += 16)
            if (d.active[m.u0 + c]) { const double v = Wr[c] * dv; Ys[c * 16 + 3 * q] = v * j0; Ys[c * 16 + 3 * q + 1] = v * j1; Ys[c * 16 + 3 * q + 2] = v * j2; }
          if (sub == 0 && cend <= P - 1 && d.active[m.u0 + P - 1]) {
            const double v = Wr[P - 1] * dv;
            Ys[(P - 1) * 16 + 3 * q] = v * j0; Ys[(P - 1) * 16 + 3 * q + 1] = v * j1; Ys[(P - 1) * 16 + 3 * q + 2] = v * j2;
          }
        }
      }
      __syncthreads();
      for (int e = tid; e < 75 * t.count; e += COV_NT) {   // + Jp^T: rows 6 s .. 6 (s + nk) - 1 (r < 24), then the line-delay row (r = 24)
        const int q = e / 75, r = (e % 75) / 3, a = e % 3;
        const PointRec &pr = io.lrec[m.lm0 + d.lm_at[m.lm0 + t.first + q]];
        if (pr.status != LMP_OK) continue;
        const int c = r < 24 ? 6 * pr.s + r : P - 1;
        if ((r < 6 * pr.nk || r == 24) && d.active[m.u0 + c]) Ys[c * 16 + 3 * q + a] += r < 24 ? pr.jt[3 * r + a] : pr.jld[a];
      }
      if (tid == 0)
        for (int q = 0; q < t.count; ++q) {
          const int row = m.lm0 + t.first + q;
          const PointRec &pr = io.lrec[m.lm0 + d.lm_at[row]];
          if (pr.status != LMP_OK) continue;
          s_first = min(s_first, 6 * pr.s);
          if (d.lm_khi[row] >= d.lm_klo[row]) s_first = min(s_first, 6 * d.lm_klo[row]);
        }
    } else {
      const int col = tid >> 4, sub = tid & 15;
      if (col < t.count) {
        const int row = m.lm0 + t.first + col, klo = d.lm_klo[row], khi = d.lm_khi[row];
        const double dv = d.dinv[row];
        const double *Wr = d.WS[cur] + m.W0 + (long long)(t.first + col) * m.ldw;
        if (khi >= klo && dv != 0.0) {   // the row's planned span, then the line-delay column
          const int cend = min(6 * khi + 6, P);
          for (int c = 6 * klo + sub; c < cend; c += 16)
            if (d.active[m.u0 + c]) Ys[c * 16 + col] = Wr[c] * dv;
          if (sub == 0) {
            if (cend <= P - 1 && d.active[m.u0 + P - 1]) Ys[(P - 1) * 16 + col] = Wr[P - 1] * dv;
            atomicMin(&s_first, 6 * klo);
          }
        }
      }
    }
  } else cov_prologue<I>(x, io);
  const int b0 = cov_forward_subst(x);
  if constexpr (I == COV_BASE) {
    if (t.kind == TILE_SEL) {   // a selection tile: Y to the scratch, for k_cov_gram
      double *yo = io.Y + t.yoff;
      for (int e = tid; e < 16 * P; e += COV_NT) yo[e] = Ys[e];
      return;
    }
    if (t.kind == TILE_POSE) { cov_gram6(x, b0, io.slot, io.blocks); return; }
    if (t.kind == TILE_NAV) {   // state tiles: the 15 x 15 Gram block
      cov_gram15(Ys, part, min(32 * b0, P), P, tid, io.nav_cov, io.slot + t.first, false);
      return;
    }
    if (t.kind == TILE_POINT) {   // point tiles: the five 3 x 3 Gram blocks; every entry four partial sums over the rows k = p mod 4, added in sequence
      const int k0 = min(32 * b0, P);
      constexpr int NE = 9 * LMP_PER_TILE;
      if (tid < 4 * NE) {
        const int p = tid / NE, e = tid % NE, ci = 3 * (e / 9) + (e % 9) / 3, cj = 3 * (e / 9) + e % 3;
        double s = 0.0;
        for (int k = k0 + p; k < P; k += 4) s += Ys[k * 16 + ci] * Ys[k * 16 + cj];
        part[p * NE + e] = s;
      }
      __syncthreads();
      if (tid < 9 * t.count) {
        const int q = tid / 9, a = (tid % 9) / 3, b = tid % 3, row = m.lm0 + t.first + q, l = m.lm0 + d.lm_at[row];
        const PointRec &pr = io.lrec[l];
        if (pr.status == LMP_OK)
          io.lm_cov[(long long)9 * (l - io.lm_base) + 3 * a + b] = (((part[tid] + part[NE + tid]) + part[2 * NE + tid]) + part[3 * NE + tid]) + (pr.jrho[a] * pr.jrho[b]) * d.dinv[row];
      }
      return;
    }
    // ---- a landmark tile: column sums of squares in a fixed order (16 strided partial sums per column, then added in sequence)
    {
      const int col = tid & 15, p = tid >> 4;
      double s = 0.0;
      for (int k = min(32 * b0, P) + p; k < P; k += 16) { const double v = Ys[k * 16 + col]; s += v * v; }
      part[p * 16 + col] = s;
    }
    __syncthreads();
    if (tid < t.count) {
      double tot = 0.0;
      for (int p = 0; p < 16; ++p) tot += part[p * 16 + tid];
      const int row = m.lm0 + t.first + tid, l = d.lm_at[row];
      const double dv = d.dinv[row];
      io.var_rho[m.lm0 + l] = dv == 0.0 ? __builtin_inf() : dv + tot;   // (Hll = 0: no information)
    }
  } else cov_epilogue<I>(x, io, b0);
}

// cov[i][j] = Y_i^T Y_j over the pairs of selection tiles of a window (grid: pair, window with a selection); one entry per thread, summed over
// the rows in sequence.  A constant selected unknown gives a zero row and column, an untouched one +inf on its diagonal and 0 elsewhere.
__global__ __launch_bounds__(256) void k_cov_gram(Dev d, const CovWin *wins, const int32_t *sel, const uint8_t *excl, const double *yscr, double *cov) {
  const CovWin cw = wins[blockIdx.y];
  int ti, tj;
  tile_decode(blockIdx.x, ti, tj);
  if (16 * ti >= cw.nsel) return;
  const WinMeta &m = d.wins[cw.win];
  const int P = m.P, i = threadIdx.x >> 4, j = threadIdx.x & 15, si = 16 * ti + i, sj = 16 * tj + j;
  if (si >= cw.nsel || sj >= cw.nsel) return;
  const int ui = sel[cw.sel0 + si], uj = sel[cw.sel0 + sj];
  const double *yi = yscr + cw.y0 + (long long)16 * P * ti + i, *yj = yscr + cw.y0 + (long long)16 * P * tj + j;
  double s = 0.0;
  for (int k = 0; k < P; ++k) s += yi[16 * k] * yj[16 * k];
  if (excl[m.u0 + ui] != COV_IN || excl[m.u0 + uj] != COV_IN) s = (si == sj && excl[m.u0 + ui] == COV_UNTOUCHED) ? __builtin_inf() : 0.0;
  double *c = cov + cw.cov0;
  c[(long long)si * cw.nsel + sj] = s;
  if (ti != tj) c[(long long)sj * cw.nsel + si] = s;
}

}  // namespace ctv
