// kernels.hpp -- gfx950 kernels of the sliding-window solve (all fp64).  One launch covers a whole batch of windows.  This header holds
// what the kernels share (linearisation modes, the LDS sync / clock-stamp / opaque-zero idioms, column maps, knot loading) and includes the
// sections in order:
//
//   kernels_control.hpp   k_lm_init, k_initial_cost, k_pass_end (gradient norm, cost, Ceres 1.14 accept / reject / terminate / Armijo, set
//                         swap, next iteration's damping), k_zero_normal (only for batches with an IMU-less window), k_knot_prep (d =
//                         log(R_k^-1 R_k+1) and Jr^-1(d) of every knot pair, shared by all blocks; the candidate's table is made by k_step_finish)
//   kernels_imu.hpp       k_imu_linearize_f64 (waves walking the IMU groups: rows through LDS, per-group A^T A on the fp64 matrix cores; it
//                         also clears the accumulated parts of the normal equations), k_imu_linearize_rest (groups the specialised body
//                         leaves out), assemble_imu_window (run by k_misc)
//   kernels_visual.hpp    k_vis_anchor (one record per anchor end), k_vis_eval (landmark-major: block records via LDS, the rows of W, Hll,
//                         g_rho formed in the same kernel), k_linearize_f64 (IMU + visual in one launch for small batches)
//   kernels_assemble.hpp  k_assemble_vis_mfma (MFMA + fp64 LDS Hessian, or global atomics for K > 25; STORE = the order-fixed tail of the
//                         deterministic mode with k_reduce_finalize / k_bias_rows), k_misc
//                         (IMU tiles' bias rows + bias chain + prior), k_post_linearize (first linearisation only); for the windows whose
//                         packed Hessian is not LDS resident under deterministic = 2: k_vis_expand, k_assemble_wide, k_bias_rows_wide
//   kernels_solve.hpp     k_begin_iter, k_schur_window_f64 (large batches) / k_schur_tile_f64, k_schur_tile2_f64 (small; all also produce the
//                         reduced rhs), k_cholesky_flow (P <= 223: register-resident 16 x 16 tiles as a data-flow of waves; k_cholesky_tiles =
//                         its barrier-per-panel form, kept as the timing-independent twin the tests compare it with: it shares the tile steps
//                         (chol_*) with the flow form and differs only in scheduling; k_cholesky_solve =
//                         panel kernel for P > 223), k_step_finish (back-substitution, candidate x (+) alpha delta, its knot-pair table)
//   kernels_query.hpp     k_gauge_restore (double2vector), k_residual_summary, k_spline_eval (trajectory queries)
//   kernels_cov.hpp       k_cov_prepare, k_cov_solve<CovInst> (cov_prologue, cov_forward_subst, cov_epilogue over CovSolveIO), k_cov_gram (marginal
//                         covariances from the factor of the reduced system); the record kernels that feed k_cov_solve, one record per query:
//                         k_cov_pose_jac, k_cov_point_jac, k_cov_nav_jac, k_cov_rel_jac, k_cov_proj_jac, k_cov_rates_jac, k_cov_pred_jac,
//                         k_cov_gate_jac (+ k_cov_gate_reduce: per-landmark statistics of the visual gate)
//   kernels_prop.hpp      k_imu_propagate (IMU dead reckoning from a navigation state: mean and 15 x 15 covariance, four queries per wave)
//   kernels_tri.hpp       k_triangulate (landmark depths by one-sided Jacobi, one wave per landmark), k_shift_anchor (depths re-anchored)
#pragma once
#include <utility>

#include "device_types.hpp"
#include "factors.hpp"
#include "imugate6.hpp"

namespace ctv {

// SPECULATIVE LINEARISATION.  Every pass evaluates the candidate x (+) alpha delta exactly once -- residuals, Jacobians and the
// normal equations together, into the normal-equation set that is NOT the current one (Lm::cur).  The cost at the candidate is
// a by-product (per-group / per-wave partial sums, added up in a fixed order by k_pass_end); on acceptance the sets swap and the
// next iteration starts from a finished linearisation; on rejection the current set is still intact.  The trial points of
// Ceres' projected line search need value and gradient anyway.  Only the last allowed iteration (nothing can follow it) is
// costed without Jacobians.  Modes of the linearisation kernels:
enum { LIN_AT_X = 0,      // the current state into the current set (the first linearisation of a solve, diagnostics)
       LIN_SPEC = 1,      // the candidate into the other set (every pass)
       COST_AT_X = 2 };   // residuals of the current state only (ctvio_cost)
__device__ __forceinline__ bool lin_run(const Lm &lm, int mode) { return lm.status == 0 && (mode != LIN_SPEC || lm.step_valid != 0); }
__device__ __forceinline__ bool lin_cost_only(const Lm &lm, int mode, const LmParams &p) {
  return mode == COST_AT_X || (mode == LIN_SPEC && lm.iter >= p.max_iters && lm.ls_active == 0);
}
__device__ __forceinline__ int lin_target(const Lm &lm, int mode) { return mode == LIN_SPEC ? 1 - lm.cur : lm.cur; }

// (defined with the Schur / step kernels, used by k_pass_end)
__device__ __forceinline__ double grad_norm_entry(const Dev &d, const WinMeta &m, int w, int j, const double *g, bool at_cand);
__device__ __forceinline__ double grad_norm_rot(const Dev &d, const WinMeta &m, int k, const double *g, bool at_cand);
__device__ __forceinline__ bool grad_norm_is_rot(const WinMeta &m, int j);
__device__ __forceinline__ double grad_norm_other(const Dev &d, const WinMeta &m, int w, int j, const double *g, bool at_cand);
__device__ __forceinline__ void begin_iteration(const Dev &d, int w, int *s_go);

// a lane's double as a wave-uniform value (two v_readlane_b32)
__device__ __forceinline__ double readlane_d(double x, int lane) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// the quiet NaN the kernels report for a value that does not exist
__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the sum of a value over the four 16-lane row groups of the wave, in every lane (the tree of two __shfl_xor steps, without the LDS crossbar)
__device__ __forceinline__ double rowgroup_sum(double p) {
  unsigned lo = (unsigned)__double2loint(p), hi = (unsigned)__double2hiint(p);
  const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);   // [0] = {g0, g0, g2, g2}, [1] = {g1, g1, g3, g3}
  const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const double s = __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
  lo = (unsigned)__double2loint(s); hi = (unsigned)__double2hiint(s);
  const auto c = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);   // [0] = {lower half, lower half}, [1] = {upper, upper}
  const auto e = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double((int)e[0], (int)c[0]) + __hiloint2double((int)e[1], (int)c[1]);
}

// A wave-uniform zero the compiler cannot see through (an SGPR written by an opaque s_mov): added to an index or an address, it makes
// the result depend on this point of the program, so that it is recomputed here instead of being hoisted and kept live -- or spilled --
// across a loop or a phase.  Each use says what it keeps from being hoisted.
__device__ __forceinline__ int opaque_zero() {
  int z;
  asm volatile("s_mov_b32 %0, 0" : "=s"(z));
  return z;
}

// LDS hand-over between lanes: wait for this wave's LDS traffic, then meet the other lanes.  The s_waitcnt immediate used here (and
// by the few waits without a barrier) is the gfx9 encoding of lgkmcnt (bits 11:8) = 0 with vmcnt (15:14, 3:0) and expcnt (6:4) at their
// maxima: "every LDS and scalar-memory operation of this wave has completed; outstanding global loads and stores are not waited for" --
// the wait for those is what __syncthreads() would add.
__device__ __forceinline__ void lds_wave_sync() {    // the lanes of one wave (the barrier only pins the compiler's ordering)
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void lds_block_sync() {   // the waves of one workgroup
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();
}

// CTVIO_DEBUG_STAMPS (Dev::dbg, null otherwise): the lane that satisfies `lane_cond` writes clock64() to stamps[idx++], at most `cap`
// slots per kernel.  An optional fifth argument is a double the stamp is made to depend on (x * 0.0 is not folded without fast-math),
// so that the clock is read after the value is complete and not wherever the scheduler finds room.
#define CTV_STAMP(stamps, idx, cap, lane_cond, ...)                                                        \
  do {                                                                                                     \
    if ((stamps) && (lane_cond) && (idx) < (cap))                                                          \
      (stamps)[(idx)++] = clock64() __VA_OPT__(+ (long long)((__VA_ARGS__) * 0.0));                        \
  } while (0)

// local column -> unknown index maps
__device__ __forceinline__ int imu_col(int c, int s, int K, int bias) {
  if (c < 12) return 6 * (s + c / 3) + c % 3;
  if (c < 24) return 6 * (s + (c - 12) / 3) + 3 + (c - 12) % 3;
  return 6 * K + 6 * bias + (c - 24);
}
constexpr __device__ __forceinline__ int vis_col(int c, int si, int sj, int P) {
  if (c < 12) return 6 * (si + c / 3) + c % 3;
  if (c < 24) return 6 * (si + (c - 12) / 3) + 3 + (c - 12) % 3;
  if (c < 36) return 6 * (sj + (c - 24) / 3) + (c - 24) % 3;
  if (c < 48) return 6 * (sj + (c - 36) / 3) + 3 + (c - 36) % 3;
  if (c == 48) return -1;  // inverse depth: landmark block
  return P - 1;            // line delay
}
// The visual assembly multiplies the 48 pose columns of a run in KNOT-MAJOR order: [i end: knot 0 (dtheta 3, dp 3) .. knot 3][j end: the
// same], so that local column c is unknown 6 si + c (c < 24) or 6 sj + c - 24: contiguous per end, no division in the scatter.  The staged
// rows keep vis_col's order (rotations of the four knots, then positions); vis_knot_major_to_col(c) is the vis_col column behind c.
constexpr __device__ __forceinline__ int vis_knot_major_to_col(int c) {
  const int end = c / 24, r = c % 24, k = r / 6, cc = r % 6;
  return 24 * end + (cc < 3 ? 3 * k + cc : 12 + 3 * k + (cc - 3));
}
constexpr bool vis_knot_major_complete() {   // a bijection of 0 .. 47 that vis_col maps onto the contiguous formula
  bool seen[48] = {};
  for (int c = 0; c < 48; ++c) {
    const int o = vis_knot_major_to_col(c);
    if (o < 0 || o >= 48 || seen[o]) return false;
    seen[o] = true;
    for (int si = 0; si < 3; ++si)
      for (int sj = 0; sj < 9; sj += 4)
        if (vis_col(o, si, sj, 1000) != (c < 24 ? 6 * si + c : 6 * sj + c - 24)) return false;
  }
  return true;
}
static_assert(vis_knot_major_complete(), "vis_knot_major_to_col must permute the 48 pose columns into [end][knot][6]");

__device__ __forceinline__ void load_knots(const double *quat, const double *pos, int k0, const double *origin,
                                                            Knots4 &k) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double *q = quat + 4 * (k0 + i), *p = pos + 3 * (k0 + i);
    k.q[i] = qmk(q[0], q[1], q[2], q[3]);
    k.p[i] = mk(p[0] - origin[0], p[1] - origin[1], p[2] - origin[2]);
  }
}

// Knots k0..k0+3 in the local frame of the reference knot `kref`:
//   q'_k = q_ref^-1 q_k (near identity), p'_k = R_ref^T (p_k - p_ref).
struct LocalFrame {
  Q4 qref_inv;
  M3 RT;      // R_ref^T
  double o[3];
  __device__ __forceinline__ void init(const double *quat, const double *pos, int kref) {
    const double *q = quat + 4 * kref, *p = pos + 3 * kref;
    qref_inv = qmk(-q[0], -q[1], -q[2], q[3]);
    const M3 R = q2R(qmk(q[0], q[1], q[2], q[3]));
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) RT.m[3 * i + j] = R.m[3 * j + i];
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
  }
  __device__ __forceinline__ void load(const double *quat, const double *pos, int k0, Knots4 &k) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double *q = quat + 4 * (k0 + i), *p = pos + 3 * (k0 + i);
      k.q[i] = qmul_raw(qref_inv, qmk(q[0], q[1], q[2], q[3]));   // unit x unit: no renormalisation in fp64
      k.p[i] = mul(RT, mk(p[0] - o[0], p[1] - o[1], p[2] - o[2]));
    }
  }
  __device__ __forceinline__ V3 rotate(const double *v) const { return mul(RT, mk(v[0], v[1], v[2])); }  // R_ref^T v
  __device__ __forceinline__ M3 RrefT() const { return RT; }
};

}  // namespace ctv

#include "kernels_control.hpp"
#include "kernels_imu.hpp"
#include "kernels_visual.hpp"
#include "kernels_assemble.hpp"
#include "kernels_solve.hpp"
#include "kernels_query.hpp"
#include "kernels_cov.hpp"
#include "kernels_prop.hpp"
#include "kernels_tri.hpp"
