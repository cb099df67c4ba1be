// kernels_prop.hpp -- IMU dead reckoning past the end of the solve (ctvio_imu_predict_batch): k_imu_propagate carries the navigation state of
// every query, and with it the 15 x 15 covariance, through the query's IMU samples by the midpoint rule (factors.hpp: imu_step).  It runs
// after k_cov_nav_jac (+ k_cov_solve on TILE_NAV tiles) have left every query's state, status and covariance block on the device.
// Part of kernels.hpp (included from there, in order; not a stand-alone header).
//
//   P_j = F P_{j-1} F^T + G Q G^T,   Q = diag(gyr_n^2, acc_n^2, gyr_n^2, acc_n^2, gyr_w^2, acc_w^2) (x) I_3,
// F (15 x 15) and G (15 x 18) from the blocks of imu_step; neither is formed densely: row r of F has the entries
//   ct (columns theta), cg (columns bg), ca (columns ba), `self` on its own column and `cv` on the velocity column of a position row,
// so that row r of T = F P is ct P[theta rows] + cg P[bg rows] + ca P[ba rows] + self P[r] + cv P[6 + r mod 3], and, P' being symmetric,
// row r of P' = F T^T + N is the same combination of the COLUMNS of T.
//
// Mapping: a workgroup is one wave and takes four queries; the 16-lane group g owns query 4 b + g, lane r of the group row r of its P (lane
// 15 idles).  The recurrence is serial in the samples; a group whose query is shorter leaves the loop earlier, the others do not notice: no
// value crosses from one group to another.  Every lane of a group advances the mean and evaluates imu_step redundantly (the same
// instructions on the same operands, so the same bits in every lane), then keeps its own row of F and of G only.
// LDS per query (PROP_Q doubles): P and T as 15 rows of stride 17 -- odd, so that a row read (lane r: r * 17 + j) and a column read (lane r:
// j * 17 + r) both touch 16 distinct double-wide bank pairs (34 r mod 64 is a permutation of the even banks used) -- and the 15 x 9 rows of
// G (cg | acceleration noise of sample 0 | of sample 1).  PROP_Q = 16 mod 32 doubles, so that the two queries of one 32-lane half, which a
// ds_read_b64 serves in one pass, use the complementary bank pairs.  The lanes of a group meet at lds_wave_sync: one wave, no s_barrier.
// Lane r writes the entries (r, c >= r) of P' and their mirrors; what it computed below the diagonal is dropped: symmetric to the bit.
#pragma once

namespace ctv {

// One query of k_imu_propagate, in the order of the navigation-state queries (sorted by window).
struct PropQuery {
  int32_t win, m;        // samples, >= 1 (sample 0 is the start)
  long long s0, o0;      // first sample in the concatenated sample arrays; first output entry (last_only: the only one)
};
struct ImuNoise { double gyr_n, acc_n, gyr_w, acc_w; };

constexpr int PROP_LD = 17, PROP_T = 256, PROP_G = 512, PROP_Q = 656;   // doubles: row stride; offsets of T and G; per query
static_assert(PROP_Q % 32 == 16 && PROP_G + 15 * 9 <= PROP_Q && 15 * PROP_LD <= PROP_T, "k_imu_propagate: LDS layout");

// Row a of a 3 x 3 block as e^T A with e the one-hot vector of a: exact (products with 1 and 0, sums with 0), and plain arithmetic on
// values -- a select between elements of a block the compiler is free to turn into an indexed load, which would put the block in scratch.
__device__ __forceinline__ V3 m3_row(const M3 &A, V3 e) {
  return mk(e.x * A.m[0] + e.y * A.m[3] + e.z * A.m[6], e.x * A.m[1] + e.y * A.m[4] + e.z * A.m[7], e.x * A.m[2] + e.y * A.m[5] + e.z * A.m[8]);
}
__device__ __forceinline__ V3 ld3(const double *p) { return mk(p[0], p[1], p[2]); }

// status: of every query, as k_cov_nav_jac left it (POSE_OUTSIDE: nothing is propagated or written, the host fills the outputs; any other:
// the means; POSE_OK with cov_out: the covariances too).  state0: the 16 state values per query (k_cov_nav_jac); cov_out: the query's P_0
// stands at entry o0 (k_cov_solve wrote it there).  state_out / cov_out: entry o0 + j for sample j, or, last_only, entry o0 for the last.
__global__ __launch_bounds__(64) void k_imu_propagate(Dev d, int n, const PropQuery *qs, const int32_t *status, const long long *imu_t, const double *gyro,
                                                      const double *acc, ImuNoise nz, int last_only, const double *state0, double *state_out,
                                                      double *cov_out) {
  __shared__ double lds[4 * PROP_Q];
  const int lane = threadIdx.x, grp = lane >> 4, r = lane & 15, rr = min(r, 14), blk = rr / 3, a = rr % 3;
  const int qi = blockIdx.x * 4 + grp;
  if (qi >= n) return;
  const int st = status[qi];
  if (st == POSE_OUTSIDE) return;
  const PropQuery pq = qs[qi];
  const bool cov = cov_out != nullptr && st == POSE_OK, row = r < 15;
  double *P = lds + grp * PROP_Q, *T = P + PROP_T, *G = P + PROP_G;

  const double *x0 = state0 + 16 * (size_t)qi;
  V3 p = ld3(x0), v = ld3(x0 + 7);
  Q4 q = qmk(x0[3], x0[4], x0[5], x0[6]);
  const V3 bg = ld3(x0 + 10), ba = ld3(x0 + 13), grav = ld3(d.wins[pq.win].gravity);
  // lane r stores value r of the state
  auto put_state = [&](long long entry) {
    const double val[16] = {p.x, p.y, p.z, q.x, q.y, q.z, q.w, v.x, v.y, v.z, bg.x, bg.y, bg.z, ba.x, ba.y, ba.z};
    double x = val[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) x = r == j ? val[j] : x;
    state_out[16 * entry + r] = x;
  };
  if (!last_only || pq.m == 1) put_state(pq.o0);

  if (cov) {   // P_0: row rr, from where k_cov_solve left it
    const double *c0 = cov_out + 225 * pq.o0 + 15 * rr;
    if (row)
      for (int c = 0; c < 15; ++c) P[rr * PROP_LD + c] = c0[c];
    lds_wave_sync();
  }
  const V3 ea = mk(a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0);
  // the noise that does not depend on the step
  const double hg = 0.5 * nz.gyr_n * nz.gyr_n, an2 = nz.acc_n * nz.acc_n;
  const double walk = blk == 3 ? nz.gyr_w : blk == 4 ? nz.acc_w : 0.0;

  long long t0 = imu_t[pq.s0];
  V3 w0 = ld3(gyro + 3 * pq.s0), a0 = ld3(acc + 3 * pq.s0);
  for (int j = 1; j < pq.m; ++j) {
    const long long t1 = imu_t[pq.s0 + j];
    const V3 w1 = ld3(gyro + 3 * (pq.s0 + j)), a1 = ld3(acc + 3 * (pq.s0 + j));
    const double dt = (double)(t1 - t0) * 1e-9;
    ImuStepJac J;
    imu_step(q, p, v, bg, ba, grav, w0, a0, w1, a1, dt, cov, J);
    t0 = t1; w0 = w1; a0 = a1;
    const bool out = !last_only || j == pq.m - 1;
    const long long entry = last_only ? pq.o0 : pq.o0 + j;
    if (out) put_state(entry);
    if (!cov) continue;
    // ---- this lane's row of F and of G
    const double h = 0.5 * dt;
    const double sv = blk == 1 ? h : blk == 2 ? 1.0 : 0.0;   // position rows are dt / 2 times the velocity rows
    const V3 vt = m3_row(J.Fvt, ea), vg = m3_row(J.Fvg, ea), va = m3_row(J.Fva, ea), tt = m3_row(J.Ett, ea), tg = m3_row(J.Ftg, ea);
    const V3 ct = blk == 0 ? tt : sv * vt, cg = blk == 0 ? tg : sv * vg, ca = sv * va;
    const double self = blk == 0 ? 0.0 : 1.0, cv = blk == 1 ? dt : 0.0;
    const V3 g0 = (sv * h) * m3_row(J.R0, ea), g1 = (sv * h) * m3_row(J.R1, ea);   // p: dt^2 / 4, v: dt / 2
    const double nb = (walk * dt) * (walk * dt);
    if (row) {
      double *gr = G + rr * 9;
      gr[0] = cg.x; gr[1] = cg.y; gr[2] = cg.z; gr[3] = g0.x; gr[4] = g0.y; gr[5] = g0.z; gr[6] = g1.x; gr[7] = g1.y; gr[8] = g1.z;
    }
    // ---- T = F P: row rr.  (Three columns per trip: some thirty LDS reads in flight, and no more registers than that.)
    const double *Pv = P + (6 + a) * PROP_LD, *Pr = P + rr * PROP_LD;
#pragma unroll 3
    for (int c = 0; c < 15; ++c) {
      double s = ct.x * P[c] + ct.y * P[PROP_LD + c] + ct.z * P[2 * PROP_LD + c];
      s += cg.x * P[9 * PROP_LD + c] + cg.y * P[10 * PROP_LD + c] + cg.z * P[11 * PROP_LD + c];
      s += ca.x * P[12 * PROP_LD + c] + ca.y * P[13 * PROP_LD + c] + ca.z * P[14 * PROP_LD + c];
      s += self * Pr[c] + cv * Pv[c];
      if (row) T[rr * PROP_LD + c] = s;
    }
    lds_wave_sync();
    // ---- P' = F T^T + G Q G^T: row rr, from the columns of T; P is not read any more, so the upper triangle and its mirror go straight in
#pragma unroll 3
    for (int c = 0; c < 15; ++c) {
      const double *Tc = T + c * PROP_LD;
      double s = ct.x * Tc[0] + ct.y * Tc[1] + ct.z * Tc[2];
      s += cg.x * Tc[9] + cg.y * Tc[10] + cg.z * Tc[11];
      s += ca.x * Tc[12] + ca.y * Tc[13] + ca.z * Tc[14];
      s += self * Tc[rr] + cv * Tc[6 + a];
      if (c < 9) {
        const double *gc = G + c * 9;
        s += hg * (cg.x * gc[0] + cg.y * gc[1] + cg.z * gc[2]) +
             an2 * ((g0.x * gc[3] + g0.y * gc[4] + g0.z * gc[5]) + (g1.x * gc[6] + g1.y * gc[7] + g1.z * gc[8]));
      } else {
        s += c == rr ? nb : 0.0;
      }
      if (row && c >= rr) { P[rr * PROP_LD + c] = s; P[c * PROP_LD + rr] = s; }
    }
    lds_wave_sync();
    if (out && row) {   // full rows, mirrored entries included
      double *o = cov_out + 225 * entry + 15 * rr;
      for (int c = 0; c < 15; ++c) o[c] = P[rr * PROP_LD + c];
    }
  }
}

// ---- ctvio_predict_landmarks_batch: the same dead reckoning, kept as a TRANSITION.  k_imu_transition carries, beside the mean, the product
// Phi = F_{m-1} ... F_1 of the step Jacobians (identity for one sample) and the process noise N_j = F N_{j-1} F^T + G Q G^T from N_0 = 0, so
// that the covariance of the end state is Phi P_0 Phi^T + N for ANY P_0: k_cov_pred_jac pulls an image point's row A back through Phi onto
// the unknowns of the window (A Phi J_nav), where the landmark's own terms are added before the substitution, and adds A N A^T at the end.
// Mapping, lane roles and the imu_step call sequence are k_imu_propagate's: the end state has ctvio_imu_predict's bits.  N is the recurrence
// above with P := N (T = F N, then N' = F T^T + noise, upper triangle mirrored).  Phi' = F Phi is the row combination of T = F P applied to a
// block that is not symmetric; it reads rows of Phi only, so it is written into a second block and the two swap roles every step.
// LDS per prediction (TRN_Q doubles): N, T, Phi (two blocks), each 15 rows of stride 17 at a multiple of 32 doubles (one full turn of the 64
// banks), so k_imu_propagate's argument holds block by block: row stride 17 is odd, a row read (lane r: 17 r + j) and a column read (lane
// r: 17 j + r) both touch 16 distinct bank pairs; then the 15 x 9 rows of G at 1024.  TRN_Q = 1168 = 16 mod 32: the two predictions of one
// 32-lane half use complementary bank pairs.  4 x 1168 doubles = 37376 bytes per workgroup.
// out: per prediction TRN_OUT doubles (kernels_cov.hpp): Phi (225, row-major), then N (225, symmetric to the bit); written for POSE_OK with want_cov only.
// state_out: the 16 values of the end state per prediction, for every status but POSE_OUTSIDE.
constexpr int TRN_T = 256, TRN_PHI = 512, TRN_G = 1024, TRN_Q = 1168;
static_assert(TRN_Q % 32 == 16 && TRN_G + 15 * 9 <= TRN_Q && 15 * PROP_LD <= TRN_T && TRN_T % 32 == 0 && TRN_PHI % 32 == 0 && TRN_G % 32 == 0,
              "k_imu_transition: LDS layout");

__global__ __launch_bounds__(64) void k_imu_transition(Dev d, int n, const PropQuery *qs, const int32_t *status, const long long *imu_t, const double *gyro,
                                                       const double *acc, ImuNoise nz, int want_cov, const double *state0, double *state_out, double *out) {
  __shared__ double lds[4 * TRN_Q];
  const int lane = threadIdx.x, grp = lane >> 4, r = lane & 15, rr = min(r, 14), blk = rr / 3, a = rr % 3;
  const int qi = blockIdx.x * 4 + grp;
  if (qi >= n) return;
  const int st = status[qi];
  if (st == POSE_OUTSIDE) return;
  const PropQuery pq = qs[qi];
  const bool cov = want_cov != 0 && st == POSE_OK, row = r < 15;
  double *N = lds + grp * TRN_Q, *T = N + TRN_T, *G = N + TRN_G;
  double *Phi = N + TRN_PHI, *Phn = Phi + 256;

  const double *x0 = state0 + 16 * (size_t)qi;
  V3 p = ld3(x0), v = ld3(x0 + 7);
  Q4 q = qmk(x0[3], x0[4], x0[5], x0[6]);
  const V3 bg = ld3(x0 + 10), ba = ld3(x0 + 13), grav = ld3(d.wins[pq.win].gravity);
  if (cov) {   // N_0 = 0, Phi_0 = I: row rr
    if (row)
      for (int c = 0; c < 15; ++c) { N[rr * PROP_LD + c] = 0.0; Phi[rr * PROP_LD + c] = c == rr ? 1.0 : 0.0; }
    lds_wave_sync();
  }
  const V3 ea = mk(a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0);
  const double hg = 0.5 * nz.gyr_n * nz.gyr_n, an2 = nz.acc_n * nz.acc_n;
  const double walk = blk == 3 ? nz.gyr_w : blk == 4 ? nz.acc_w : 0.0;

  long long t0 = imu_t[pq.s0];
  V3 w0 = ld3(gyro + 3 * pq.s0), a0 = ld3(acc + 3 * pq.s0);
  for (int j = 1; j < pq.m; ++j) {
    const long long t1 = imu_t[pq.s0 + j];
    const V3 w1 = ld3(gyro + 3 * (pq.s0 + j)), a1 = ld3(acc + 3 * (pq.s0 + j));
    const double dt = (double)(t1 - t0) * 1e-9;
    ImuStepJac J;
    imu_step(q, p, v, bg, ba, grav, w0, a0, w1, a1, dt, cov, J);
    t0 = t1; w0 = w1; a0 = a1;
    if (!cov) continue;
    // ---- this lane's row of F and of G (k_imu_propagate's)
    const double h = 0.5 * dt;
    const double sv = blk == 1 ? h : blk == 2 ? 1.0 : 0.0;
    const V3 vt = m3_row(J.Fvt, ea), vg = m3_row(J.Fvg, ea), va = m3_row(J.Fva, ea), tt = m3_row(J.Ett, ea), tg = m3_row(J.Ftg, ea);
    const V3 ct = blk == 0 ? tt : sv * vt, cg = blk == 0 ? tg : sv * vg, ca = sv * va;
    const double self = blk == 0 ? 0.0 : 1.0, cv = blk == 1 ? dt : 0.0;
    const V3 g0 = (sv * h) * m3_row(J.R0, ea), g1 = (sv * h) * m3_row(J.R1, ea);
    const double nb = (walk * dt) * (walk * dt);
    if (row) {
      double *gr = G + rr * 9;
      gr[0] = cg.x; gr[1] = cg.y; gr[2] = cg.z; gr[3] = g0.x; gr[4] = g0.y; gr[5] = g0.z; gr[6] = g1.x; gr[7] = g1.y; gr[8] = g1.z;
    }
    // ---- T = F N and Phi' = F Phi: row rr of each
    const double *Nv = N + (6 + a) * PROP_LD, *Nr = N + rr * PROP_LD, *Fv = Phi + (6 + a) * PROP_LD, *Fr = Phi + rr * PROP_LD;
#pragma unroll 3
    for (int c = 0; c < 15; ++c) {
      double s = ct.x * N[c] + ct.y * N[PROP_LD + c] + ct.z * N[2 * PROP_LD + c];
      s += cg.x * N[9 * PROP_LD + c] + cg.y * N[10 * PROP_LD + c] + cg.z * N[11 * PROP_LD + c];
      s += ca.x * N[12 * PROP_LD + c] + ca.y * N[13 * PROP_LD + c] + ca.z * N[14 * PROP_LD + c];
      s += self * Nr[c] + cv * Nv[c];
      double f = ct.x * Phi[c] + ct.y * Phi[PROP_LD + c] + ct.z * Phi[2 * PROP_LD + c];
      f += cg.x * Phi[9 * PROP_LD + c] + cg.y * Phi[10 * PROP_LD + c] + cg.z * Phi[11 * PROP_LD + c];
      f += ca.x * Phi[12 * PROP_LD + c] + ca.y * Phi[13 * PROP_LD + c] + ca.z * Phi[14 * PROP_LD + c];
      f += self * Fr[c] + cv * Fv[c];
      if (row) { T[rr * PROP_LD + c] = s; Phn[rr * PROP_LD + c] = f; }
    }
    lds_wave_sync();
    // ---- N' = F T^T + G Q G^T: row rr, from the columns of T; the upper triangle and its mirror
#pragma unroll 3
    for (int c = 0; c < 15; ++c) {
      const double *Tc = T + c * PROP_LD;
      double s = ct.x * Tc[0] + ct.y * Tc[1] + ct.z * Tc[2];
      s += cg.x * Tc[9] + cg.y * Tc[10] + cg.z * Tc[11];
      s += ca.x * Tc[12] + ca.y * Tc[13] + ca.z * Tc[14];
      s += self * Tc[rr] + cv * Tc[6 + a];
      if (c < 9) {
        const double *gc = G + c * 9;
        s += hg * (cg.x * gc[0] + cg.y * gc[1] + cg.z * gc[2]) +
             an2 * ((g0.x * gc[3] + g0.y * gc[4] + g0.z * gc[5]) + (g1.x * gc[6] + g1.y * gc[7] + g1.z * gc[8]));
      } else {
        s += c == rr ? nb : 0.0;
      }
      if (row && c >= rr) { N[rr * PROP_LD + c] = s; N[c * PROP_LD + rr] = s; }
    }
    lds_wave_sync();
    double *sw = Phi; Phi = Phn; Phn = sw;
  }
  {   // lane r stores value r of the end state
    const double val[16] = {p.x, p.y, p.z, q.x, q.y, q.z, q.w, v.x, v.y, v.z, bg.x, bg.y, bg.z, ba.x, ba.y, ba.z};
    double x = val[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) x = r == j ? val[j] : x;
    state_out[16 * (size_t)qi + r] = x;
  }
  if (cov && row) {
    double *o = out + (size_t)TRN_OUT * qi;
    for (int c = 0; c < 15; ++c) { o[15 * rr + c] = Phi[rr * PROP_LD + c]; o[225 + 15 * rr + c] = N[rr * PROP_LD + c]; }
  }
}

}  // namespace ctv
