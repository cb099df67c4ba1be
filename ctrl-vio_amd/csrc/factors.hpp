// factors.hpp -- per-residual-block device evaluation (residual + analytic Jacobian), fp64.  Knots are addressed by global index:
// the 4 active control points of an evaluation at time t are knots s..s+3 with s = (t - t0)/dt, so the reference's SplineMeta /
// parameter-pointer bookkeeping (src/spline/spline_segment.h:131-191, trajectory_estimator.cpp:114-141) disappears.
//
//   imu_eval*                         SplitSpineView::Evaluate (split_spline_view.h:67-214) fused with IMUFactor::Evaluate
//                                     (trajectory_value_factor.h:141-248): general form and the product kernel's staged form
//   vis_anchor_eval / vis_block_eval  ImageFeatureDelayFactor::Evaluate (image_feature_factor.h:63-269) with So3SplineView::EvaluateRp /
//                                     EvaluateRTp / VelocityBody (so3_spline_view.h:136-276,356-411), RdSplineView::evaluate
//                                     (rd_spline_view.h:63-94) and ceres::CauchyLoss + Corrector (restated in the reference at
//                                     marginalization_factor.cpp:39-67), factored through the anchor end
#pragma once
#include "so3.hpp"

namespace ctv {

struct Knots4 {
  Q4 q[4];
  V3 p[4];  // positions relative to a per-block origin (residuals are translation invariant)
};

// Quantities of a 4-knot group that do not depend on the evaluation time u.
struct SegConst {
  V3 d[3];      // d_i = log(R_i^-1 R_{i+1})
  M3 JrI[3];    // Jr^-1(d_i)
  CTV_DI M3 jri(int i) const { return JrI[i]; }
};
// The same with Jr^-1(d_i) left in the per-window table (k_knot_prep) and fetched where it is used: the 27 values per knot
// group are not held in registers across the whole block evaluation (54 VGPRs per spline end).
struct SegConstLazy {
  V3 d[3];
  const double *tab;   // [3][9]
  CTV_DI M3 jri(int i) const {
    M3 J;
#pragma unroll
    for (int e = 0; e < 9; ++e) J.m[e] = tab[9 * i + e];
    return J;
  }
};
// The same with everything held by value in wave-uniform registers (the caller has made the values scalar): Jr^-1 costs no vector
// registers and no loads inside the evaluation loop.
struct SegConstS {
  V3 d[3];
  M3 JrI[3];
  CTV_DI const M3 &jri(int i) const { return JrI[i]; }
};
CTV_DI void seg_const_lazy(const double *kd, const double *kjri, SegConstLazy &sc) {
#pragma unroll
  for (int i = 0; i < 3; ++i) sc.d[i] = mk(kd[3 * i], kd[3 * i + 1], kd[3 * i + 2]);
  sc.tab = kjri;
}
CTV_DI void seg_const(const Knots4 &k, SegConst &sc, bool want_jac) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    sc.d[i] = so3_log(qmul(qconj(k.q[i]), k.q[i + 1]));
    if (want_jac) sc.JrI[i] = so3_Jr_inv(sc.d[i]);
  }
}

// The same from the per-window tables k_knot_prep fills once per state (d of every consecutive knot pair and Jr^-1(d)): the per-pair
// quantities do not depend on the residual block, so they are hoisted out of the per-block evaluation (the reference recomputes
// them inside every factor, so3_spline_view.h:160-166).  One table entry: d = log(q_a^-1 q_b) and Jr^-1(d).
CTV_DI void knot_pair_const(const double *qa, const double *qb, double *d3, double *jri9) {
  const V3 dd = so3_log(qmul(qconj(qmk(qa[0], qa[1], qa[2], qa[3])), qmk(qb[0], qb[1], qb[2], qb[3])));
  d3[0] = dd.x; d3[1] = dd.y; d3[2] = dd.z;
  if (jri9) {
    const M3 J = so3_Jr_inv(mk(dd.x, dd.y, dd.z));
#pragma unroll
    for (int e = 0; e < 9; ++e) jri9[e] = J.m[e];
  }
}
CTV_DI void seg_const_load(const double *kd, const double *kjri, SegConst &sc, bool want_jac) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    sc.d[i] = mk(kd[3 * i], kd[3 * i + 1], kd[3 * i + 2]);
    if (want_jac) {
#pragma unroll
      for (int e = 0; e < 9; ++e) sc.JrI[i].m[e] = kjri[9 * i + e];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// IMU block.  Local column order of J (6 x 30): rot k0..k3 (12) | pos k0..k3 (12) | bg (3) | ba (3).
// Sink::put_col(col, v[6]) receives every column of J (all 6 rows, structural zeros included);
// r[6] is returned whitened.
//
// Local frame (general form only): the caller passes the knots expressed relative to a reference knot,
// q'_k = q_ref^-1 q_k, p'_k = R_ref^T (p_k - p_ref), and gravity as R_ref^T g.  Residuals are invariant under this
// change of gauge and right-perturbation rotation Jacobians are unchanged; only the position Jacobians need
// J_p = J_p' R_ref^T (RrefT).  (The staged form of the product kernel works in the global frame.)
// Jacobian of one IMU block in factored form: the 6 x 30 matrix is w .* [Jw | 0 | I3 | 0 ; Ja | lamA (x) Rinv_g | 0 | I3]
// (trajectory_value_factor.h:198-245).  Consumers read it column by column (imu_emit_cols) or row by row (imu_row_*).
struct ImuJac {
  M3 Jw[4], Ja[4];   // d(gyro) / d(rot knot k), d(accel) / d(rot knot k)
  M3 Rinv_g;         // R(t)^T in the global frame: d(accel) / d(pos knot k) = lamA[k] * Rinv_g
  double lamA[4];
};

template <class SC> 
CTV_DI void imu_eval_core(const Knots4 &k, const SC &sc, double u, double idt, V3 gravity, const double bias[6],
                          const double gyro[3], const double acc[3], const double w[6], const M3 &RrefT, double r[6], bool want_jac, ImuJac &J) {
  double lamR[4], lamW[4];
  double (&lamA)[4] = J.lamA;
  basis<false, 2>(u, idt * idt, lamA);
  basis<true, 0>(u, 1.0, lamR);
  basis<true, 1>(u, idt, lamW);

  V3 accel = mk(0, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) accel = accel + lamA[i] * k.p[i];

  Q4 Ainv[3], accq = qmk(0, 0, 0, 1);
  M3 Apost[4], JrK[3];
  Apost[3] = m3_id();
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    const V3 nkd = (-lamR[i + 1]) * sc.d[i];
    Ainv[i] = so3_exp(nkd);
    accq = qmul_unit(accq, Ainv[i]);
    if (want_jac) { Apost[i] = q2R(accq); JrK[i] = so3_Jr(nkd); }
  }
  V3 om[4];
  om[0] = mk(0, 0, 0);
#pragma unroll
  for (int i = 0; i < 3; ++i) om[i + 1] = qrot(Ainv[i], om[i]) + lamW[i + 1] * sc.d[i];

  const Q4 Rinv_q = qmul_unit(accq, qconj(k.q[0]));
  const V3 ag = accel + gravity;
  const V3 a_pred = qrot(Rinv_q, ag);
  r[0] = w[0] * (om[3].x - (gyro[0] - bias[0]));
  r[1] = w[1] * (om[3].y - (gyro[1] - bias[1]));
  r[2] = w[2] * (om[3].z - (gyro[2] - bias[2]));
  r[3] = w[3] * (a_pred.x - (acc[0] - bias[3]));
  r[4] = w[4] * (a_pred.y - (acc[1] - bias[4]));
  r[5] = w[5] * (a_pred.z - (acc[2] - bias[5]));
  if (!want_jac) return;

  // gyro rows: d(omega)/d(d_j), split_spline_view.h:157-181
  M3 (&Jw)[4] = J.Jw;
  M3 (&Ja)[4] = J.Ja;
#pragma unroll
  for (int i = 0; i < 4; ++i) { Jw[i] = m3_zero(); Ja[i] = m3_zero(); }
  {
    M3 dod = scale(Apost[1], lamW[1]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i > 0) dod = add(scale(mul(mul_hat(Apost[i], om[i]), JrK[i]), lamR[i + 1]), scale(Apost[i + 1], lamW[i + 1]));
      const M3 JrIi = sc.jri(i);
      Jw[i] = sub(Jw[i], mulT(dod, JrIi));
      Jw[i + 1] = add(Jw[i + 1], mul(dod, JrIi));
    }
  }
  // accel rows, split_spline_view.h:183-211 (three R_accum entries: the reference's 2-entry array is a bug)
  const M3 Rinv = q2R(Rinv_q);
  J.Rinv_g = mul(Rinv, RrefT);  // R(t)^T in the global frame, for the position-knot columns
  {
    const M3 lhs = mul_hat(Rinv, ag);
    M3 Racc = q2R(k.q[0]);
    Ja[0] = add(Ja[0], mul(lhs, Racc));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i > 0) Racc = mulT(Racc, q2R(Ainv[i - 1]));
      const M3 dad = scale(mul(mul(lhs, Racc), JrK[i]), lamR[i + 1]);
      const M3 JrIi = sc.jri(i);
      Ja[i] = sub(Ja[i], mulT(dad, JrIi));
      Ja[i + 1] = add(Ja[i + 1], mul(dad, JrIi));
    }
  }
}

// ---- Staged form (k_imu_linearize_f64's product path: values, then the gyro Jacobians, then the accelerometer Jacobians, each stage's
// rows consumed before the next starts, so the two 36-entry Jacobians are never live together), algebraically the same Jacobian with the rotation chain of the accelerometer
// rows rewritten: with A_i = exp(lamR[i+1] d_i), Apost_i = (A_i .. A_2)^T and R(t)^T = Apost_0 R_0^T,
//   R(t)^T hat(a + g) R_0 A_0 .. A_{i-1} = Apost_i hat(b_i),   b_0 = R_0^T (a + g),  b_{i+1} = A_i^T b_i
// (R hat(v) R^T = hat(R v) applied i + 1 times), so d(accel)/d(d_i) = lamR[i+1] Apost_i hat(b_i) Jr(-lamR[i+1] d_i): the very shape of the
// gyro rows (Apost_i hat(omega_i) Jr) -- no rotation matrices of q_0 / A_0 / A_1, no running product.  Small-angle series only
// (so3_exp_small / so3_Jr_small): the kernel checks |d_i| < 0.5 for the group and takes the general body otherwise.
struct ImuMid3 {
  M3 Apost[3];           // Apost[i] = (A_i .. A_2)^T
  M3 JrK[3];             // Jr(-lamR[i + 1] d_i)
  V3 om1, om2;           // omega recursion
  V3 b[3];               // b_i above
  double lamR[4], lamW[4], lamA[4];
};
// gc: the group's other constants, read where they are used (the kernel keeps them in LDS: one broadcast read each per pass instead of
// a register pair for the whole loop): [0..11] knot positions relative to knot 0, [12..20] R_0^T (row major), [21..23] gravity, [24..29] bias
template <class SC> 
CTV_DI void imu_eval_values3(const double *gc, const SC &sc, double u, double idt, const double gyro[3], const double acc[3], const double w[6], double r[6], ImuMid3 &md) {
  basis<false, 2>(u, idt * idt, md.lamA);
  basis<true, 0>(u, 1.0, md.lamR);
  basis<true, 1>(u, idt, md.lamW);
  V3 ag = mk(gc[21], gc[22], gc[23]);   // spline acceleration + gravity (world)
#pragma unroll
  for (int i = 1; i < 4; ++i) ag = ag + md.lamA[i] * mk(gc[3 * i], gc[3 * i + 1], gc[3 * i + 2]);   // (p_0 - p_0 = 0)
  Q4 Ainv[3], accq;
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    const V3 nkd = (-md.lamR[i + 1]) * sc.d[i];
    Ainv[i] = so3_exp_small(nkd);
    accq = i == 2 ? Ainv[2] : qmul_unit(accq, Ainv[i]);
    md.Apost[i] = q2R(accq);
    md.JrK[i] = so3_Jr_small(nkd);
  }
  V3 om3;
  md.om1 = md.lamW[1] * sc.d[0];
  md.om2 = qrot(Ainv[1], md.om1) + md.lamW[2] * sc.d[1];
  om3 = qrot(Ainv[2], md.om2) + md.lamW[3] * sc.d[2];
  md.b[0] = mk(gc[12] * ag.x + gc[13] * ag.y + gc[14] * ag.z, gc[15] * ag.x + gc[16] * ag.y + gc[17] * ag.z,
                  gc[18] * ag.x + gc[19] * ag.y + gc[20] * ag.z);   // R_0^T (a + g)
  md.b[1] = qrot(Ainv[0], md.b[0]);
  md.b[2] = qrot(Ainv[1], md.b[1]);
  const V3 a_pred = qrot(Ainv[2], md.b[2]);   // = R(t)^T (a + g)
  r[0] = w[0] * (om3.x - (gyro[0] - gc[24]));
  r[1] = w[1] * (om3.y - (gyro[1] - gc[25]));
  r[2] = w[2] * (om3.z - (gyro[2] - gc[26]));
  r[3] = w[3] * (a_pred.x - (acc[0] - gc[27]));
  r[4] = w[4] * (a_pred.y - (acc[1] - gc[28]));
  r[5] = w[5] * (a_pred.z - (acc[2] - gc[29]));
}
// ---- Pair-log coordinates.  Every rotation column of a sample goes through the knot-pair table: with M_i (3 x 3) the derivative of a
// sensor's rows with respect to the pair log d_i, knot i receives -M_i JrI_i^T and knot i + 1 receives +M_i JrI_i, so
//   J_rot (3 x 12) = [D0 | M_0 M_1 M_2] (3 x 12) * T (12 x 12),   T = [I3 at knot 0 ; rows (i, e): -JrI_i^T at knot i, +JrI_i at knot i + 1]
// (D0 = Apost_0 hat(b_0), the accelerometer's direct term on knot 0; zero for the gyro).  T is a constant of the group: the per-sample rows
// are streamed in the COMPACT order [D0 3 | M_0 M_1 M_2 9 | bias 3 | r] (16 columns for either sensor), their Gram matrix G^ is accumulated
// as it is, and the group pays T^T G^ T once (T extended by the identity on bias and residual) instead of six M JrI products per sample.
// Entry JrI_i[a][b] lands on two places of the row-major 16 x 16 T: `plus` with its own sign, `minus` negated.
CTV_DI void imu_pairlog_slots(int i, int a, int b, int &plus, int &minus) {
  plus = (3 + 3 * i + a) * 16 + 3 * (i + 1) + b;
  minus = (3 + 3 * i + b) * 16 + 3 * i + a;
}
template <class SC> CTV_DI void imu_pairlog_T(const SC &sc, double T[256]) {
  for (int e = 0; e < 256; ++e) T[e] = 0.0;
  for (int k = 0; k < 16; ++k)
    if (k < 3 || k >= 12) T[17 * k] = 1.0;
  for (int i = 0; i < 3; ++i) {
    const M3 J = sc.jri(i);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        int plus, minus;
        imu_pairlog_slots(i, a, b, plus, minus);
        T[plus] = J.m[3 * a + b];
        T[minus] = -J.m[3 * a + b];
      }
  }
}
// The gyro rows' M_0, M_1, M_2
CTV_DI void imu_pair_gyro3(const ImuMid3 &md, M3 (&M)[3]) {
  M[0] = scale(md.Apost[1], md.lamW[1]);
  M[1] = add(scale(mul(mul_hat(md.Apost[1], md.om1), md.JrK[1]), md.lamR[2]), scale(md.Apost[2], md.lamW[2]));
  M[2] = scale(mul(mul_hat(md.Apost[2], md.om2), md.JrK[2]), md.lamR[3]);
  M[2].m[0] += md.lamW[3]; M[2].m[4] += md.lamW[3]; M[2].m[8] += md.lamW[3];
}
// Gyro row a in the compact order: w_a [0 3 | M_0 M_1 M_2 | e_a] | r_a
CTV_DI void imu_row_gyro_pl(const M3 (&M)[3], const double w[6], const double r[6], int a, double out[16]) {
  out[0] = out[1] = out[2] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int b = 0; b < 3; ++b) out[3 + 3 * i + b] = w[a] * M[i].m[3 * a + b];
  out[12] = out[13] = out[14] = 0.0;
  out[12 + a] = w[a];
  out[15] = r[a];
}
// The three accelerometer rows of a sample in the compact order, ROTATED INTO THE WORLD FRAME: Y = R(t) w [D0 | M_0 M_1 M_2 | I3 | r / w]
// (3 x 16), R(t) = R_0 Apost_0^T (R_0^T: gc[12..20]).  With one weight w for the three rows (the fast body's groups) Y^T Y is the Gram matrix
// of the unrotated rows, and the position columns w lamA_k R(t)^T of the same rows become w lamA_k I3: their product with the compact rows
// is the lamA-weighted sum of Y over the samples.  R(t) D0 = R_0 hat(b_0) and R(t) M_0 = lamR_1 R_0 hat(b_0) Jr: no Apost_0 in either.
CTV_DI void imu_world_accel3(const ImuMid3 &md, const double *gc, const double w[6], const double r[6], double Y[3][16]) {
  M3 R0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R0.m[3 * i + j] = gc[12 + 3 * j + i];
  const M3 Rs = mulT(R0, md.Apost[0]), wRs = scale(Rs, w[3]);
  M3 blk[4];
  blk[0] = mul_hat(R0, w[3] * md.b[0]);
  blk[1] = mul(scale(blk[0], md.lamR[1]), md.JrK[0]);
#pragma unroll
  for (int i = 1; i < 3; ++i) blk[i + 1] = mul(Rs, scale(mul(mul_hat(md.Apost[i], md.b[i]), md.JrK[i]), w[3] * md.lamR[i + 1]));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int b = 0; b < 3; ++b) Y[a][3 * kk + b] = blk[kk].m[3 * a + b];
#pragma unroll
    for (int b = 0; b < 3; ++b) Y[a][12 + b] = wRs.m[3 * a + b];
  }
  // (the residual is whitened already: zero on a lane whose weights are zero, like every other column)
#pragma unroll
  for (int a = 0; a < 3; ++a) Y[a][15] = Rs.m[3 * a] * r[3] + Rs.m[3 * a + 1] * r[4] + Rs.m[3 * a + 2] * r[5];
}
// trajectory_value_factor.h:198-245, column by column
template <class Sink> CTV_DI void imu_emit_cols(const ImuJac &J, const double w[6], Sink &sink) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      double c6[6], p6[6];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        c6[a] = w[a] * J.Jw[kk].m[3 * a + b];
        c6[3 + a] = w[3 + a] * J.Ja[kk].m[3 * a + b];
        p6[a] = 0.0;
        p6[3 + a] = w[3 + a] * J.lamA[kk] * J.Rinv_g.m[3 * a + b];
      }
      sink.put_col(3 * kk + b, c6);
      sink.put_col(12 + 3 * kk + b, p6);
    }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double g6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, h6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    g6[a] = w[a];
    h6[3 + a] = w[3 + a];
    sink.put_col(24 + a, g6);
    sink.put_col(27 + a, h6);
  }
}
// The same entries row by row (same expressions, hence bit-identical values):
//   accelerometer row a: 32 columns [rot 0..11 | pos 12..23 | bg 24..26 = 0 | ba 27..29 | residual 30 | 0]
//   gyroscope row a    : its 16 non-zero columns [rot 0..11 | bg (columns 24..26) | residual (column 30)]
CTV_DI void imu_row_accel(const ImuJac &J, const double w[6], const double r[6], int a, double out[32]) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      out[3 * kk + b] = w[3 + a] * J.Ja[kk].m[3 * a + b];
      out[12 + 3 * kk + b] = w[3 + a] * J.lamA[kk] * J.Rinv_g.m[3 * a + b];
    }
#pragma unroll
  for (int c = 24; c < 32; ++c) out[c] = 0.0;
  out[27 + a] = w[3 + a];
  out[30] = r[3 + a];
}
CTV_DI void imu_row_gyro(const ImuJac &J, const double w[6], const double r[6], int a, double out[16]) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int b = 0; b < 3; ++b) out[3 * kk + b] = w[a] * J.Jw[kk].m[3 * a + b];
  out[12] = out[13] = out[14] = 0.0;
  out[12 + a] = w[a];
  out[15] = r[a];
}

template <class Sink, class SC> 
CTV_DI void imu_eval(const Knots4 &k, const SC &sc, double u, double idt, V3 gravity, const double bias[6],
                     const double gyro[3], const double acc[3], const double w[6], const M3 &RrefT, double r[6], bool want_jac, Sink &sink) {
  ImuJac J;
  imu_eval_core<SC>(k, sc, u, idt, gravity, bias, gyro, acc, w, RrefT, r, want_jac, J);
  if (want_jac) imu_emit_cols(J, w, sink);
}

// ------------------------------------------------------------------------------------------------
// SO(3) spline views on 4 knots.  (Products of unit quaternions -- normalised knots, exp() -- through qmul_unit: Sophus' renormalising
// product without the division, so3.hpp.)
// EvaluateRp (so3_spline_view.h:136-198): returns R(t); J[k] = per-knot 3x3 "partial" Jacobians.
template <class SC, bool SMALL = false> CTV_DI Q4 eval_Rp(const Q4 q[4], const SC &sc, double u, M3 J[4], bool want_jac) {
  double c[4];
  basis<true, 0>(u, 1.0, c);
  Q4 accq = qmk(0, 0, 0, 1);
  M3 Apost[4], JrK[3];
  Apost[3] = m3_id();
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    const V3 kd = c[i + 1] * sc.d[i];
    accq = qmul_unit(accq, so3_exp_sel<SMALL>(neg(kd)));
    if (want_jac) { JrK[i] = so3_Jr_sel<SMALL>(kd); Apost[i] = q2R(accq); }
  }
  const Q4 res = qmul_unit(q[0], qconj(accq));
  if (want_jac) {
    J[0] = Apost[0];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const M3 Jh = scale(mul(Apost[i + 1], JrK[i]), c[i + 1]);
      J[i] = sub(J[i], mulT(Jh, sc.jri(i)));
      J[i + 1] = mul(Jh, sc.jri(i));
    }
  }
  return res;
}
// EvaluateRTp (so3_spline_view.h:208-276): returns R(t)^T.
template <class SC, bool SMALL = false> CTV_DI Q4 eval_RTp(const Q4 q[4], const SC &sc, double u, M3 J[4], bool want_jac) {
  double c[4];
  basis<true, 0>(u, 1.0, c);
  Q4 S[4];
  M3 JrK[3];
  S[0] = q[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const V3 kd = c[i + 1] * sc.d[i];
    S[i + 1] = qmul_unit(S[i], so3_exp_sel<SMALL>(kd));
    if (want_jac) JrK[i] = so3_Jr_sel<SMALL>(neg(kd));
  }
  if (want_jac) {
    J[0] = q2R(S[0]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const M3 Jh = scale(mul(q2R(S[i]), JrK[i]), c[i + 1]);
      J[i] = sub(J[i], mulT(Jh, sc.jri(i)));
      J[i + 1] = mul(Jh, sc.jri(i));
    }
  }
  return qconj(S[3]);
}
// VelocityBody value (so3_spline_view.h:356-411)
template <class SC, bool SMALL = false> CTV_DI V3 eval_omega(const SC &sc, double u, double idt) {
  double c[4], dc[4];
  basis<true, 0>(u, 1.0, c);
  basis<true, 1>(u, idt, dc);
  V3 rv = dc[1] * sc.d[0];
#pragma unroll
  for (int i = 1; i < 3; ++i) rv = qrot(so3_exp_sel<SMALL>((-c[i + 1]) * sc.d[i]), rv) + dc[i + 1] * sc.d[i];
  return rv;
}
// R(t) only (So3Spline::evaluate, so3_spline.h:240-289)
template <class SC> CTV_DI Q4 eval_R(const Q4 q[4], const SC &sc, double u) {
  double c[4];
  basis<true, 0>(u, 1.0, c);
  Q4 res = q[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) res = qmul_unit(res, so3_exp(c[i + 1] * sc.d[i]));
  return res;
}

// Jacobian of the pose at u against the tangents of its four knots (ctvio_pose_covariance), TRANSPOSED: jt[(6 k + c) * 6 + a] =
// d(output a) / d(unknown c of knot k), unknowns (rot 0..2, pos 3..5) under R_k <- R_k exp(delta_k), p_k <- p_k + dp_k, outputs
// (dtheta 0..2, dp 3..5) under R(t) <- R(t) exp(dtheta), p(t) <- p(t) + dp.  Body pose: d(dtheta) / d(delta_k) = J^Rp_k (eval_Rp),
// d(dp) / d(dp_k) = c_k I with c the blending coefficients of the position spline, cross blocks zero.  With a sensor extrinsic (q_SI, p_SI) the
// pose is T_I(t) T_SI: dtheta_S = R_SI^T dtheta_I, dp_S = dp_I - R_I(t) hat(p_SI) dtheta_I.  All 144 entries are written, each once.
// At u = 0 the last knot's blocks are exact zeros (c_3 = u^3 / 6 in both bases).
template <class SC> CTV_DI void pose_jac_T(const Q4 q[4], const SC &sc, double u, bool ext_on, Q4 q_SI, V3 p_SI, double *jt) {
  M3 J[4];
  const Q4 R = eval_Rp<SC>(q, sc, u, J, true);
  double c[4];
  basis<false, 0>(u, 1.0, c);
  M3 RSI = m3_id(), X = m3_zero();   // X = -R_I(t) hat(p_SI)
  if (ext_on) { RSI = q2R(q_SI); X = scale(mul_hat(q2R(R), p_SI), -1.0); }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const M3 B = mul(X, J[k]);
#pragma unroll
    for (int cc = 0; cc < 3; ++cc)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        // rotation unknown cc of knot k: (R_SI^T J_k)[a][cc], then the lever arm
        jt[(6 * k + cc) * 6 + a] = ext_on ? RSI.m[a] * J[k].m[cc] + RSI.m[3 + a] * J[k].m[3 + cc] + RSI.m[6 + a] * J[k].m[6 + cc] : J[k].m[3 * a + cc];
        jt[(6 * k + cc) * 6 + 3 + a] = ext_on ? B.m[3 * a + cc] : 0.0;
        jt[(6 * k + 3 + cc) * 6 + a] = 0.0;
        jt[(6 * k + 3 + cc) * 6 + 3 + a] = a == cc ? c[k] : 0.0;
      }
  }
}

// Jacobian of the navigation state at u (ctvio_nav_state) against the tangents of its four knots: the 24 x 6 block jt of the BODY pose as
// pose_jac_T writes it, and cv[k] = c'_k(u) / dt, the derivative of the blending coefficients of the position spline: the world velocity is
// v(t) = sum_k cv[k] p_k, so d(dv) / d(dp_k) = cv[k] I and the velocity does not depend on the rotations.  At u = 0 the last knot's blocks
// and cv[3] are exact zeros (c'_3 = u^2 / 2).  The bias rows of the state's Jacobian are one-hot and need no evaluation.
template <class SC> CTV_DI void nav_jac_T(const Q4 q[4], const SC &sc, double u, double idt, double *jt, double cv[4]) {
  pose_jac_T(q, sc, u, false, qmk(0.0, 0.0, 0.0, 1.0), mk(0.0, 0.0, 0.0), jt);
  basis<false, 1>(u, idt, cv);
}

// Jacobian of the body rates at u (ctvio_body_rates) -- body angular velocity omega, specific force f = R(t)^T (p''(t) + g), body-frame
// velocity v_B = R(t)^T v_W(t) -- against the tangents of its four knots, TRANSPOSED: jt[(6 k + c) * 9 + a] = d(output a) / d(unknown c of
// knot k), unknowns (rot 0..2, pos 3..5) under R_k <- R_k exp(delta_k), p_k <- p_k + dp_k, outputs (domega 0..2, df 3..5, dv_B 6..8),
// all additive.  The omega and f rows are the IMU factor's (imu_eval_core, the general body, unit weights, zero measurement and bias,
// global frame: Jw, Ja, lamA (x) Rinv_g); under R(t) <- R(t) exp(dtheta), v_B <- v_B + [v_B]x dtheta, so the v_B rows are [v_B]x J^Rp_k
// (eval_Rp: the rotation rows of pose_jac_T) on the rotations and c'_k(u) / dt R(t)^T on the positions.  All 216 entries are written, each
// once.  At u = 0 the last knot's blocks are exact zeros (up to the sign of a zero): lamR_3 = u^3 / 6, lamW_3 and c'_3 = u^2 / 2, lamA_3 = u.
// NC = 6 (ctvio_imu_gate): the omega and f columns alone, jt[(6 k + c) * 6 + a], the same entries with the same bits.
template <class SC, int NC = 9> CTV_DI void rates_jac_T(const Knots4 &k, const SC &sc, double u, double idt, V3 gravity, double *jt) {
  static_assert(NC == 9 || NC == 6, "rates_jac_T: 9 columns, or 6 without v_B");
  const double zero6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, one6[6] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
  double r[6], cv[4];
  ImuJac J;
  imu_eval_core<SC>(k, sc, u, idt, gravity, zero6, zero6, zero6 + 3, one6, m3_id(), r, true, J);
  M3 Jth[4];
  eval_Rp<SC>(k.q, sc, u, Jth, true);
  basis<false, 1>(u, idt, cv);
  V3 v = mk(0, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) v = v + cv[i] * k.p[i];
  const M3 VBx = hat(mul(J.Rinv_g, v));
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const M3 B = mul(VBx, Jth[kk]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        double *rot = jt + (6 * kk + c) * NC, *pos = jt + (6 * kk + 3 + c) * NC;
        rot[a] = J.Jw[kk].m[3 * a + c];
        rot[3 + a] = J.Ja[kk].m[3 * a + c];
        pos[a] = 0.0;
        pos[3 + a] = J.lamA[kk] * J.Rinv_g.m[3 * a + c];
        if (NC == 9) {
          rot[6 + a] = B.m[3 * a + c];
          pos[6 + a] = cv[kk] * J.Rinv_g.m[3 * a + c];
        }
      }
  }
}

// The pose increment T_ab = T_a^-1 T_b of two poses (q_a, p_a), (q_b, p_b) (ctvio_relative_pose): R_ab = R_a^T R_b, p_ab = R_a^T (p_b - p_a),
// and its Jacobian against the knots of both poses.  jt_a, jt_b: the 24 x 6 blocks pose_jac_T wrote for the two poses; they are mapped IN
// PLACE into the two blocks of J_rel^T, J_rel = A_a J_a + A_b J_b.  Tangent of the result (dtheta 0..2, dp 3..5): R_ab <- R_ab exp(dtheta),
// p_ab <- p_ab + dp (dp in frame a):
//   dtheta_ab = dtheta_b - R_ab^T dtheta_a,   dp_ab = [p_ab]x dtheta_a + R_a^T (dp_b - dp_a)
//   A_a = [[-R_ab^T, 0], [[p_ab]x, -R_a^T]],  A_b = [[I, 0], [0, R_a^T]].
// Rows that are exact zeros in jt_a / jt_b (the last knot at u = 0) stay exact zeros (up to the sign of a zero).  jt_a == nullptr: the value alone.
CTV_DI void rel_pose_jac_T(Q4 q_a, V3 p_a, Q4 q_b, V3 p_b, double *jt_a, double *jt_b, Q4 &q_ab, V3 &p_ab) {
  q_ab = qmul(qconj(q_a), q_b);
  const M3 Ra = q2R(q_a), Rab = q2R(q_ab);
  const V3 d = p_b - p_a;
  p_ab = mk(Ra.m[0] * d.x + Ra.m[3] * d.y + Ra.m[6] * d.z, Ra.m[1] * d.x + Ra.m[4] * d.y + Ra.m[7] * d.z, Ra.m[2] * d.x + Ra.m[5] * d.y + Ra.m[8] * d.z);
  if (!jt_a) return;
  for (int r = 0; r < 24; ++r) {
    double *ja = jt_a + 6 * r, *jb = jt_b + 6 * r;
    const V3 th = mk(ja[0], ja[1], ja[2]), dp = mk(ja[3], ja[4], ja[5]), db = mk(jb[3], jb[4], jb[5]);
    const V3 x = cross(p_ab, th);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      ja[a] = -(Rab.m[a] * th.x + Rab.m[3 + a] * th.y + Rab.m[6 + a] * th.z);
      ja[3 + a] = (a == 0 ? x.x : a == 1 ? x.y : x.z) - (Ra.m[a] * dp.x + Ra.m[3 + a] * dp.y + Ra.m[6 + a] * dp.z);
      jb[3 + a] = Ra.m[a] * db.x + Ra.m[3 + a] * db.y + Ra.m[6 + a] * db.z;
    }
  }
}

// The visual factor's prediction of a landmark in the camera at a query time (ctvio_project_landmarks; ImageFeatureDelayFactor::Evaluate,
// image_feature_factor.h:63-269, x_j): anchor camera pose (q_Ci, p_Ci), query camera pose (q_Cq, p_Cq), anchor observation (px, py, 1) and
// inverse depth rho: X = R_Ci (p_i / rho) + p_Ci, y = R_Cq^T (X - p_Cq).  The prediction is (y.x / y.z, y.y / y.z) at depth y.z.
CTV_DI V3 proj_point(Q4 q_Ci, V3 p_Ci, Q4 q_Cq, V3 p_Cq, double px, double py, double rho) {
  const double z = 1.0 / rho;
  const V3 dX = (mul(q2R(q_Ci), mk(px * z, py * z, z)) + p_Ci) - p_Cq;
  const M3 R = q2R(q_Cq);
  return mk(R.m[0] * dX.x + R.m[3] * dX.y + R.m[6] * dX.z, R.m[1] * dX.x + R.m[4] * dX.y + R.m[7] * dX.z, R.m[2] * dX.x + R.m[5] * dX.y + R.m[8] * dX.z);
}
// Its linear maps at y: Pi = (1 / y.z) [[1, 0, -y.x / y.z], [0, 1, -y.y / y.z]] (2 x 3, row-major) and M = Pi R_Cq^T, the map of a world
// displacement of X.
struct ProjLin { double Pi[6], M[6]; };
CTV_DI ProjLin proj_lin(Q4 q_Cq, V3 y) {
  ProjLin L;
  const double iz = 1.0 / y.z;
  L.Pi[0] = iz; L.Pi[1] = 0.0; L.Pi[2] = -(y.x * iz) * iz;
  L.Pi[3] = 0.0; L.Pi[4] = iz; L.Pi[5] = -(y.y * iz) * iz;
  const M3 R = q2R(q_Cq);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) L.M[3 * a + b] = L.Pi[3 * a] * R.m[3 * b] + L.Pi[3 * a + 1] * R.m[3 * b + 1] + L.Pi[3 * a + 2] * R.m[3 * b + 2];
  return L;
}
// One time's 24 x 2 block of the prediction's Jacobian, TRANSPOSED, from the 24 x 6 block jp that pose_jac_T wrote for the CAMERA pose at that
// time (extrinsic on): jt[2 r + a] = d(proj_a) / d(unknown r of knots s .. s + 3).  Anchor time: M [-R_Ci [x_c]x, I] jp^T, x_c = p_i / rho (the
// point Jacobian of ctvio_landmark_points, mapped by M); query time: [Pi [y]x, -M] jp^T (dy = [y]x dtheta_C - R_Cq^T dp_C).  Rows that are
// exact zeros in jp (the last knot at u = 0) stay exact zeros (up to the sign of a zero).  jp and jt may not overlap.
CTV_DI void proj_jac_T(const ProjLin &L, bool query, const M3 &R_Ci, V3 x_c, V3 y, const double *jp, double *jt) {
  double B[12];
  const M3 Hx = query ? hat(y) : scale(mul_hat(R_Ci, x_c), -1.0);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double *T = query ? L.Pi : L.M;
      B[6 * a + c] = T[3 * a] * Hx.m[c] + T[3 * a + 1] * Hx.m[3 + c] + T[3 * a + 2] * Hx.m[6 + c];
      B[6 * a + 3 + c] = query ? -L.M[3 * a + c] : L.M[3 * a + c];
    }
  for (int r = 0; r < 24; ++r)
#pragma unroll
    for (int a = 0; a < 2; ++a)
      jt[2 * r + a] = ((B[6 * a] * jp[6 * r] + B[6 * a + 1] * jp[6 * r + 1]) + B[6 * a + 2] * jp[6 * r + 2]) +
                      ((B[6 * a + 3] * jp[6 * r + 3] + B[6 * a + 4] * jp[6 * r + 4]) + B[6 * a + 5] * jp[6 * r + 5]);
}
// Its two remaining columns.  j = M (-R_Ci p_i / rho^2), the inverse depth; jld = the line delay, the formal derivative the factor uses, both
// times summed: row_i M (R_Ii [omega_Ii]x (R_CI x_c + p_CI) + v_Ii) + row_q Pi ([y]x omega_C - R_Cq^T v_C) with omega_C = R_CI^T omega_Iq,
// v_C = v_Iq + R_Iq [omega_Iq]x p_CI (omega: body rates of eval_omega, v: world velocities of the position spline).
CTV_DI void proj_cols(const ProjLin &L, const M3 &R_Ci, double px, double py, double rho, V3 y, Q4 q_CI, V3 p_CI, double row_i, const M3 &R_Ii, V3 om_i,
                      V3 v_i, double row_q, Q4 q_Iq, V3 om_q, V3 v_q, double j[2], double jld[2]) {
  const double z = 1.0 / rho;
  const V3 jr = (-z * z) * mul(R_Ci, mk(px, py, 1.0));
  const V3 p_I = qrot(q_CI, mk(px * z, py * z, z)) + p_CI;
  const V3 da = row_i * (mul(R_Ii, cross(om_i, p_I)) + v_i);
  const V3 om_C = qrot(qconj(q_CI), om_q);
  const V3 v_C = v_q + qrot(q_Iq, cross(om_q, p_CI));
  const V3 rv = qrot(qconj(qmul(q_Iq, q_CI)), v_C);
  const V3 dq = row_q * (cross(y, om_C) - rv);
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    j[a] = L.M[3 * a] * jr.x + L.M[3 * a + 1] * jr.y + L.M[3 * a + 2] * jr.z;
    jld[a] = (L.M[3 * a] * da.x + L.M[3 * a + 1] * da.y + L.M[3 * a + 2] * da.z) + (L.Pi[3 * a] * dq.x + L.Pi[3 * a + 1] * dq.y + L.Pi[3 * a + 2] * dq.z);
  }
}

// One midpoint step of the IMU dead reckoning (ctvio_imu_predict; the mean of VisualOdometry::ProcessIMU, visual_odometry.cpp:137-172) from
// sample (w0, a0) to sample (w1, a1), dt apart, with the biases (bg, ba) held and g the window's gravity (sign as in the IMU factor):
//   w = (w0 + w1) / 2 - bg,  R' = R Exp(w dt),  A = ((R (a0 - ba) - g) + (R' (a1 - ba) - g)) / 2,  p' = p + dt v + dt^2 A / 2,  v' = v + dt A.
// (q, p, v) are advanced in place.  With want_jac the 3 x 3 blocks of F = d(state') / d(state) and G = d(state') / d(noise) that are not 0, I
// or dt I, in the tangent (dtheta, dp, dv, dbg, dba) of R <- R Exp(dtheta), the rest additive, with E = Exp(w dt), J = Jr(w dt), u0 = a0 - ba,
// u1 = a1 - ba:
//   F[theta, theta] = E^T            F[theta, bg] = -J dt
//   F[v, theta] = -dt (R [u0] + R' [u1] E^T) / 2     F[v, bg] = dt^2 R' [u1] J / 2     F[v, ba] = -dt (R + R') / 2
//   F[p, .] = (dt / 2) F[v, .] in the same three columns (beside F[p, p] = I, F[p, v] = dt I: formed by the caller, not stored)
//   G: gyro noise of either sample -F[., bg] / 2 on the rows theta, p, v; accelerometer noise of sample 0 / 1: dt R0 / 2, dt R1 / 2 on the v
//   rows and dt / 2 times that on the p rows (R0 = R, R1 = R'); the bias walks dt I on their own rows.
// The mean does not depend on want_jac: it is formed first, by the same operations.
struct ImuStepJac {
  M3 Ett, Ftg;             // F[theta, theta], F[theta, bg]
  M3 Fvt, Fvg, Fva;        // F[v, theta], F[v, bg], F[v, ba]
  M3 R0, R1;               // R and R'
};
CTV_DI void imu_step(Q4 &q, V3 &p, V3 &v, V3 bg, V3 ba, V3 g, V3 w0, V3 a0, V3 w1, V3 a1, double dt, bool want_jac, ImuStepJac &J) {
  const V3 u0 = a0 - ba, u1 = a1 - ba;
  const V3 phi = dt * (0.5 * (w0 + w1) - bg);
  const Q4 e = so3_exp(phi);
  const Q4 q1 = qmul_unit(q, e);
  const M3 R0 = q2R(q), R1 = q2R(q1);
  const V3 A = 0.5 * ((mul(R0, u0) - g) + (mul(R1, u1) - g));
  p = p + dt * v + (0.5 * dt * dt) * A;
  v = v + dt * A;
  q = q1;
  if (!want_jac) return;
  const M3 E = q2R(e), Jr = so3_Jr(phi);
  const M3 Ru0 = mul_hat(R0, u0), Ru1 = mul_hat(R1, u1);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) J.Ett.m[3 * i + j] = E.m[3 * j + i];
  J.Ftg = scale(Jr, -dt);
  J.Fvt = scale(add(Ru0, mulT(Ru1, E)), -0.5 * dt);
  J.Fvg = scale(mul(Ru1, Jr), 0.5 * dt * dt);
  J.Fva = scale(add(R0, R1), -0.5 * dt);
  J.R0 = R0;
  J.R1 = R1;
}

// A landmark seen from an IMU-PREDICTED pose beyond the spline (ctvio_predict_landmarks).  The end state (q, p, v) of the dead reckoning and
// the last body rate w_e = gyro - bg are carried over the read-out of image row `row` at a constant rate, delta = row * line delay:
//   R_I(tau) = R Exp(w_e delta),   p_I(tau) = p + delta v                                                       (pred_row_pose)
// and the camera pose is T_I(tau) (q_CI, p_CI).  In the tangent of ctvio_imu_predict (dtheta, dp, dv, dbg, dba) the body pose at tau moves by
//   B (6 x 15) = [[E^T, 0, 0, -delta Jr(w_e delta), 0], [0, I, delta I, 0, 0]],  E = Exp(w_e delta)   (pred_B: the blocks E^T and -delta Jr),
// the camera pose by C_ext = [[R_CI^T, 0], [-R_I(tau) [p_CI]x, I]] times that (pred_Cext: the blocks R_CI^T and -R_I(tau) [p_CI]x, the
// tangent map of pose_jac_T's extrinsic), and with dy = [y]x dtheta_C - R_C^T dp_C the image point by
//   A (2 x 15, row-major) = Pi [[y]x, -R_C^T] C_ext B                                                           (pred_A).
// delta = 0 gives E = Jr = I exactly and exact zeros in the velocity and gyro-bias columns.
CTV_DI void pred_row_pose(Q4 q, V3 p, V3 v, V3 w_e, double delta, Q4 &q_I, V3 &p_I) {
  q_I = qmul_unit(q, so3_exp(delta * w_e));
  p_I = p + delta * v;
}
CTV_DI void pred_B(V3 w_e, double delta, M3 &Et, M3 &Bg) {
  const M3 E = q2R(so3_exp(delta * w_e));
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Et.m[3 * i + j] = E.m[3 * j + i];
  Bg = scale(so3_Jr(delta * w_e), -delta);
}
CTV_DI void pred_Cext(Q4 q_CI, V3 p_CI, Q4 q_I, M3 &Rt, M3 &X) {
  const M3 R = q2R(q_CI);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rt.m[3 * i + j] = R.m[3 * j + i];
  X = scale(mul_hat(q2R(q_I), p_CI), -1.0);
}
CTV_DI void pred_A(const ProjLin &L, V3 y, const M3 &Rt, const M3 &X, const M3 &Et, const M3 &Bg, double delta, double A[30]) {
  const M3 Hy = hat(y);
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    double h[3], dth[3];   // row a of Pi [y]x, then of D_theta = Pi [y]x R_CI^T - M X (the camera-pose row against dtheta_I)
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c] = L.Pi[3 * a] * Hy.m[c] + L.Pi[3 * a + 1] * Hy.m[3 + c] + L.Pi[3 * a + 2] * Hy.m[6 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dth[c] = (h[0] * Rt.m[c] + h[1] * Rt.m[3 + c] + h[2] * Rt.m[6 + c]) - (L.M[3 * a] * X.m[c] + L.M[3 * a + 1] * X.m[3 + c] + L.M[3 * a + 2] * X.m[6 + c]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      A[15 * a + c] = dth[0] * Et.m[c] + dth[1] * Et.m[3 + c] + dth[2] * Et.m[6 + c];
      A[15 * a + 3 + c] = -L.M[3 * a + c];
      A[15 * a + 6 + c] = -(delta * L.M[3 * a + c]);
      A[15 * a + 9 + c] = dth[0] * Bg.m[c] + dth[1] * Bg.m[3 + c] + dth[2] * Bg.m[6 + c];
      A[15 * a + 12 + c] = 0.0;
    }
  }
}

// Streaming forms of the two views: the per-knot partial Jacobians are handed to `f(knot, J)` one at a time, as soon as they
// are final, instead of being returned as four 3 x 3 matrices -- the same operations in the same order (bit-identical
// values), but only ~5 matrices are live at any time (the array forms keep 11, i.e. ~200 fp64 registers for both ends).
//   EvaluateRp : J_3 = H_2 JrI_2 ; J_i = H_{i-1} JrI_{i-1} - H_i JrI_i^T ; J_0 = Apost_0 - H_0 JrI_0^T, H_i = c_{i+1} Apost_{i+1} Jr(c_{i+1} d_i):
//                Apost is built from the last knot backwards, so the knots come out 3, 2, 1, 0.
//   EvaluateRTp: H_i = c_{i+1} R(S_i) Jr(-c_{i+1} d_i), S built forwards: knots come out 0, 1, 2, 3.
template <class SC, bool SMALL = false, class F> CTV_DI void eval_Rp_jac_stream(const SC &sc, double u, F &&f) {
  double c[4];
  basis<true, 0>(u, 1.0, c);
  Q4 accq = qmk(0, 0, 0, 1);
  M3 Ap = m3_id(), pending = m3_zero();
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    const V3 kd = c[i + 1] * sc.d[i];
    const M3 Jh = scale(mul(Ap, so3_Jr_sel<SMALL>(kd)), c[i + 1]);
    const M3 JrIi = sc.jri(i);
    const M3 Jn = mul(Jh, JrIi);
    f(i + 1, i == 2 ? Jn : add(Jn, pending));
    pending = scale(mulT(Jh, JrIi), -1.0);
    accq = qmul_unit(accq, so3_exp_sel<SMALL>(neg(kd)));
    Ap = q2R(accq);
  }
  f(0, add(Ap, pending));
}
template <class SC, bool SMALL = false, class F> CTV_DI void eval_RTp_jac_stream(const Q4 q[4], const SC &sc, double u, F &&f) {
  double c[4];
  basis<true, 0>(u, 1.0, c);
  Q4 S = q[0];
  M3 pending = q2R(S);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const V3 kd = c[i + 1] * sc.d[i];
    const M3 Jh = scale(mul(q2R(S), so3_Jr_sel<SMALL>(neg(kd))), c[i + 1]);
    const M3 JrIi = sc.jri(i);
    f(i, sub(pending, mulT(Jh, JrIi)));
    pending = mul(Jh, JrIi);
    S = qmul_unit(S, so3_exp_sel<SMALL>(kd));
  }
  f(3, pending);
}

// ------------------------------------------------------------------------------------------------
// Visual block (ImageFeatureDelayFactor::Evaluate, image_feature_factor.h:63-269), FACTORED THROUGH THE ANCHOR END.
//
// The reprojection residual depends on the pose unknowns only through the 3-vector x_j (the point in camera j):
//     x_j = R_CI^T (R_Ij^T (p_G - p_Ij) - p_CI),     p_G = R_Ii p_Ii + p_IiinG   (the point in the global frame),
// so every column of the block's 2 x 50 Jacobian is A (2 x 3) times a 3-vector, A = sw J_v R_CI^T R_Ij^T (:184-197), and the
// robust corrector (linear in J) turns A into A~ once.  Everything on the anchor side of p_G -- EvaluateRp and its per-knot
// Jacobians, VelocityBody, p(t_i), v(t_i) (:104-131, 199-216) -- depends on (t_i, row_i, p_i, rho) alone, and the reference gives
// all blocks of a feature the same (t_i, row_i, p_i) (trajectory_manager.cpp:367-383): it is evaluated ONCE per anchor
// (vis_anchor_eval -> a record of AREC doubles) instead of once per block (5-6 times per landmark), and a block evaluates only its
// own j end (vis_block_eval).  Column by column (local order rot_i 12 | pos_i 12 | rot_j 12 | pos_j 12 | rho | ld):
//     rot_i (k, b)  = A~ GR_k[:, b],   GR_k = -R_Ii hat(p_Ii) J^Rp_k              (record)
//     pos_i (k, b)  = cp0[k] A~[:, b]                                              (record: cp0)
//     rot_j (k, b)  = (A~ hat(p_G - p_Ij)) J^RTp_k[:, b]                           (block)
//     pos_j (k, b)  = -cp1[k] A~[:, b]                                             (block: cp1)
//     rho           = A~ y,   y = -(1 / rho) R_Ii R_CI x_ci                        (record)
//     ld            = B~ (R_Ij^T (h - row_j v_j) - row_j Om_j x (R_Ij^T (p_G - p_Ij))),  h = row_i (v_i + R_Ii (Om_i x p_Ii))  (record),
//                     B~ = corrector(sw J_v R_CI^T), A~ = B~ R_Ij^T
// The i-end columns are never materialised per block: the assembly rebuilds them from A~ and the record, the rows of W take
// sum_b (A~^T J~_rho) over the anchor's blocks times the record.
constexpr int AREC = 50;        // doubles per anchor record
constexpr int AR_PG = 0;        // [3]  p_G
constexpr int AR_GR = 3;        // [12][3] GR[c][m] = GR_k(m, b), c = 3 k + b: the three factors of column c are consecutive
constexpr int AR_CP0 = 39;      // [4]  blending coefficients of the position spline at t_i
constexpr int AR_Y = 43;        // [3]
constexpr int AR_H = 46;        // [3]  (entry 49 unused: records are 16-byte multiples)

// q0 / p[4]: rotation of the first active knot and the positions of the four active knots of the anchor end (global frame).
template <bool SMALL, class SC>
CTV_DI void vis_anchor_eval(const Q4 &q0, const V3 p[4], const SC &sc, double u, double idt, const Q4 &q_CI,
                            const V3 &p_CI, double pix, double piy, double rowi, double d_inv, bool want_jac, double *rec) {
  const double inv_d = 1.0 / d_inv;
  const V3 c_i = qrot(q_CI, mk(pix * inv_d, piy * inv_d, inv_d));   // R_CI x_ci
  const V3 p_Ii = c_i + p_CI;
  Q4 qk[4];
  qk[0] = q0;
  const Q4 S_IitoG = eval_Rp<SC, SMALL>(qk, sc, u, (M3 *)nullptr, false);
  const M3 RIiG = q2R(S_IitoG);
  double cp0[4];
  basis<false, 0>(u, 1.0, cp0);
  V3 pI = mk(0, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) pI = pI + cp0[i] * p[i];
  const V3 pG = mul(RIiG, p_Ii) + pI;
  rec[AR_PG] = pG.x; rec[AR_PG + 1] = pG.y; rec[AR_PG + 2] = pG.z;
  if (!want_jac) return;
  double dcp0[4];
  basis<false, 1>(u, idt, dcp0);
  V3 v_i = mk(0, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) v_i = v_i + dcp0[i] * p[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) rec[AR_CP0 + i] = cp0[i];
  const V3 y = (-inv_d) * mul(RIiG, c_i);
  rec[AR_Y] = y.x; rec[AR_Y + 1] = y.y; rec[AR_Y + 2] = y.z;
  const V3 Om_i = eval_omega<SC, SMALL>(sc, u, idt);
  const V3 h = rowi * (v_i + mul(RIiG, cross(Om_i, p_Ii)));
  rec[AR_H] = h.x; rec[AR_H + 1] = h.y; rec[AR_H + 2] = h.z;
  const M3 M0 = scale(mul_hat(RIiG, p_Ii), -1.0);     // -R_Ii hat(p_Ii)
  eval_Rp_jac_stream<SC, SMALL>(sc, u, [&](int kk, const M3 &Jk) {
    const M3 G = mul(M0, Jk);
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int mm = 0; mm < 3; ++mm) rec[AR_GR + 3 * (3 * kk + b) + mm] = G.m[3 * mm + b];
  });
}

// Entries of a block's record in Dev::Jt (VT_ROWS doubles, robust-corrected): the assembly's input.
constexpr int VB_JROT = 0;      // [12][2] rotation columns of the j end: entry 2 c + residual row, c = 3 k + b
constexpr int VB_RHO = 24;      // [2]  inverse-depth column
constexpr int VB_LD = 26;       // [2]  line-delay column
constexpr int VB_RES = 28;      // [2]  r~
constexpr int VB_AT = 30;       // [3][2] A~: entry 30 + 2 m + residual row
constexpr int VB_CP1 = 36;      // [4]  blending coefficients of the position spline at t_j

// q0 / p[4]: the j end's knots.  RCIT = R_CI^T (row major).  Emit receives the block record entry by entry -- put(entry, value) --
// with the inverse-depth column first (sinks that form J_rho^T J_c need it up front); r[2] = r~; returns the block's cost rho(s)/2.
// The j end's rotation spline is walked ONCE: A_i = exp(c_{i+1} d_i) serves EvaluateRTp's chain S_{i+1} = S_i A_i
// (so3_spline_view.h:208-276), VelocityBody's conjugates (:356-411) and the Jacobian recursion, and the per-knot partial Jacobians
// J_i = H_{i-1} JrI_{i-1} - H_i JrI_i^T, H_i = c_{i+1} R(S_i) Jr(-c_{i+1} d_i) are never formed: the rotation columns need only
// E J_i with E = A~ hat(p_G - p_Ij) (2 x 3), so the recursion runs on the 2 x 3 products E H_i (a third of the multiplications).
template <bool SMALL, class SC, class Emit>
CTV_DI double vis_block_eval(const double *rec, const Q4 &q0, const V3 p[4], const SC &sc, double u, double idt,
                             const M3 &RCIT, const V3 &p_CI, double sw, double cauchy_a, double pjx, double pjy, double rowj,
                             double r[2], bool want_jac, Emit &emit) {
  double c[4], cp1[4];
  basis<true, 0>(u, 1.0, c);
  basis<false, 0>(u, 1.0, cp1);
  Q4 A[3], S[4];
  S[0] = q0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    A[i] = so3_exp_sel<SMALL>(c[i + 1] * sc.d[i]);
    S[i + 1] = qmul_unit(S[i], A[i]);
  }
  const Q4 S_GtoIj = qconj(S[3]);
  V3 pIj = mk(0, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) pIj = pIj + cp1[i] * p[i];
  const V3 dpg = mk(rec[AR_PG], rec[AR_PG + 1], rec[AR_PG + 2]) - pIj;
  const V3 bj = qrot(S_GtoIj, dpg);             // R_Ij^T (p_G - p_Ij)
  const V3 x_j = mul(RCIT, bj - p_CI);
  const double dji = 1.0 / x_j.z;
  const double r0 = sw * (x_j.x * dji - pjx), r1 = sw * (x_j.y * dji - pjy);
  // robust loss (Cauchy): rho(s) = b log(1 + s/b), rho' = 1/(1+s/b), rho'' = -rho'^2/b; corrector as marginalization_factor.cpp:39-67
  const double s = r0 * r0 + r1 * r1;
  double cost, sq = 1.0, rs = 1.0, alpha_sq = 0.0;
  if (cauchy_a > 0.0) {
    const double b = cauchy_a * cauchy_a, cc = 1.0 / b;
    const double inv = 1.0 / (1.0 + s * cc);
    cost = 0.5 * b * log1p(s * cc);
    const double rho1 = inv, rho2 = -cc * inv * inv;
    sq = sqrt(rho1);
    if (s == 0.0 || rho2 <= 0.0) { rs = sq; alpha_sq = 0.0; }
    else { const double D = 1.0 + 2.0 * s * rho2 / rho1; const double al = 1.0 - sqrt(D); rs = sq / (1.0 - al); alpha_sq = al / s; }
  } else {
    cost = 0.5 * s;
  }
  r[0] = rs * r0;
  r[1] = rs * r1;
  if (!want_jac) return cost;
  // B~ = corrector(sw J_v R_CI^T), J_v = [dji 0 -dji^2 x; 0 dji -dji^2 y] (image_feature_factor.h:184-186)
  double Bt[6], At[6];
  {
    const double fx = -dji * dji * x_j.x, fy = -dji * dji * x_j.y;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double j0 = sw * (dji * RCIT.m[k] + fx * RCIT.m[6 + k]), j1 = sw * (dji * RCIT.m[3 + k] + fy * RCIT.m[6 + k]);
      const double rj = r0 * j0 + r1 * j1;
      Bt[k] = sq * (j0 - alpha_sq * r0 * rj);
      Bt[3 + k] = sq * (j1 - alpha_sq * r1 * rj);
    }
  }
  const M3 RGIj = q2R(S_GtoIj);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int k = 0; k < 3; ++k) At[3 * a + k] = Bt[3 * a] * RGIj.m[k] + Bt[3 * a + 1] * RGIj.m[3 + k] + Bt[3 * a + 2] * RGIj.m[6 + k];
  // inverse depth (image_feature_factor.h:239-248)
  emit.put(VB_RHO, At[0] * rec[AR_Y] + At[1] * rec[AR_Y + 1] + At[2] * rec[AR_Y + 2]);
  emit.put(VB_RHO + 1, At[3] * rec[AR_Y] + At[4] * rec[AR_Y + 1] + At[5] * rec[AR_Y + 2]);
#pragma unroll
  for (int mm = 0; mm < 3; ++mm) { emit.put(VB_AT + 2 * mm, At[mm]); emit.put(VB_AT + 2 * mm + 1, At[3 + mm]); }
#pragma unroll
  for (int i = 0; i < 4; ++i) emit.put(VB_CP1 + i, cp1[i]);
  // line delay (image_feature_factor.h:251-264), in the frame of IMU j
  {
    double dc[4], dcp1[4];
    basis<true, 1>(u, idt, dc);
    basis<false, 1>(u, idt, dcp1);
    V3 v_j = mk(0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) v_j = v_j + dcp1[i] * p[i];
    V3 Om_j = dc[1] * sc.d[0];                  // VelocityBody: conj(A_i) = exp(-c_{i+1} d_i)
#pragma unroll
    for (int i = 1; i < 3; ++i) Om_j = qrot(qconj(A[i]), Om_j) + dc[i + 1] * sc.d[i];
    const V3 hv = mk(rec[AR_H], rec[AR_H + 1], rec[AR_H + 2]) - rowj * v_j;
    const V3 Jx = qrot(S_GtoIj, hv) - rowj * cross(Om_j, bj);
    emit.put(VB_LD, Bt[0] * Jx.x + Bt[1] * Jx.y + Bt[2] * Jx.z);
    emit.put(VB_LD + 1, Bt[3] * Jx.x + Bt[4] * Jx.y + Bt[5] * Jx.z);
  }
  // rotation columns of the j end (image_feature_factor.h:199-216): E = A~ hat(p_G - p_Ij), row by row A~[a] x dpg;
  // knots come out 0, 1, 2, 3
  {
    const V3 E0 = cross(mk(At[0], At[1], At[2]), dpg), E1 = cross(mk(At[3], At[4], At[5]), dpg);
    const double E[6] = {E0.x, E0.y, E0.z, E1.x, E1.y, E1.z};
    auto mul23 = [](const double X[6], const M3 &M, double Y[6]) {          // Y = X M
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) Y[3 * a + k] = X[3 * a] * M.m[k] + X[3 * a + 1] * M.m[3 + k] + X[3 * a + 2] * M.m[6 + k];
    };
    auto mul23T = [](const double X[6], const M3 &M, double Y[6]) {         // Y = X M^T
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) Y[3 * a + k] = X[3 * a] * M.m[3 * k] + X[3 * a + 1] * M.m[3 * k + 1] + X[3 * a + 2] * M.m[3 * k + 2];
    };
    double Ep[6];                                       // E times the pending term of the recursion
    mul23(E, q2R(S[0]), Ep);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double ER[6], EH[6], t6[6];
      if (i == 0) {
#pragma unroll
        for (int e = 0; e < 6; ++e) ER[e] = Ep[e];
      } else {
        mul23(E, q2R(S[i]), ER);
      }
      mul23(ER, so3_Jr_sel<SMALL>((-c[i + 1]) * sc.d[i]), EH);
#pragma unroll
      for (int e = 0; e < 6; ++e) EH[e] *= c[i + 1];
      const M3 JrIi = sc.jri(i);
      mul23T(EH, JrIi, t6);
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        emit.put(VB_JROT + 2 * (3 * i + b), Ep[b] - t6[b]);
        emit.put(VB_JROT + 2 * (3 * i + b) + 1, Ep[3 + b] - t6[3 + b]);
      }
      mul23(EH, JrIi, Ep);
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) { emit.put(VB_JROT + 2 * (9 + b), Ep[b]); emit.put(VB_JROT + 2 * (9 + b) + 1, Ep[3 + b]); }
  }
  return cost;
}

}  // namespace ctv
