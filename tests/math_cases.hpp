// math_cases.hpp -- TEST-ONLY: one case = one call of the device math (ctrl-vio_amd/csrc/so3.hpp, factors.hpp, ls_poly.hpp) on plain
// pointers.  The same text is compiled twice: by g++ into the tests/host_*_check.cpp libraries (the extern "C" wrappers there only
// forward to these bodies) and by hipcc for gfx950 into tests/device_math_probe.hip (one thread per case), so the host tests and the
// GPU test of tests/test_gpu_device_math.py cannot drift apart.  Never included by the product.
#pragma once
#include "../ctrl-vio_amd/csrc/factors.hpp"
#include "../ctrl-vio_amd/csrc/ls_poly.hpp"

namespace mc {
using namespace ctv;
constexpr int VT_ROWS_HOST = 40;   // = device_types.hpp: VT_ROWS (entries of a block record)

struct ImuSink {
  double *J;
  CTV_DI void put_col(int col, const double v[6]) { for (int r = 0; r < 6; ++r) J[r * 30 + col] = v[r]; }
};
struct RecSink {
  double *e;
  CTV_DI void put(int entry, double v) { e[entry] = v; }
};

// local frame of the reference knot (q_ref, p_ref): the same preparation the kernels do (LocalFrame in kernels.hpp)
struct HostLocalFrame {
  Q4 qi; M3 RT; double o[3];
  CTV_DI HostLocalFrame(const double *q, const double *p) {
    qi = qmk(-q[0], -q[1], -q[2], q[3]);
    const M3 R = q2R(qmk(q[0], q[1], q[2], q[3]));
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) RT.m[3 * i + j] = R.m[3 * j + i];
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
  }
  CTV_DI void load(const double *q, const double *p, Knots4 &k) const {
    for (int i = 0; i < 4; ++i) {
      const Q4 ql = qmul(qi, qmk(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]));
      const V3 pl = mul(RT, mk(p[3 * i] - o[0], p[3 * i + 1] - o[1], p[3 * i + 2] - o[2]));
      k.q[i] = qmk(ql.x, ql.y, ql.z, ql.w);
      k.p[i] = mk(pl.x, pl.y, pl.z);
    }
  }
  CTV_DI M3 RrefT() const { M3 r; for (int i = 0; i < 9; ++i) r.m[i] = RT.m[i]; return r; }
  CTV_DI V3 rotate(const double *v) const { const V3 r = mul(RT, mk(v[0], v[1], v[2])); return mk(r.x, r.y, r.z); }
};

CTV_DI void load_knots(const double *q, const double *p, Knots4 &k) {   // p null: rotations only
  for (int i = 0; i < 4; ++i) {
    k.q[i] = qmk(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
    k.p[i] = p ? mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]) : mk(0, 0, 0);
  }
}

// ---- the IMU block: r (6), J (6 x 30, row-major)
CTV_DI void imu_eval_case(const double *q, const double *p, double u, double idt, const double *g, const double *bias,
                          const double *gyro, const double *acc, const double *w, double *r, double *J) {
  Knots4 k;
  HostLocalFrame lf(q, p);
  lf.load(q, p, k);
  SegConst sc;   // as on the device: pair constants from the fp64 table (k_knot_prep)
  {
    double dt[9]; double jt[27];
    for (int i = 0; i < 3; ++i) knot_pair_const(q + 4 * i, q + 4 * i + 4, dt + 3 * i, jt + 9 * i);
    seg_const_load(dt, jt, sc, true);
  }
  double b[6], gy[3], ac[3], ww[6], rr[6], JJ[180];
  for (int i = 0; i < 6; ++i) { b[i] = bias[i]; ww[i] = w[i]; }
  for (int i = 0; i < 3; ++i) { gy[i] = gyro[i]; ac[i] = acc[i]; }
  for (int i = 0; i < 180; ++i) JJ[i] = 0;
  ImuSink sink{JJ};
  imu_eval(k, sc, u, idt, lf.rotate(g), b, gy, ac, ww, lf.RrefT(), rr, true, sink);
  for (int i = 0; i < 6; ++i) r[i] = rr[i];
  for (int i = 0; i < 180; ++i) J[i] = JJ[i];
}

// The factored visual block (factors.hpp: vis_anchor_eval + vis_block_eval), composed back into the reference's 2 x 50 Jacobian
// (local column order rot_i 12 | pos_i 12 | rot_j 12 | pos_j 12 | rho | ld) exactly as the kernels consume it: i-end rotation
// columns = A~ GR, position columns = cp0 / -cp1 times A~.
template <bool SMALL>
CTV_DI double visual_eval_case(const double *qi, const double *pi, const double *qj, const double *pj, double ui, double uj,
                               double idt, const double *q_CI, const double *p_CI, double img_w, double cauchy_a, const double *obs,
                               double rowi, double rowj, double d_inv, double *r, double *J) {
  SegConst sci, scj;   // as on the device: pair constants from the fp64 table (k_knot_prep)
  {
    double dt[9], jt[27];
    for (int i = 0; i < 3; ++i) knot_pair_const(qi + 4 * i, qi + 4 * i + 4, dt + 3 * i, jt + 9 * i);
    seg_const_load(dt, jt, sci, true);
    for (int i = 0; i < 3; ++i) knot_pair_const(qj + 4 * i, qj + 4 * i + 4, dt + 3 * i, jt + 9 * i);
    seg_const_load(dt, jt, scj, true);
  }
  V3 Pi[4], Pj[4];
  for (int i = 0; i < 4; ++i) { Pi[i] = mk(pi[3 * i], pi[3 * i + 1], pi[3 * i + 2]); Pj[i] = mk(pj[3 * i], pj[3 * i + 1], pj[3 * i + 2]); }
  const Q4 qci = qmk(q_CI[0], q_CI[1], q_CI[2], q_CI[3]);
  const V3 pci = mk(p_CI[0], p_CI[1], p_CI[2]);
  double rec[AREC];
  vis_anchor_eval<SMALL>(qmk(qi[0], qi[1], qi[2], qi[3]), Pi, sci, ui, idt, qci, pci, obs[0], obs[1], rowi, d_inv, true, rec);
  const M3 R = q2R(qci);
  M3 RCIT;
  for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) RCIT.m[3 * a + b] = R.m[3 * b + a];
  double blk[VT_ROWS_HOST];
  for (int i = 0; i < VT_ROWS_HOST; ++i) blk[i] = 0;
  RecSink sink{blk};
  const double cost = vis_block_eval<SMALL>(rec, qmk(qj[0], qj[1], qj[2], qj[3]), Pj, scj, uj, idt, RCIT, pci, img_w, cauchy_a, obs[2], obs[3],
                                            rowj, r, true, sink);
  for (int rr = 0; rr < 2; ++rr) {
    double *Jr = J + 50 * rr;
    const double At[3] = {blk[VB_AT + rr], blk[VB_AT + 2 + rr], blk[VB_AT + 4 + rr]};
    for (int c = 0; c < 12; ++c) {
      Jr[c] = At[0] * rec[AR_GR + 3 * c] + At[1] * rec[AR_GR + 3 * c + 1] + At[2] * rec[AR_GR + 3 * c + 2];
      Jr[24 + c] = blk[VB_JROT + 2 * c + rr];
    }
    for (int k = 0; k < 4; ++k)
      for (int b = 0; b < 3; ++b) { Jr[12 + 3 * k + b] = rec[AR_CP0 + k] * At[b]; Jr[36 + 3 * k + b] = -blk[VB_CP1 + k] * At[b]; }
    Jr[48] = blk[VB_RHO + rr];
    Jr[49] = blk[VB_LD + rr];
  }
  return cost;
}

// ---- the Lie primitives of so3.hpp
CTV_DI void so3_case(const double *phi, double *exp_q, double *Jr, double *JrInv, double *log_of_exp) {
  V3 v = mk(phi[0], phi[1], phi[2]);
  Q4 q = so3_exp(v);
  exp_q[0] = q.x; exp_q[1] = q.y; exp_q[2] = q.z; exp_q[3] = q.w;
  M3 a = so3_Jr(v), b = so3_Jr_inv(v);
  for (int i = 0; i < 9; ++i) { Jr[i] = a.m[i]; JrInv[i] = b.m[i]; }
  V3 l = so3_log(q);
  log_of_exp[0] = l.x; log_of_exp[1] = l.y; log_of_exp[2] = l.z;
}
// the series-only forms (|phi| < 0.5: the caller's contract)
CTV_DI void so3_small_case(const double *phi, double *exp_q, double *Jr) {
  const V3 v = mk(phi[0], phi[1], phi[2]);
  const Q4 q = so3_exp_small(v);
  exp_q[0] = q.x; exp_q[1] = q.y; exp_q[2] = q.z; exp_q[3] = q.w;
  const M3 a = so3_Jr_small(v);
  for (int i = 0; i < 9; ++i) Jr[i] = a.m[i];
}
CTV_DI void so3_log_case(const double *q, double *lg) {
  const V3 l = so3_log(qmk(q[0], q[1], q[2], q[3]));
  lg[0] = l.x; lg[1] = l.y; lg[2] = l.z;
}
// qmul (Sophus' renormalisation) and qmul_unit (its expansion) of the same pair
CTV_DI void qmul_case(const double *a, const double *b, double *prod, double *prod_unit) {
  const Q4 qa = qmk(a[0], a[1], a[2], a[3]), qb = qmk(b[0], b[1], b[2], b[3]);
  const Q4 o = qmul(qa, qb), ou = qmul_unit(qa, qb);
  prod[0] = o.x; prod[1] = o.y; prod[2] = o.z; prod[3] = o.w;
  prod_unit[0] = ou.x; prod_unit[1] = ou.y; prod_unit[2] = ou.z; prod_unit[3] = ou.w;
}
// c: 6 x 4 = basis<true, D> for D = 0, 1, 2, then basis<false, D>, each with idt_pow = idt^D
CTV_DI void basis_case(double u, double idt, double *c) {
  basis<true, 0>(u, 1.0, c);
  basis<true, 1>(u, idt, c + 4);
  basis<true, 2>(u, idt * idt, c + 8);
  basis<false, 0>(u, 1.0, c + 12);
  basis<false, 1>(u, idt, c + 16);
  basis<false, 2>(u, idt * idt, c + 20);
}

// ---- the query Jacobians
// q: 4 knots x (x,y,z,w); ext: 0 = body pose, else q_SI (unit) / p_SI; jt: 24 x 6, jt[(6 k + c) * 6 + a] = d(output a) / d(unknown c of knot k)
CTV_DI void pose_jac_case(const double *q, double u, int ext, const double *q_SI, const double *p_SI, double *jt) {
  Knots4 k;
  load_knots(q, nullptr, k);
  SegConst sc;
  seg_const(k, sc, true);   // as the kernel: pair constants straight from the knots
  pose_jac_T(k.q, sc, u, ext != 0, qmk(q_SI[0], q_SI[1], q_SI[2], q_SI[3]), mk(p_SI[0], p_SI[1], p_SI[2]), jt);
}
// idt = 1 / dt in 1 / s; jt: 24 x 6 as pose_jac_case; cv: c'_k(u) / dt
CTV_DI void nav_jac_case(const double *q, double u, double idt, double *jt, double *cv) {
  Knots4 k;
  load_knots(q, nullptr, k);
  SegConst sc;
  seg_const(k, sc, true);   // as the kernel: pair constants straight from the knots
  nav_jac_T(k.q, sc, u, idt, jt, cv);
}
// p: 4 knots x 3; g: the window's gravity; jt: 24 x 9, jt[(6 k + c) * 9 + a] = d(output a) / d(unknown c of knot k), outputs
// (omega 0..2, f 3..5, v_B 6..8)
CTV_DI void rates_jac_case(const double *q, const double *p, double u, double idt, const double *g, double *jt) {
  Knots4 k;
  load_knots(q, p, k);
  SegConst sc;
  seg_const(k, sc, true);   // as the kernel: pair constants straight from the knots
  rates_jac_T(k, sc, u, idt, mk(g[0], g[1], g[2]), jt);
}

// one time of the pair, as k_cov_rel_jac's rel_side: the pose (with the extrinsic applied) and the 24 x 6 block of pose_jac_T
CTV_DI void rel_side(const double *q, const double *p, double u, int ext, const double *q_SI, const double *p_SI, double *jt, Q4 &qo, V3 &po) {
  Knots4 k;
  load_knots(q, p, k);
  SegConst sc;
  seg_const(k, sc, true);   // as the kernel: pair constants straight from the knots
  double c[4];
  basis<false, 0>(u, 1.0, c);
  V3 pp = mk(0, 0, 0);
  for (int j = 0; j < 4; ++j) pp = pp + c[j] * k.p[j];
  const Q4 qq = eval_R(k.q, sc, u);
  const Q4 qe = qmk(q_SI[0], q_SI[1], q_SI[2], q_SI[3]);
  const V3 pe = mk(p_SI[0], p_SI[1], p_SI[2]);
  qo = ext ? qmul(qq, qe) : qq;
  po = ext ? pp + qrot(qq, pe) : pp;
  pose_jac_T(k.q, sc, u, ext != 0, qe, pe, jt);
}
// qa, pa / qb, pb: the 4 knots of each time, quaternions (x,y,z,w) and positions; q_SI unit; jt_a, jt_b: 24 x 6, jt[(6 k + c) * 6 + o] =
// d(output o of the increment) / d(unknown c of knot k of that time); rel7: (p_ab, q_ab as x, y, z, w)
CTV_DI void rel_pose_jac_case(const double *qa, const double *pa, double ua, const double *qb, const double *pb, double ub, int ext,
                              const double *q_SI, const double *p_SI, double *jt_a, double *jt_b, double *rel7) {
  Q4 q_a, q_b, q_ab;
  V3 p_a, p_b, p_ab;
  rel_side(qa, pa, ua, ext, q_SI, p_SI, jt_a, q_a, p_a);
  rel_side(qb, pb, ub, ext, q_SI, p_SI, jt_b, q_b, p_b);
  rel_pose_jac_T(q_a, p_a, q_b, p_b, jt_a, jt_b, q_ab, p_ab);
  rel7[0] = p_ab.x; rel7[1] = p_ab.y; rel7[2] = p_ab.z;
  rel7[3] = q_ab.x; rel7[4] = q_ab.y; rel7[5] = q_ab.z; rel7[6] = q_ab.w;
}

// one time, as k_cov_proj_jac's proj_side: the body pose, the body rate and world velocity, the 24 x 6 block of pose_jac_T for the camera pose
CTV_DI void proj_side(const double *q, const double *p, double u, double idt, Q4 q_CI, V3 p_CI, double *jp, Q4 &q_I, V3 &p_I, V3 &om, V3 &v) {
  Knots4 k;
  load_knots(q, p, k);
  SegConst sc;
  seg_const(k, sc, true);   // as the kernel: pair constants straight from the knots
  double c[4], dc[4];
  basis<false, 0>(u, 1.0, c);
  basis<false, 1>(u, idt, dc);
  p_I = mk(0, 0, 0); v = mk(0, 0, 0);
  for (int j = 0; j < 4; ++j) { p_I = p_I + c[j] * k.p[j]; v = v + dc[j] * k.p[j]; }
  q_I = eval_R(k.q, sc, u);
  om = eval_omega<SegConst>(sc, u, idt);
  pose_jac_T(k.q, sc, u, true, q_CI, p_CI, jp);
}
// qa, pa / qq, pq: the 4 knots of the anchor / query time; idt = 1 / dt (1 / s); q_CI unit; obs3 = (px, py, rho); rows = (row_i, row_q);
// jt_a, jt_q: 24 x 2, jt[2 (6 k + c) + o] = d(proj_o) / d(unknown c of knot k of that time); out7 = (proj3, j (2), jld (2))
CTV_DI void proj_jac_case(const double *qa, const double *pa, double ua, const double *qq, const double *pq, double uq, double idt,
                          const double *q_CI_, const double *p_CI_, const double *obs3, const double *rows, double *jt_a, double *jt_q,
                          double *out7) {
  const Q4 q_CI = qmk(q_CI_[0], q_CI_[1], q_CI_[2], q_CI_[3]);
  const V3 p_CI = mk(p_CI_[0], p_CI_[1], p_CI_[2]);
  const double px = obs3[0], py = obs3[1], rho = obs3[2];
  double jp[144];
  Q4 q_Ii, q_Iq;
  V3 p_Ii, p_Iq, om_i, v_i, om_q, v_q;
  proj_side(qa, pa, ua, idt, q_CI, p_CI, jp, q_Ii, p_Ii, om_i, v_i);
  const Q4 q_Ci = qmul(q_Ii, q_CI);
  const V3 p_Ci = p_Ii + qrot(q_Ii, p_CI);
  double jq[144];
  proj_side(qq, pq, uq, idt, q_CI, p_CI, jq, q_Iq, p_Iq, om_q, v_q);
  const Q4 q_Cq = qmul(q_Iq, q_CI);
  const V3 p_Cq = p_Iq + qrot(q_Iq, p_CI);
  const V3 y = proj_point(q_Ci, p_Ci, q_Cq, p_Cq, px, py, rho);
  const ProjLin L = proj_lin(q_Cq, y);
  const M3 R_Ci = q2R(q_Ci);
  const double z = 1.0 / rho;
  const V3 x_c = mk(px * z, py * z, z);
  proj_jac_T(L, false, R_Ci, x_c, y, jp, jt_a);
  proj_jac_T(L, true, R_Ci, x_c, y, jq, jt_q);
  out7[0] = y.x / y.z; out7[1] = y.y / y.z; out7[2] = y.z;
  proj_cols(L, R_Ci, px, py, rho, y, q_CI, p_CI, rows[0], q2R(q_Ii), om_i, v_i, rows[1], q_Iq, om_q, v_q, out7 + 3, out7 + 5);
}

// q_e = (x, y, z, w), p_e, v_e: the end state; w_e, delta: the read-out; X: the world point; q_CI unit, p_CI.
// pose7 = (p_I(tau), q_I(tau)); proj3; B (6 x 15), C (6 x 6), A (2 x 15), row-major and dense.
CTV_DI void pred_jac_case(const double *q_e, const double *p_e, const double *v_e, const double *w_e_, double delta, const double *X_,
                          const double *q_CI_, const double *p_CI_, double *pose7, double *proj3, double *B, double *C, double *A) {
  const Q4 q_CI = qmk(q_CI_[0], q_CI_[1], q_CI_[2], q_CI_[3]);
  const V3 p_CI = mk(p_CI_[0], p_CI_[1], p_CI_[2]), w_e = mk(w_e_[0], w_e_[1], w_e_[2]), X = mk(X_[0], X_[1], X_[2]);
  Q4 q_I;
  V3 p_I;
  pred_row_pose(qmk(q_e[0], q_e[1], q_e[2], q_e[3]), mk(p_e[0], p_e[1], p_e[2]), mk(v_e[0], v_e[1], v_e[2]), w_e, delta, q_I, p_I);
  pose7[0] = p_I.x; pose7[1] = p_I.y; pose7[2] = p_I.z; pose7[3] = q_I.x; pose7[4] = q_I.y; pose7[5] = q_I.z; pose7[6] = q_I.w;
  const Q4 q_C = qmul(q_I, q_CI);
  const V3 p_C = p_I + qrot(q_I, p_CI);
  const V3 y = qrot(qconj(q_C), X - p_C);   // R_C^T (X - p_C)
  proj3[0] = y.x / y.z; proj3[1] = y.y / y.z; proj3[2] = y.z;
  const ProjLin L = proj_lin(q_C, y);
  M3 Et, Bg, Rt, Xm;
  pred_B(w_e, delta, Et, Bg);
  pred_Cext(q_CI, p_CI, q_I, Rt, Xm);
  pred_A(L, y, Rt, Xm, Et, Bg, delta, A);
  for (int i = 0; i < 90; ++i) B[i] = 0.0;
  for (int i = 0; i < 36; ++i) C[i] = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      B[15 * i + j] = Et.m[3 * i + j];
      B[15 * i + 9 + j] = Bg.m[3 * i + j];
      B[15 * (3 + i) + 3 + j] = i == j ? 1.0 : 0.0;
      B[15 * (3 + i) + 6 + j] = i == j ? delta : 0.0;
      C[6 * i + j] = Rt.m[3 * i + j];
      C[6 * (3 + i) + j] = Xm.m[3 * i + j];
      C[6 * (3 + i) + 3 + j] = i == j ? 1.0 : 0.0;
    }
}

// x: (qx, qy, qz, qw, p 3, v 3, bg 3, ba 3) = 16 doubles, advanced in place (the biases stay); meas: w0, a0, w1, a1 (12); g: gravity.
// blocks (or null: the mean alone): seven row-major 3 x 3 blocks in the order of ImuStepJac: Ett, Ftg, Fvt, Fvg, Fva, R0, R1.
CTV_DI void imu_step_case(double *x, const double *meas, const double *g, double dt, double *blocks) {
  Q4 q = qmk(x[0], x[1], x[2], x[3]);
  V3 p = mk(x[4], x[5], x[6]), v = mk(x[7], x[8], x[9]);
  const V3 bg = mk(x[10], x[11], x[12]), ba = mk(x[13], x[14], x[15]);
  ImuStepJac J;
  imu_step(q, p, v, bg, ba, mk(g[0], g[1], g[2]), mk(meas[0], meas[1], meas[2]), mk(meas[3], meas[4], meas[5]), mk(meas[6], meas[7], meas[8]),
           mk(meas[9], meas[10], meas[11]), dt, blocks != nullptr, J);
  x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  x[4] = p.x; x[5] = p.y; x[6] = p.z; x[7] = v.x; x[8] = v.y; x[9] = v.z;
  if (!blocks) return;
  const M3 *b[7] = {&J.Ett, &J.Ftg, &J.Fvt, &J.Fvg, &J.Fva, &J.R0, &J.R1};
  for (int i = 0; i < 7; ++i)
    for (int e = 0; e < 9; ++e) blocks[9 * i + e] = b[i]->m[e];
}

// ---- the line-search interpolation (ls_poly.hpp): ns samples (x, value, gradient), the minimiser over [lo, hi].  coef (or null): the 2 ns
// coefficients of the interpolating polynomial as the elimination left them, highest power first, zeros behind them (6 in all).
// The work arrays are a private struct of the calling thread here; k_pass_end keeps them in LDS and calls from one lane of a 256-thread
// block.  The arithmetic is the same text, the address space and the inlining context are not: this is not a bit-identical copy of k_pass_end.
CTV_DI double ls_minimize_case(int ns, const double *x, const double *v, const double *g, double lo, double hi, double *coef) {
  LsWork ws;
  for (int i = 0; i < 6; ++i) ws.coef[i] = 0.0;
  for (int i = 0; i < ns; ++i) ws.sp[i] = LsSample{x[i], v[i], g[i]};   // (where lm_decide puts them)
  const double step = ls_minimize_interpolating(ws.sp, ns, lo, hi, ws);
  if (coef) for (int i = 0; i < 6; ++i) coef[i] = i < 2 * ns ? ws.coef[i] : 0.0;
  return step;
}
// ls_root_real_parts on its own: p = n <= 5 coefficients, highest power first; re[4] (entries past the count are left alone); the count
CTV_DI int ls_roots_case(int n, const double *p, double *re) {
  LsWork ws;
  return ls_root_real_parts(p, n, re, ws);
}

}  // namespace mc
