// host_projjac_check.cpp -- TEST-ONLY g++ build of proj_point / proj_lin / proj_jac_T / proj_cols (ctrl-vio_amd/csrc/factors.hpp), the maps
// k_cov_proj_jac applies to the camera-pose Jacobians of the anchor time and the query time, so that they can be compared with the NumPy
// restatement (tests/projection_helpers.py) on a machine without a GPU.  Never loaded by the product.
#include "../ctrl-vio_amd/csrc/factors.hpp"

using namespace ctv;

namespace {
// one time, as k_cov_proj_jac's proj_side: the body pose, the body rate and world velocity, the 24 x 6 block of pose_jac_T for the camera pose
void side(const double *q, const double *p, double u, double idt, Q4 q_CI, V3 p_CI, double *jp, Q4 &q_I, V3 &p_I, V3 &om, V3 &v) {
  Knots4 k;
  for (int i = 0; i < 4; ++i) { k.q[i] = qmk(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]); k.p[i] = mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
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
}  // namespace

extern "C" {
// qa, pa / qq, pq: the 4 knots of the anchor / query time; idt = 1 / dt (1 / s); q_CI unit; obs3 = (px, py, rho); rows = (row_i, row_q);
// jt_a, jt_q: 24 x 2, jt[2 (6 k + c) + o] = d(proj_o) / d(unknown c of knot k of that time); out7 = (proj3, j (2), jld (2))
void hm_proj_jac(const double *qa, const double *pa, double ua, const double *qq, const double *pq, double uq, double idt, const double *q_CI_,
                 const double *p_CI_, const double *obs3, const double *rows, double *jt_a, double *jt_q, double *out7) {
  const Q4 q_CI = qmk(q_CI_[0], q_CI_[1], q_CI_[2], q_CI_[3]);
  const V3 p_CI = mk(p_CI_[0], p_CI_[1], p_CI_[2]);
  const double px = obs3[0], py = obs3[1], rho = obs3[2];
  double jp[144];
  Q4 q_Ii, q_Iq;
  V3 p_Ii, p_Iq, om_i, v_i, om_q, v_q;
  side(qa, pa, ua, idt, q_CI, p_CI, jp, q_Ii, p_Ii, om_i, v_i);
  const Q4 q_Ci = qmul(q_Ii, q_CI);
  const V3 p_Ci = p_Ii + qrot(q_Ii, p_CI);
  double jq[144];
  side(qq, pq, uq, idt, q_CI, p_CI, jq, q_Iq, p_Iq, om_q, v_q);
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
}
