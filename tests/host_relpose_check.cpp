// host_relpose_check.cpp -- TEST-ONLY g++ build of rel_pose_jac_T (ctrl-vio_amd/csrc/factors.hpp), the map k_cov_rel_jac applies to the two pose
// Jacobians of a query, so that it can be compared with the NumPy restatement (tests/relpose_helpers.py) on a machine without a GPU.  Never
// loaded by the product.
#include "../ctrl-vio_amd/csrc/factors.hpp"

using namespace ctv;

namespace {
// one time of the pair, as k_cov_rel_jac's rel_side: the pose (with the extrinsic applied) and the 24 x 6 block of pose_jac_T
void side(const double *q, const double *p, double u, int ext, const double *q_SI, const double *p_SI, double *jt, Q4 &qo, V3 &po) {
  Knots4 k;
  for (int i = 0; i < 4; ++i) { k.q[i] = qmk(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]); k.p[i] = mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
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
}  // namespace

extern "C" {
// qa, pa / qb, pb: the 4 knots of each time, quaternions (x,y,z,w) and positions; q_SI unit; jt_a, jt_b: 24 x 6, jt[(6 k + c) * 6 + o] =
// d(output o of the increment) / d(unknown c of knot k of that time); rel7: (p_ab, q_ab as x, y, z, w)
void hm_rel_pose_jac(const double *qa, const double *pa, double ua, const double *qb, const double *pb, double ub, int ext, const double *q_SI,
                     const double *p_SI, double *jt_a, double *jt_b, double *rel7) {
  Q4 q_a, q_b, q_ab;
  V3 p_a, p_b, p_ab;
  side(qa, pa, ua, ext, q_SI, p_SI, jt_a, q_a, p_a);
  side(qb, pb, ub, ext, q_SI, p_SI, jt_b, q_b, p_b);
  rel_pose_jac_T(q_a, p_a, q_b, p_b, jt_a, jt_b, q_ab, p_ab);
  rel7[0] = p_ab.x; rel7[1] = p_ab.y; rel7[2] = p_ab.z;
  rel7[3] = q_ab.x; rel7[4] = q_ab.y; rel7[5] = q_ab.z; rel7[6] = q_ab.w;
}
}
