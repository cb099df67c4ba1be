// host_posejac_check.cpp -- TEST-ONLY g++ build of pose_jac_T (ctrl-vio_amd/csrc/factors.hpp), the Jacobian k_cov_pose_jac evaluates per query, so
// that it can be compared with the NumPy restatement (tests/posecov_helpers.py) on a machine without a GPU.  Never loaded by the product.
#include "../ctrl-vio_amd/csrc/factors.hpp"

using namespace ctv;

extern "C" {
// q: 4 knots x (x,y,z,w); ext: 0 = body pose, else q_SI (unit) / p_SI; jt: 24 x 6, jt[(6 k + c) * 6 + a] = d(output a) / d(unknown c of knot k)
void hm_pose_jac(const double *q, double u, int ext, const double *q_SI, const double *p_SI, double *jt) {
  Knots4 k;
  for (int i = 0; i < 4; ++i) { k.q[i] = qmk(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]); k.p[i] = mk(0, 0, 0); }
  SegConst sc;
  seg_const(k, sc, true);   // as the kernel: pair constants straight from the knots
  pose_jac_T(k.q, sc, u, ext != 0, qmk(q_SI[0], q_SI[1], q_SI[2], q_SI[3]), mk(p_SI[0], p_SI[1], p_SI[2]), jt);
}
}
