// host_relpose_check.cpp -- TEST-ONLY g++ build of rel_pose_jac_T (ctrl-vio_amd/csrc/factors.hpp), the map k_cov_rel_jac applies to the two pose
// Jacobians of a query, so that it can be compared with the NumPy restatement (tests/relpose_helpers.py) on a machine without a GPU.  Never
// loaded by the product.  The case body is mc::rel_pose_jac_case (tests/math_cases.hpp), shared with the device build.
#include "math_cases.hpp"

extern "C" {
// qa, pa / qb, pb: the 4 knots of each time, quaternions (x,y,z,w) and positions; q_SI unit; jt_a, jt_b: 24 x 6, jt[(6 k + c) * 6 + o] =
// d(output o of the increment) / d(unknown c of knot k of that time); rel7: (p_ab, q_ab as x, y, z, w)
void hm_rel_pose_jac(const double *qa, const double *pa, double ua, const double *qb, const double *pb, double ub, int ext, const double *q_SI,
                     const double *p_SI, double *jt_a, double *jt_b, double *rel7) {
  mc::rel_pose_jac_case(qa, pa, ua, qb, pb, ub, ext, q_SI, p_SI, jt_a, jt_b, rel7);
}
}
