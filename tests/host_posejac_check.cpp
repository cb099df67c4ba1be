// host_posejac_check.cpp -- TEST-ONLY g++ build of pose_jac_T (ctrl-vio_amd/csrc/factors.hpp), the Jacobian k_cov_pose_jac evaluates per query, so
// that it can be compared with the NumPy restatement (tests/posecov_helpers.py) on a machine without a GPU.  Never loaded by the product.
// The case body is mc::pose_jac_case (tests/math_cases.hpp), shared with the device build.
#include "math_cases.hpp"

extern "C" {
// q: 4 knots x (x,y,z,w); ext: 0 = body pose, else q_SI (unit) / p_SI; jt: 24 x 6, jt[(6 k + c) * 6 + a] = d(output a) / d(unknown c of knot k)
void hm_pose_jac(const double *q, double u, int ext, const double *q_SI, const double *p_SI, double *jt) { mc::pose_jac_case(q, u, ext, q_SI, p_SI, jt); }
}
