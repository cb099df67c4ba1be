// host_predjac_check.cpp -- TEST-ONLY g++ build of pred_row_pose / pred_B / pred_Cext / pred_A (ctrl-vio_amd/csrc/factors.hpp), the maps
// k_cov_pred_jac applies to an IMU-predicted end state, so that they can be compared with the NumPy restatement (tests/predproj_helpers.py)
// on a machine without a GPU.  Never loaded by the product.  The case body is mc::pred_jac_case (tests/math_cases.hpp), shared with the
// device build.
#include "math_cases.hpp"

extern "C" {
// q_e = (x, y, z, w), p_e, v_e: the end state; w_e, delta: the read-out; X: the world point; q_CI unit, p_CI.
// pose7 = (p_I(tau), q_I(tau)); proj3; B (6 x 15), C (6 x 6), A (2 x 15), row-major and dense.
void hm_pred_jac(const double *q_e, const double *p_e, const double *v_e, const double *w_e_, double delta, const double *X_, const double *q_CI_,
                 const double *p_CI_, double *pose7, double *proj3, double *B, double *C, double *A) {
  mc::pred_jac_case(q_e, p_e, v_e, w_e_, delta, X_, q_CI_, p_CI_, pose7, proj3, B, C, A);
}
}
