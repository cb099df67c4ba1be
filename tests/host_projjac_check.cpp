// host_projjac_check.cpp -- TEST-ONLY g++ build of proj_point / proj_lin / proj_jac_T / proj_cols (ctrl-vio_amd/csrc/factors.hpp), the maps
// k_cov_proj_jac applies to the camera-pose Jacobians of the anchor time and the query time, so that they can be compared with the NumPy
// restatement (tests/projection_helpers.py) on a machine without a GPU.  Never loaded by the product.  The case body is mc::proj_jac_case
// (tests/math_cases.hpp), shared with the device build.
#include "math_cases.hpp"

extern "C" {
// qa, pa / qq, pq: the 4 knots of the anchor / query time; idt = 1 / dt (1 / s); q_CI unit; obs3 = (px, py, rho); rows = (row_i, row_q);
// jt_a, jt_q: 24 x 2, jt[2 (6 k + c) + o] = d(proj_o) / d(unknown c of knot k of that time); out7 = (proj3, j (2), jld (2))
void hm_proj_jac(const double *qa, const double *pa, double ua, const double *qq, const double *pq, double uq, double idt, const double *q_CI_,
                 const double *p_CI_, const double *obs3, const double *rows, double *jt_a, double *jt_q, double *out7) {
  mc::proj_jac_case(qa, pa, ua, qq, pq, uq, idt, q_CI_, p_CI_, obs3, rows, jt_a, jt_q, out7);
}
}
