// host_navjac_check.cpp -- TEST-ONLY g++ build of nav_jac_T (ctrl-vio_amd/csrc/factors.hpp), the Jacobian k_cov_nav_jac evaluates per query, so
// that it can be compared with the NumPy restatement (tests/navstate_helpers.py) on a machine without a GPU.  Never loaded by the product.
// The case body is mc::nav_jac_case (tests/math_cases.hpp), shared with the device build.
#include "math_cases.hpp"

extern "C" {
// q: 4 knots x (x,y,z,w); idt = 1 / dt in 1 / s; jt: 24 x 6, jt[(6 k + c) * 6 + a] = d(pose output a) / d(unknown c of knot k); cv: c'_k(u) / dt
void hm_nav_jac(const double *q, double u, double idt, double *jt, double *cv) { mc::nav_jac_case(q, u, idt, jt, cv); }
}
