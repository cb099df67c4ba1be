// host_rates_check.cpp -- TEST-ONLY g++ build of rates_jac_T (ctrl-vio_amd/csrc/factors.hpp), the Jacobian k_cov_rates_jac evaluates per query,
// so that it can be compared with the NumPy restatement (tests/rates_helpers.py) on a machine without a GPU.  Never loaded by the product.
// The case body is mc::rates_jac_case (tests/math_cases.hpp), shared with the device build.
#include "math_cases.hpp"

extern "C" {
// q: 4 knots x (x,y,z,w); p: 4 knots x 3; idt = 1 / dt in 1 / s; g: the window's gravity; jt: 24 x 9, jt[(6 k + c) * 9 + a] = d(output a) /
// d(unknown c of knot k), outputs (omega 0..2, f 3..5, v_B 6..8)
void hm_rates_jac(const double *q, const double *p, double u, double idt, const double *g, double *jt) { mc::rates_jac_case(q, p, u, idt, g, jt); }
}
