// host_lspoly_check.cpp -- TEST-ONLY g++ build of the line-search interpolation (ctrl-vio_amd/csrc/ls_poly.hpp), the step lm_decide takes on
// one lane of k_pass_end, so that it can be compared with NumPy's solve / roots on a machine without a GPU.  Never loaded by the product.
// The case body is mc::ls_minimize_case (tests/math_cases.hpp), shared with the device build.
#include "math_cases.hpp"

extern "C" {
// ns samples (abscissa x, value v, gradient g); the minimiser of the interpolating polynomial over [lo, hi]; coef (or null): its 6 coefficients
double hl_ls_minimize(int ns, const double *x, const double *v, const double *g, double lo, double hi, double *coef) {
  return mc::ls_minimize_case(ns, x, v, g, lo, hi, coef);
}
// real parts of the roots of a polynomial of n <= 5 coefficients, highest power first; returns their number
int hl_ls_roots(int n, const double *p, double *re) { return mc::ls_roots_case(n, p, re); }
}
