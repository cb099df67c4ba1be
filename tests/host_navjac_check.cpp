// host_navjac_check.cpp -- TEST-ONLY g++ build of nav_jac_T (ctrl-vio_amd/csrc/factors.hpp), the Jacobian k_cov_nav_jac evaluates per query, so
// that it can be compared with the NumPy restatement (tests/navstate_helpers.py) on a machine without a GPU.  Never loaded by the product.
#include "../ctrl-vio_amd/csrc/factors.hpp"

using namespace ctv;

extern "C" {
// q: 4 knots x (x,y,z,w); idt = 1 / dt in 1 / s; jt: 24 x 6, jt[(6 k + c) * 6 + a] = d(pose output a) / d(unknown c of knot k); cv: c'_k(u) / dt
void hm_nav_jac(const double *q, double u, double idt, double *jt, double *cv) {
  Knots4 k;
  for (int i = 0; i < 4; ++i) { k.q[i] = qmk(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]); k.p[i] = mk(0, 0, 0); }
  SegConst sc;
  seg_const(k, sc, true);   // as the kernel: pair constants straight from the knots
  nav_jac_T(k.q, sc, u, idt, jt, cv);
}
}
