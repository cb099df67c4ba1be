// host_rates_check.cpp -- TEST-ONLY g++ build of rates_jac_T (ctrl-vio_amd/csrc/factors.hpp), the Jacobian k_cov_rates_jac evaluates per query,
// so that it can be compared with the NumPy restatement (tests/rates_helpers.py) on a machine without a GPU.  Never loaded by the product.
#include "../ctrl-vio_amd/csrc/factors.hpp"

using namespace ctv;

extern "C" {
// q: 4 knots x (x,y,z,w); p: 4 knots x 3; idt = 1 / dt in 1 / s; g: the window's gravity; jt: 24 x 9, jt[(6 k + c) * 9 + a] = d(output a) /
// d(unknown c of knot k), outputs (omega 0..2, f 3..5, v_B 6..8)
void hm_rates_jac(const double *q, const double *p, double u, double idt, const double *g, double *jt) {
  Knots4 k;
  for (int i = 0; i < 4; ++i) { k.q[i] = qmk(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]); k.p[i] = mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
  SegConst sc;
  seg_const(k, sc, true);   // as the kernel: pair constants straight from the knots
  rates_jac_T(k, sc, u, idt, mk(g[0], g[1], g[2]), jt);
}
}
