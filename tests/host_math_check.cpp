// host_math_check.cpp -- TEST-ONLY g++ build of the device math headers (ctrl-vio_amd/csrc/so3.hpp, factors.hpp) so that the per-block
// residual/Jacobian code of the HIP kernels can be checked against the oracle on a machine without a GPU (pytest -m "not gpu").  The case
// bodies are tests/math_cases.hpp, the text tests/device_math_probe.hip compiles for the device.  This library is never loaded by the
// product: libctvio.so has no CPU path.
#include "math_cases.hpp"

extern "C" {
void hm_imu_eval(const double *q, const double *p, double u, double idt, const double *g, const double *bias,
                 const double *gyro, const double *acc, const double *w, double *r, double *J) {
  mc::imu_eval_case(q, p, u, idt, g, bias, gyro, acc, w, r, J);
}
double hm_visual_eval(int small_angle, const double *qi, const double *pi, const double *qj, const double *pj, double ui, double uj,
                      double idt, const double *q_CI, const double *p_CI, double img_w, double cauchy_a, const double *obs,
                      double rowi, double rowj, double d_inv, double *r, double *J) {
  if (small_angle) return mc::visual_eval_case<true>(qi, pi, qj, pj, ui, uj, idt, q_CI, p_CI, img_w, cauchy_a, obs, rowi, rowj, d_inv, r, J);
  return mc::visual_eval_case<false>(qi, pi, qj, pj, ui, uj, idt, q_CI, p_CI, img_w, cauchy_a, obs, rowi, rowj, d_inv, r, J);
}
void hm_so3(const double *phi, double *exp_q, double *Jr, double *JrInv, double *log_of_exp) { mc::so3_case(phi, exp_q, Jr, JrInv, log_of_exp); }
// the further primitives of the high-precision fixture (tests/golden/lie_edge_grid.npz)
void hm_so3_small(const double *phi, double *exp_q, double *Jr) { mc::so3_small_case(phi, exp_q, Jr); }
void hm_so3_log(const double *q, double *lg) { mc::so3_log_case(q, lg); }
void hm_qmul(const double *a, const double *b, double *prod, double *prod_unit) { mc::qmul_case(a, b, prod, prod_unit); }
void hm_basis(double u, double idt, double *c) { mc::basis_case(u, idt, c); }
}
