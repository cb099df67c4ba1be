// host_imustep_check.cpp -- TEST-ONLY g++ build of imu_step (ctrl-vio_amd/csrc/factors.hpp), the midpoint step k_imu_propagate takes per
// sample, so that its mean and blocks can be compared with the NumPy restatement (tests/imuprop_helpers.py) on a machine without a GPU.
// Never loaded by the product.
#include "../ctrl-vio_amd/csrc/factors.hpp"

using namespace ctv;

extern "C" {
// x: (qx, qy, qz, qw, p 3, v 3, bg 3, ba 3) = 16 doubles, advanced in place (the biases stay); meas: w0, a0, w1, a1 (12); g: gravity.
// blocks (or null: the mean alone): seven row-major 3 x 3 blocks in the order of ImuStepJac: Ett, Ftg, Fvt, Fvg, Fva, R0, R1.
void hm_imu_step(double *x, const double *meas, const double *g, double dt, double *blocks) {
  Q4 q = qmk(x[0], x[1], x[2], x[3]);
  V3 p = mk(x[4], x[5], x[6]), v = mk(x[7], x[8], x[9]);
  const V3 bg = mk(x[10], x[11], x[12]), ba = mk(x[13], x[14], x[15]);
  ImuStepJac J;
  imu_step(q, p, v, bg, ba, mk(g[0], g[1], g[2]), mk(meas[0], meas[1], meas[2]), mk(meas[3], meas[4], meas[5]), mk(meas[6], meas[7], meas[8]),
           mk(meas[9], meas[10], meas[11]), dt, blocks != nullptr, J);
  x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  x[4] = p.x; x[5] = p.y; x[6] = p.z; x[7] = v.x; x[8] = v.y; x[9] = v.z;
  if (!blocks) return;
  const M3 *b[7] = {&J.Ett, &J.Ftg, &J.Fvt, &J.Fvg, &J.Fva, &J.R0, &J.R1};
  for (int i = 0; i < 7; ++i)
    for (int e = 0; e < 9; ++e) blocks[9 * i + e] = b[i]->m[e];
}
}
