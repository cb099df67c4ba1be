// host_imustep_check.cpp -- TEST-ONLY g++ build of imu_step (ctrl-vio_amd/csrc/factors.hpp), the midpoint step k_imu_propagate takes per
// sample, so that its mean and blocks can be compared with the NumPy restatement (tests/imuprop_helpers.py) on a machine without a GPU.
// Never loaded by the product.  The case body is mc::imu_step_case (tests/math_cases.hpp), shared with the device build.
#include "math_cases.hpp"

extern "C" {
// x: (qx, qy, qz, qw, p 3, v 3, bg 3, ba 3) = 16 doubles, advanced in place (the biases stay); meas: w0, a0, w1, a1 (12); g: gravity.
// blocks (or null: the mean alone): seven row-major 3 x 3 blocks in the order of ImuStepJac: Ett, Ftg, Fvt, Fvg, Fva, R0, R1.
void hm_imu_step(double *x, const double *meas, const double *g, double dt, double *blocks) { mc::imu_step_case(x, meas, g, dt, blocks); }
}
