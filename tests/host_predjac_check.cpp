// host_predjac_check.cpp -- TEST-ONLY g++ build of pred_row_pose / pred_B / pred_Cext / pred_A (ctrl-vio_amd/csrc/factors.hpp), the maps
// k_cov_pred_jac applies to an IMU-predicted end state, so that they can be compared with the NumPy restatement (tests/predproj_helpers.py)
// on a machine without a GPU.  Never loaded by the product.
#include "../ctrl-vio_amd/csrc/factors.hpp"

using namespace ctv;

extern "C" {
// q_e = (x, y, z, w), p_e, v_e: the end state; w_e, delta: the read-out; X: the world point; q_CI unit, p_CI.
// pose7 = (p_I(tau), q_I(tau)); proj3; B (6 x 15), C (6 x 6), A (2 x 15), row-major and dense.
void hm_pred_jac(const double *q_e, const double *p_e, const double *v_e, const double *w_e_, double delta, const double *X_, const double *q_CI_,
                 const double *p_CI_, double *pose7, double *proj3, double *B, double *C, double *A) {
  const Q4 q_CI = qmk(q_CI_[0], q_CI_[1], q_CI_[2], q_CI_[3]);
  const V3 p_CI = mk(p_CI_[0], p_CI_[1], p_CI_[2]), w_e = mk(w_e_[0], w_e_[1], w_e_[2]), X = mk(X_[0], X_[1], X_[2]);
  Q4 q_I;
  V3 p_I;
  pred_row_pose(qmk(q_e[0], q_e[1], q_e[2], q_e[3]), mk(p_e[0], p_e[1], p_e[2]), mk(v_e[0], v_e[1], v_e[2]), w_e, delta, q_I, p_I);
  pose7[0] = p_I.x; pose7[1] = p_I.y; pose7[2] = p_I.z; pose7[3] = q_I.x; pose7[4] = q_I.y; pose7[5] = q_I.z; pose7[6] = q_I.w;
  const Q4 q_C = qmul(q_I, q_CI);
  const V3 p_C = p_I + qrot(q_I, p_CI);
  const V3 y = qrot(qconj(q_C), X - p_C);   // R_C^T (X - p_C)
  proj3[0] = y.x / y.z; proj3[1] = y.y / y.z; proj3[2] = y.z;
  const ProjLin L = proj_lin(q_C, y);
  M3 Et, Bg, Rt, Xm;
  pred_B(w_e, delta, Et, Bg);
  pred_Cext(q_CI, p_CI, q_I, Rt, Xm);
  pred_A(L, y, Rt, Xm, Et, Bg, delta, A);
  for (int i = 0; i < 90; ++i) B[i] = 0.0;
  for (int i = 0; i < 36; ++i) C[i] = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      B[15 * i + j] = Et.m[3 * i + j];
      B[15 * i + 9 + j] = Bg.m[3 * i + j];
      B[15 * (3 + i) + 3 + j] = i == j ? 1.0 : 0.0;
      B[15 * (3 + i) + 6 + j] = i == j ? delta : 0.0;
      C[6 * i + j] = Rt.m[3 * i + j];
      C[6 * (3 + i) + j] = Xm.m[3 * i + j];
      C[6 * (3 + i) + 3 + j] = i == j ? 1.0 : 0.0;
    }
}
}
