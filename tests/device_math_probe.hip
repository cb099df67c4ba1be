// device_math_probe.hip -- TEST-ONLY gfx950 build of the device math (ctrl-vio_amd/csrc/so3.hpp, factors.hpp, ls_poly.hpp): the case bodies
// of tests/math_cases.hpp, the text the g++ host checks run, one thread per case.  Built to tests/_build/libdevprobe.so with the hipcc line
// of the product (ctrl-vio_amd/capi.py: hipcc_command) and loaded only by tests/test_gpu_device_math.py; never by the product.
//
// Every entry dp_<name>(n, inputs..., outputs...) takes host pointers to n cases stored back to back, allocates, copies in (outputs too: an
// entry the case leaves alone comes back as it went in), launches ceil(n / 64) blocks of 64 threads with an i >= n guard, synchronises, copies
// the outputs back, frees, and returns the first non-zero HIP status (0 = success).
#include "math_cases.hpp"

#include <vector>

namespace {

// device copies of one entry's arrays; the first failing HIP call is kept and every later step is skipped
class Stage {
 public:
  template <class T> const T *in(const T *h, size_t count) { return static_cast<const T *>(put(const_cast<T *>(h), count * sizeof(T), false)); }
  template <class T> T *out(T *h, size_t count) { return static_cast<T *>(put(h, count * sizeof(T), true)); }
  bool ok() const { return st_ == hipSuccess; }
  void check(hipError_t e) { if (st_ == hipSuccess) st_ = e; }
  int finish() {
    if (ok()) check(hipGetLastError());
    if (ok()) check(hipDeviceSynchronize());
    for (const Buf &b : bufs_)
      if (b.out && ok()) check(hipMemcpy(b.h, b.d, b.bytes, hipMemcpyDeviceToHost));
    for (const Buf &b : bufs_) check(hipFree(b.d));
    bufs_.clear();
    return static_cast<int>(st_);
  }

 private:
  struct Buf { void *h, *d; size_t bytes; bool out; };
  void *put(void *h, size_t bytes, bool out) {
    void *d = nullptr;
    if (!ok()) return nullptr;
    if (h == nullptr || bytes == 0) { check(hipErrorInvalidValue); return nullptr; }
    check(hipMalloc(&d, bytes));
    if (!ok()) return nullptr;
    bufs_.push_back(Buf{h, d, bytes, out});
    check(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return d;
  }
  hipError_t st_ = hipSuccess;
  std::vector<Buf> bufs_;
};

inline dim3 grid_of(int n) { return dim3((n + 63) / 64); }
#define DP_CASE_INDEX const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return

__global__ void k_so3(int n, const double *phi, double *exp_q, double *Jr, double *JrInv, double *lg) {
  DP_CASE_INDEX;
  mc::so3_case(phi + 3 * i, exp_q + 4 * i, Jr + 9 * i, JrInv + 9 * i, lg + 3 * i);
}
__global__ void k_so3_small(int n, const double *phi, double *exp_q, double *Jr) {
  DP_CASE_INDEX;
  mc::so3_small_case(phi + 3 * i, exp_q + 4 * i, Jr + 9 * i);
}
__global__ void k_so3_log(int n, const double *q, double *lg) {
  DP_CASE_INDEX;
  mc::so3_log_case(q + 4 * i, lg + 3 * i);
}
__global__ void k_qmul(int n, const double *a, const double *b, double *prod, double *prod_unit) {
  DP_CASE_INDEX;
  mc::qmul_case(a + 4 * i, b + 4 * i, prod + 4 * i, prod_unit + 4 * i);
}
__global__ void k_basis(int n, const double *u, const double *idt, double *c) {
  DP_CASE_INDEX;
  mc::basis_case(u[i], idt[i], c + 24 * i);
}
__global__ void k_imu_eval(int n, const double *q, const double *p, const double *u, const double *idt, const double *g, const double *bias,
                           const double *gyro, const double *acc, const double *w, double *r, double *J) {
  DP_CASE_INDEX;
  mc::imu_eval_case(q + 16 * i, p + 12 * i, u[i], idt[i], g + 3 * i, bias + 6 * i, gyro + 3 * i, acc + 3 * i, w + 6 * i, r + 6 * i, J + 180 * i);
}
// sc: 8 per case = (ui, uj, idt, img_w, cauchy_a, rowi, rowj, d_inv)
template <bool SMALL>
__global__ void k_visual_eval(int n, const double *qi, const double *pi, const double *qj, const double *pj, const double *sc, const double *q_CI,
                              const double *p_CI, const double *obs, double *r, double *J, double *cost) {
  DP_CASE_INDEX;
  const double *s = sc + 8 * i;
  cost[i] = mc::visual_eval_case<SMALL>(qi + 16 * i, pi + 12 * i, qj + 16 * i, pj + 12 * i, s[0], s[1], s[2], q_CI + 4 * i, p_CI + 3 * i, s[3], s[4],
                                        obs + 4 * i, s[5], s[6], s[7], r + 2 * i, J + 100 * i);
}
__global__ void k_pose_jac(int n, const double *q, const double *u, int ext, const double *q_SI, const double *p_SI, double *jt) {
  DP_CASE_INDEX;
  mc::pose_jac_case(q + 16 * i, u[i], ext, q_SI + 4 * i, p_SI + 3 * i, jt + 144 * i);
}
__global__ void k_nav_jac(int n, const double *q, const double *u, const double *idt, double *jt, double *cv) {
  DP_CASE_INDEX;
  mc::nav_jac_case(q + 16 * i, u[i], idt[i], jt + 144 * i, cv + 4 * i);
}
__global__ void k_rates_jac(int n, const double *q, const double *p, const double *u, const double *idt, const double *g, double *jt) {
  DP_CASE_INDEX;
  mc::rates_jac_case(q + 16 * i, p + 12 * i, u[i], idt[i], g + 3 * i, jt + 216 * i);
}
__global__ void k_rel_pose_jac(int n, const double *qa, const double *pa, const double *ua, const double *qb, const double *pb, const double *ub, int ext,
                               const double *q_SI, const double *p_SI, double *jt_a, double *jt_b, double *rel7) {
  DP_CASE_INDEX;
  mc::rel_pose_jac_case(qa + 16 * i, pa + 12 * i, ua[i], qb + 16 * i, pb + 12 * i, ub[i], ext, q_SI + 4 * i, p_SI + 3 * i, jt_a + 144 * i, jt_b + 144 * i,
                        rel7 + 7 * i);
}
__global__ void k_proj_jac(int n, const double *qa, const double *pa, const double *ua, const double *qq, const double *pq, const double *uq,
                           const double *idt, const double *q_CI, const double *p_CI, const double *obs3, const double *rows, double *jt_a, double *jt_q,
                           double *out7) {
  DP_CASE_INDEX;
  mc::proj_jac_case(qa + 16 * i, pa + 12 * i, ua[i], qq + 16 * i, pq + 12 * i, uq[i], idt[i], q_CI + 4 * i, p_CI + 3 * i, obs3 + 3 * i, rows + 2 * i,
                    jt_a + 48 * i, jt_q + 48 * i, out7 + 7 * i);
}
__global__ void k_pred_jac(int n, const double *q_e, const double *p_e, const double *v_e, const double *w_e, const double *delta, const double *X,
                           const double *q_CI, const double *p_CI, double *pose7, double *proj3, double *B, double *C, double *A) {
  DP_CASE_INDEX;
  mc::pred_jac_case(q_e + 4 * i, p_e + 3 * i, v_e + 3 * i, w_e + 3 * i, delta[i], X + 3 * i, q_CI + 4 * i, p_CI + 3 * i, pose7 + 7 * i, proj3 + 3 * i,
                    B + 90 * i, C + 36 * i, A + 30 * i);
}
__global__ void k_imu_step(int n, double *x, const double *meas, const double *g, const double *dt, double *blocks) {
  DP_CASE_INDEX;
  mc::imu_step_case(x + 16 * i, meas + 12 * i, g + 3 * i, dt[i], blocks ? blocks + 63 * i : nullptr);
}
__global__ void k_ls_minimize(int n, int ns, const double *x, const double *v, const double *g, const double *lo, const double *hi, double *step,
                              double *coef) {
  DP_CASE_INDEX;
  step[i] = mc::ls_minimize_case(ns, x + ns * i, v + ns * i, g + ns * i, lo[i], hi[i], coef + 6 * i);
}
__global__ void k_ls_roots(int n, int np, const double *p, double *re, double *count) {
  DP_CASE_INDEX;
  count[i] = mc::ls_roots_case(np, p + np * i, re + 4 * i);
}

}  // namespace

// launch only when every allocation and copy before it succeeded (a null device pointer is never handed to a kernel)
#define DP_LAUNCH(s, kernel, n, ...) do { if ((s).ok()) hipLaunchKernelGGL(kernel, grid_of(n), dim3(64), 0, 0, n, __VA_ARGS__); } while (0)

extern "C" {
int dp_so3(int n, const double *phi, double *exp_q, double *Jr, double *JrInv, double *lg) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(phi, 3 * N); auto o0 = s.out(exp_q, 4 * N); auto o1 = s.out(Jr, 9 * N); auto o2 = s.out(JrInv, 9 * N); auto o3 = s.out(lg, 3 * N);
  DP_LAUNCH(s, k_so3, n, a0, o0, o1, o2, o3);
  return s.finish();
}
int dp_so3_small(int n, const double *phi, double *exp_q, double *Jr) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(phi, 3 * N); auto o0 = s.out(exp_q, 4 * N); auto o1 = s.out(Jr, 9 * N);
  DP_LAUNCH(s, k_so3_small, n, a0, o0, o1);
  return s.finish();
}
int dp_so3_log(int n, const double *q, double *lg) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(q, 4 * N); auto o0 = s.out(lg, 3 * N);
  DP_LAUNCH(s, k_so3_log, n, a0, o0);
  return s.finish();
}
int dp_qmul(int n, const double *a, const double *b, double *prod, double *prod_unit) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(a, 4 * N); auto a1 = s.in(b, 4 * N); auto o0 = s.out(prod, 4 * N); auto o1 = s.out(prod_unit, 4 * N);
  DP_LAUNCH(s, k_qmul, n, a0, a1, o0, o1);
  return s.finish();
}
int dp_basis(int n, const double *u, const double *idt, double *c) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(u, N); auto a1 = s.in(idt, N); auto o0 = s.out(c, 24 * N);
  DP_LAUNCH(s, k_basis, n, a0, a1, o0);
  return s.finish();
}
int dp_imu_eval(int n, const double *q, const double *p, const double *u, const double *idt, const double *g, const double *bias, const double *gyro,
                const double *acc, const double *w, double *r, double *J) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(q, 16 * N); auto a1 = s.in(p, 12 * N); auto a2 = s.in(u, N); auto a3 = s.in(idt, N); auto a4 = s.in(g, 3 * N);
  auto a5 = s.in(bias, 6 * N); auto a6 = s.in(gyro, 3 * N); auto a7 = s.in(acc, 3 * N); auto a8 = s.in(w, 6 * N);
  auto o0 = s.out(r, 6 * N); auto o1 = s.out(J, 180 * N);
  DP_LAUNCH(s, k_imu_eval, n, a0, a1, a2, a3, a4, a5, a6, a7, a8, o0, o1);
  return s.finish();
}
int dp_visual_eval(int n, int small_angle, const double *qi, const double *pi, const double *qj, const double *pj, const double *sc, const double *q_CI,
                   const double *p_CI, const double *obs, double *r, double *J, double *cost) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(qi, 16 * N); auto a1 = s.in(pi, 12 * N); auto a2 = s.in(qj, 16 * N); auto a3 = s.in(pj, 12 * N); auto a4 = s.in(sc, 8 * N);
  auto a5 = s.in(q_CI, 4 * N); auto a6 = s.in(p_CI, 3 * N); auto a7 = s.in(obs, 4 * N);
  auto o0 = s.out(r, 2 * N); auto o1 = s.out(J, 100 * N); auto o2 = s.out(cost, N);
  if (small_angle) DP_LAUNCH(s, k_visual_eval<true>, n, a0, a1, a2, a3, a4, a5, a6, a7, o0, o1, o2);
  else DP_LAUNCH(s, k_visual_eval<false>, n, a0, a1, a2, a3, a4, a5, a6, a7, o0, o1, o2);
  return s.finish();
}
int dp_pose_jac(int n, const double *q, const double *u, int ext, const double *q_SI, const double *p_SI, double *jt) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(q, 16 * N); auto a1 = s.in(u, N); auto a2 = s.in(q_SI, 4 * N); auto a3 = s.in(p_SI, 3 * N); auto o0 = s.out(jt, 144 * N);
  DP_LAUNCH(s, k_pose_jac, n, a0, a1, ext, a2, a3, o0);
  return s.finish();
}
int dp_nav_jac(int n, const double *q, const double *u, const double *idt, double *jt, double *cv) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(q, 16 * N); auto a1 = s.in(u, N); auto a2 = s.in(idt, N); auto o0 = s.out(jt, 144 * N); auto o1 = s.out(cv, 4 * N);
  DP_LAUNCH(s, k_nav_jac, n, a0, a1, a2, o0, o1);
  return s.finish();
}
int dp_rates_jac(int n, const double *q, const double *p, const double *u, const double *idt, const double *g, double *jt) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(q, 16 * N); auto a1 = s.in(p, 12 * N); auto a2 = s.in(u, N); auto a3 = s.in(idt, N); auto a4 = s.in(g, 3 * N);
  auto o0 = s.out(jt, 216 * N);
  DP_LAUNCH(s, k_rates_jac, n, a0, a1, a2, a3, a4, o0);
  return s.finish();
}
int dp_rel_pose_jac(int n, const double *qa, const double *pa, const double *ua, const double *qb, const double *pb, const double *ub, int ext,
                    const double *q_SI, const double *p_SI, double *jt_a, double *jt_b, double *rel7) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(qa, 16 * N); auto a1 = s.in(pa, 12 * N); auto a2 = s.in(ua, N); auto a3 = s.in(qb, 16 * N); auto a4 = s.in(pb, 12 * N);
  auto a5 = s.in(ub, N); auto a6 = s.in(q_SI, 4 * N); auto a7 = s.in(p_SI, 3 * N);
  auto o0 = s.out(jt_a, 144 * N); auto o1 = s.out(jt_b, 144 * N); auto o2 = s.out(rel7, 7 * N);
  DP_LAUNCH(s, k_rel_pose_jac, n, a0, a1, a2, a3, a4, a5, ext, a6, a7, o0, o1, o2);
  return s.finish();
}
int dp_proj_jac(int n, const double *qa, const double *pa, const double *ua, const double *qq, const double *pq, const double *uq, const double *idt,
                const double *q_CI, const double *p_CI, const double *obs3, const double *rows, double *jt_a, double *jt_q, double *out7) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(qa, 16 * N); auto a1 = s.in(pa, 12 * N); auto a2 = s.in(ua, N); auto a3 = s.in(qq, 16 * N); auto a4 = s.in(pq, 12 * N);
  auto a5 = s.in(uq, N); auto a6 = s.in(idt, N); auto a7 = s.in(q_CI, 4 * N); auto a8 = s.in(p_CI, 3 * N); auto a9 = s.in(obs3, 3 * N);
  auto a10 = s.in(rows, 2 * N);
  auto o0 = s.out(jt_a, 48 * N); auto o1 = s.out(jt_q, 48 * N); auto o2 = s.out(out7, 7 * N);
  DP_LAUNCH(s, k_proj_jac, n, a0, a1, a2, a3, a4, a5, a6, a7, a8, a9, a10, o0, o1, o2);
  return s.finish();
}
int dp_pred_jac(int n, const double *q_e, const double *p_e, const double *v_e, const double *w_e, const double *delta, const double *X,
                const double *q_CI, const double *p_CI, double *pose7, double *proj3, double *B, double *C, double *A) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto a0 = s.in(q_e, 4 * N); auto a1 = s.in(p_e, 3 * N); auto a2 = s.in(v_e, 3 * N); auto a3 = s.in(w_e, 3 * N); auto a4 = s.in(delta, N);
  auto a5 = s.in(X, 3 * N); auto a6 = s.in(q_CI, 4 * N); auto a7 = s.in(p_CI, 3 * N);
  auto o0 = s.out(pose7, 7 * N); auto o1 = s.out(proj3, 3 * N); auto o2 = s.out(B, 90 * N); auto o3 = s.out(C, 36 * N); auto o4 = s.out(A, 30 * N);
  DP_LAUNCH(s, k_pred_jac, n, a0, a1, a2, a3, a4, a5, a6, a7, o0, o1, o2, o3, o4);
  return s.finish();
}
// blocks null: the mean alone
int dp_imu_step(int n, double *x, const double *meas, const double *g, const double *dt, double *blocks) {
  if (n <= 0) return 0;
  Stage s; const size_t N = n;
  auto o0 = s.out(x, 16 * N); auto a0 = s.in(meas, 12 * N); auto a1 = s.in(g, 3 * N); auto a2 = s.in(dt, N);
  double *o1 = blocks ? s.out(blocks, 63 * N) : nullptr;
  DP_LAUNCH(s, k_imu_step, n, o0, a0, a1, a2, o1);
  return s.finish();
}
// x, v, g: ns per case; coef: 6 per case
int dp_ls_minimize(int n, int ns, const double *x, const double *v, const double *g, const double *lo, const double *hi, double *step, double *coef) {
  if (n <= 0) return 0;
  if (ns < 1 || ns > 3) return static_cast<int>(hipErrorInvalidValue);
  Stage s; const size_t N = n;
  auto a0 = s.in(x, ns * N); auto a1 = s.in(v, ns * N); auto a2 = s.in(g, ns * N); auto a3 = s.in(lo, N); auto a4 = s.in(hi, N);
  auto o0 = s.out(step, N); auto o1 = s.out(coef, 6 * N);
  DP_LAUNCH(s, k_ls_minimize, n, ns, a0, a1, a2, a3, a4, o0, o1);
  return s.finish();
}
// p: 1 <= np <= 5 coefficients per case; re: 4 per case; count: the number of roots, as a double
int dp_ls_roots(int n, int np, const double *p, double *re, double *count) {
  if (n <= 0) return 0;
  if (np < 1 || np > 5) return static_cast<int>(hipErrorInvalidValue);
  Stage s; const size_t N = n;
  auto a0 = s.in(p, np * N); auto o0 = s.out(re, 4 * N); auto o1 = s.out(count, N);
  DP_LAUNCH(s, k_ls_roots, n, np, a0, o0, o1);
  return s.finish();
}
}
