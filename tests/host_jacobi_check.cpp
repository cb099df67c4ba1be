// Test-only shim: exposes the index arithmetic, the rotation rule and the convergence rule that the two device eigen-solvers of the
// prior construction share (ctrl-vio_amd/csrc/jacobi_core.hpp) to ctypes, so that tests/test_jacobi_core_host.py can compare them with
// the NumPy model without a GPU.
#include "../ctrl-vio_amd/csrc/jacobi_core.hpp"
#include <cstdint>
extern "C" void jc_tri_decode(int n, int strict, int32_t *i, int32_t *j) {   // every e < n
  for (int e = 0; e < n; ++e) {
    int a, b;
    if (strict) ctv::tri_decode_strict(e, a, b); else ctv::tri_decode(e, a, b);
    i[e] = a; j[e] = b;
  }
}
extern "C" void jc_rr_pair(int np, int32_t *pq) {   // [np - 1 steps][np / 2 pairs][p, q]
  for (int s = 0; s < np - 1; ++s)
    for (int i = 0; i < np / 2; ++i) {
      int p, q;
      ctv::rr_pair(np, s, i, p, q);
      *pq++ = p; *pq++ = q;
    }
}
extern "C" void jc_cs(int n, const double *app, const double *aqq, const double *apq, double *c, double *s) {
  for (int k = 0; k < n; ++k) {
    const double Apk[3] = {app[k], apq[k], aqq[k]};   // packed lower triangle of [app apq; apq aqq]: the pivot is (p, q) = (0, 1)
    ctv::jacobi_cs(Apk, 0, 1, c[k], s[k]);
  }
}
extern "C" int jc_converged(double off, double d2, int nd, int sweep, double prev_off) { return ctv::jacobi_converged(off, d2, nd, sweep, prev_off) ? 1 : 0; }
