// jacobi_core.hpp -- what the two device eigen-solvers of the prior construction share, each stated once so that they cannot drift
// apart: the parallel cyclic Jacobi in LDS (marg_device.hpp) and the 64 x 64 sweeps of the block two-sided Jacobi (marg_blocked.hpp,
// mb_jacobi in ctvio.hip).  Host and device, no HIP include: tests/host_jacobi_check.cpp builds it with g++.
#pragma once
#include <cmath>

#if defined(__HIPCC__)   // (CTV_DI: as so3.hpp defines it)
#define CTV_DI __host__ __device__ __forceinline__
#else
#define CTV_DI inline
#endif

namespace ctv {

constexpr int JACOBI_TRACE = 26;   // off / diagonal mass of the first sweeps kept per eigen-problem (diagnostics)

// packed lower triangle with diagonal: entry (i, j) or (j, i) of a symmetric matrix
CTV_DI int pk_idx(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// e = i (i + 1) / 2 + j, j <= i: a float guess of the row, made exact by the two loops.  (The local row, like the index arguments further
// down, keeps the instruction streams the kernels had before they shared these functions.)
CTV_DI void tri_decode(int e, int &ri, int &j) {
  int i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  while (i * (i + 1) / 2 > e) --i;
  j = e - i * (i + 1) / 2;
  ri = i;
}

// strict lower triangle: e = i (i - 1) / 2 + j, j < i
CTV_DI void tri_decode_strict(int e, int &ri, int &j) {
  int i = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)e)) * 0.5f);
  while (i * (i - 1) / 2 > e) --i;
  while ((i + 1) * i / 2 <= e) ++i;
  j = e - i * (i - 1) / 2;
  ri = i;
}

// round-robin tournament over np players (np even), step s in [0, np-1), pair i in [0, np/2): (p < q)
CTV_DI void rr_pair(int np, int s, int i, int &p, int &q) {
  const int r = np - 1;
  int a, b;
  if (i == 0) { a = r; b = s; }
  else { a = (s + i) % r; b = (s + r - i) % r; }
  p = a < b ? a : b; q = a < b ? b : a;
}

// the rotation that annihilates entry (q, p) of the packed matrix Apk (the smaller root of t^2 + 2 theta t - 1); the identity if it is
// zero already, and then the diagonal is not read
CTV_DI void jacobi_cs(const double *Apk, int p, int q, double &c, double &s) {
  c = 1.0; s = 0.0;
  const double apq = Apk[pk_idx(q, p)];
  if (apq != 0.0) {
    const double app = Apk[pk_idx(p, p)], aqq = Apk[pk_idx(q, q)];
    const double theta = (aqq - app) / (2.0 * apq);
    const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(tt * tt + 1.0); s = tt * c;
  }
}

// One tournament step on the packed matrix Apk, one call per 2 x 2 block (pair I, pair J): pair I = (p1, q1) rotates by (c1, s1).
// The diagonal block (I == J):
CTV_DI void jacobi_diag_update(double *Apk, int p1, int q1, double c1, double s1) {
  const double app = Apk[pk_idx(p1, p1)], aqq = Apk[pk_idx(q1, q1)], apq = Apk[pk_idx(q1, p1)];
  Apk[pk_idx(p1, p1)] = c1 * c1 * app - 2.0 * c1 * s1 * apq + s1 * s1 * aqq;
  Apk[pk_idx(q1, q1)] = s1 * s1 * app + 2.0 * c1 * s1 * apq + c1 * c1 * aqq;
  Apk[pk_idx(q1, p1)] = 0.0;
}

// The off-diagonal block (I != J).  kGuardDummy: the dimension nd may be odd, and the dummy player q = nd has no row / column.
template <bool kGuardDummy>
CTV_DI void jacobi_block_update(double *Apk, int nd, int p1, int q1, int p2, int q2, double c1, double s1, double c2, double s2) {
  const bool vq1 = !kGuardDummy || q1 < nd, vq2 = !kGuardDummy || q2 < nd;
  const double a_pp = Apk[pk_idx(p1, p2)], a_pq = vq2 ? Apk[pk_idx(p1, q2)] : 0.0;
  const double a_qp = vq1 ? Apk[pk_idx(q1, p2)] : 0.0, a_qq = (vq1 && vq2) ? Apk[pk_idx(q1, q2)] : 0.0;
  const double t_pp = c2 * a_pp - s2 * a_pq, t_pq = s2 * a_pp + c2 * a_pq;   // columns (pair J)
  const double t_qp = c2 * a_qp - s2 * a_qq, t_qq = s2 * a_qp + c2 * a_qq;
  Apk[pk_idx(p1, p2)] = c1 * t_pp - s1 * t_qp;                                // rows (pair I)
  if (vq2) Apk[pk_idx(p1, q2)] = c1 * t_pq - s1 * t_qq;
  if (vq1) Apk[pk_idx(q1, p2)] = s1 * t_pp + c1 * t_qp;
  if (vq1 && vq2) Apk[pk_idx(q1, q2)] = s1 * t_pq + c1 * t_qq;
}

// columns p, q of one row of a row-major matrix M times the rotation (eigenvector slab, Q <- Q R): ip, iq = row * ld + p, row * ld + q
CTV_DI void rotate_cols(double *M, int ip, int iq, double c, double s) {
  const double vp = M[ip], vq = M[iq];
  M[ip] = c * vp - s * vq;
  M[iq] = s * vp + c * vq;
}

// off, d2: off-diagonal (one triangle) and diagonal sums of squares before sweep `sweep`; prev_off: off before the previous sweep.
// converged: the oracle's test (one full sweep beyond ~1e-29 is what resolves the noise-level eigenvalues of a rank-deficient
// A', which decide what falls under eps); stagnation just above it after many sweeps is accepted as the rounding floor
// (the floor of the off-diagonal mass is ~ n^2 eps^2 d2: at n = 180 that is 1.6e-27 d2, above a fixed 1e-28)
CTV_DI bool jacobi_converged(double off, double d2, int nd, int sweep, double prev_off) {
  const double floor_rel = fmax(1e-28, 4.0 * (double)nd * (double)nd * 4.93e-32);
  return off <= 1e-60 || off <= 1e-32 * d2 || (sweep >= 12 && off <= floor_rel * d2 && off > 0.25 * prev_off);
}

}  // namespace ctv
