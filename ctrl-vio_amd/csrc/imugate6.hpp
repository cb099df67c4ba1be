// imugate6.hpp -- the 6 x 6 step of ctvio_imu_gate_batch's epilogue (kernels_cov.hpp: cov_imugate_epilogue), one sample, one thread.
// Given the 21 unique entries of A = J Sigma J^T (0 <= A <= I: the sample's own J^T J is part of H) and the whitened residual r, with
// M = I - A:
//   chi2       = r^T M^-1 r = |L^-1 r|^2, M = L L^T,
//   cov36      = M^-1 - I = L^-T L^-1 - I   (optional; row-major, mirrored from the lower triangle: symmetric to the bit),
//   redundancy = lambda_min(M), cyclic Jacobi on a copy of M.
// Everything that is indexed at run time lives in `work` (IMUGATE6_WORK doubles: LDS on the device, so nothing goes to scratch memory);
// the entries of M are at most 1 in magnitude.  Built for the device with the rest of the kernels and for the host by
// tests/host_imugate_check.cpp (the __HIPCC__ shim of so3.hpp).
//
// The Jacobi sweeps: the pairs (p, q), p < q, row by row; a pair is skipped where |M_pq| <= 2^-54 (|M_pp| + |M_qq|) -- by Weyl's bound
// the fifteen entries left behind move an eigenvalue by less than 15 * 2^-53 --; the sweeps end with the first one that rotates nothing,
// after IMUGATE6_SWEEPS at the latest (6 x 6: the off-diagonal norm falls quadratically from the third sweep on; five are typical).  The
// order is fixed and nothing depends on another thread: the bits depend on (A, r) alone.  A = 0 gives chi2 = |r|^2 (summed in index
// order), a zero cov36 and redundancy 1 exactly.  Where M is not positive definite (redundancy <= 0: the caller reports status 4) chi2 and
// cov36 are NaN or meaningless and the redundancy is still the smallest eigenvalue.
#pragma once
#include "so3.hpp"

namespace ctv {

constexpr int IMUGATE6_WORK = 114;   // M (36) | L (36) | L^-1 (36) | z (6)
constexpr int IMUGATE6_SWEEPS = 12;

CTV_DI void imugate6(const double *a21, const double *r, bool want_cov, double *work, double &redundancy, double &chi2, double *cov36) {
  double *M = work, *L = work + 36, *Li = work + 72, *z = work + 108;
#pragma unroll 1
  for (int i = 0; i < 6; ++i)
#pragma unroll 1
    for (int j = 0; j <= i; ++j) {
      const double v = (i == j ? 1.0 : 0.0) - a21[i * (i + 1) / 2 + j];
      M[6 * i + j] = v;
      M[6 * j + i] = v;
    }
  // ---- M = L L^T column by column, z = L^-1 r on the way
  double chi = 0.0;
#pragma unroll 1
  for (int j = 0; j < 6; ++j) {
    double dj = M[7 * j], ej = r[j];
#pragma unroll 1
    for (int k = 0; k < j; ++k) { dj -= L[6 * j + k] * L[6 * j + k]; ej -= L[6 * j + k] * z[k]; }
    const double ljj = sqrt(dj);
    L[7 * j] = ljj;
#pragma unroll 1
    for (int i = j + 1; i < 6; ++i) {
      double v = M[6 * i + j];
#pragma unroll 1
      for (int k = 0; k < j; ++k) v -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = v / ljj;
    }
    const double zj = ej / ljj;
    z[j] = zj;
    chi += zj * zj;
  }
  chi2 = chi;
  if (want_cov) {
    // ---- L^-1 (lower) column by column, then M^-1 - I = L^-T L^-1 - I
#pragma unroll 1
    for (int j = 0; j < 6; ++j) {
      Li[7 * j] = 1.0 / L[7 * j];
#pragma unroll 1
      for (int i = j + 1; i < 6; ++i) {
        double s = 0.0;
#pragma unroll 1
        for (int k = j; k < i; ++k) s -= L[6 * i + k] * Li[6 * k + j];
        Li[6 * i + j] = s / L[7 * i];
      }
    }
#pragma unroll 1
    for (int a = 0; a < 6; ++a)
#pragma unroll 1
      for (int b = 0; b <= a; ++b) {
        double s = 0.0;
#pragma unroll 1
        for (int k = a; k < 6; ++k) s += Li[6 * k + a] * Li[6 * k + b];
        if (a == b) s -= 1.0;
        cov36[6 * a + b] = s;
        cov36[6 * b + a] = s;
      }
  }
  // ---- lambda_min(M): cyclic Jacobi, both triangles kept
#pragma unroll 1
  for (int sweep = 0; sweep < IMUGATE6_SWEEPS; ++sweep) {
    bool rotated = false;
#pragma unroll 1
    for (int p = 0; p < 5; ++p)
#pragma unroll 1
      for (int q = p + 1; q < 6; ++q) {
        const double apq = M[6 * p + q], app = M[7 * p], aqq = M[7 * q];
        if (!(fabs(apq) > 5.5511151231257827e-17 * (fabs(app) + fabs(aqq)))) continue;   // 2^-54
        rotated = true;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        M[7 * p] = app - t * apq;
        M[7 * q] = aqq + t * apq;
        M[6 * p + q] = 0.0;
        M[6 * q + p] = 0.0;
#pragma unroll 1
        for (int k = 0; k < 6; ++k) {
          if (k == p || k == q) continue;
          const double akp = M[6 * k + p], akq = M[6 * k + q];
          const double np = c * akp - s * akq, nq = s * akp + c * akq;
          M[6 * k + p] = np; M[6 * p + k] = np;
          M[6 * k + q] = nq; M[6 * q + k] = nq;
        }
      }
    if (!rotated) break;
  }
  double lo = M[0];
#pragma unroll 1
  for (int i = 1; i < 6; ++i) lo = fmin(lo, M[7 * i]);
  redundancy = lo;
}

}  // namespace ctv
