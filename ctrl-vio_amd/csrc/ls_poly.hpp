// ls_poly.hpp -- interpolation of the next trial step of the line search (Ceres polynomial.cc: FindInterpolatingPolynomial /
// MinimizePolynomial): the polynomial through the values and gradients of two or three samples, and its minimiser over an interval.
// Used by lm_decide (kernels_control.hpp) on one lane of k_pass_end.  A header of its own so that a plain g++ build can check it on the
// host (tests/host_lspoly_check.cpp, not a product path); under hipcc the functions keep the inlining hints they had in kernels_control.hpp.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CTV_LS_D __host__ __device__ inline
#define CTV_LS_DF __host__ __device__ __forceinline__
#else
#include <cmath>
#define CTV_LS_D inline
#define CTV_LS_DF inline
#endif

namespace ctv {

struct LsSample { double x, v, g; };
// The arrays of the interpolation, used by ONE lane of k_pass_end: kept in LDS (632 B per workgroup).  As private arrays they were thread 0's
// 384 B of scratch and 72 B x 256 threads of compiler-promoted LDS, and set the register count of a kernel whose other 255 threads only reduce and copy.
struct LsWork {
  double A[6][7], coef[6], der[5], roots[4];   // ls_minimize_interpolating
  double q[5], zr[4], zi[4];                   // ls_root_real_parts
  LsSample sp[3];                              // lm_decide
};
CTV_LS_D double ls_poly_eval(const double *p, int n, double x) {
  double v = 0;
  for (int i = 0; i < n; ++i) v = v * x + p[i];
  return v;
}
CTV_LS_D double ls_ipow(double x, int e) { double r = 1.0; for (int i = 0; i < e; ++i) r *= x; return r; }
// real parts of all (complex) roots of a polynomial of degree <= 4, coefficients highest power first
CTV_LS_DF int ls_root_real_parts(const double *p_in, int n, double *re, LsWork &ws) {
  while (n > 0 && p_in[0] == 0.0) { ++p_in; --n; }
  const int deg = n - 1;
  if (deg <= 0) return 0;
  if (deg == 1) { re[0] = -p_in[1] / p_in[0]; return 1; }
  if (deg == 2) {
    const double a = p_in[0], b = p_in[1], c = p_in[2], D = b * b - 4 * a * c, sD = sqrt(fabs(D));
    if (D >= 0) {
      if (b >= 0) { re[0] = (-b - sD) / (2.0 * a); re[1] = (2.0 * c) / (-b - sD); }
      else { re[0] = (2.0 * c) / (-b + sD); re[1] = (-b + sD) / (2.0 * a); }
    } else { re[0] = re[1] = -b / (2.0 * a); }
    return 2;
  }
  double *q = ws.q, *zr = ws.zr, *zi = ws.zi;
  for (int i = 0; i <= deg; ++i) q[i] = p_in[i] / p_in[0];
  double rad = 0;
  for (int i = 1; i <= deg; ++i) rad = fmax(rad, fabs(q[i]));
  rad = 1.0 + rad;
  // (deg is 3 or 4 here.  Unrolled: as a loop, the literals of the sine and cosine are hoisted out of it and spilled across it)
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < deg) { const double ang = 2.0 * 3.14159265358979323846 * k / deg + 0.4; zr[k] = 0.5 * rad * cos(ang); zi[k] = 0.5 * rad * sin(ang); }
  for (int it = 0; it < 500; ++it) {   // Durand-Kerner
    double change = 0;
    for (int k = 0; k < deg; ++k) {
      double pr = 1.0, pi = 0.0;
      for (int i = 1; i <= deg; ++i) { const double tr = pr * zr[k] - pi * zi[k] + q[i], ti = pr * zi[k] + pi * zr[k]; pr = tr; pi = ti; }
      double dr = 1.0, di = 0.0;
      for (int j = 0; j < deg; ++j) {
        if (j == k) continue;
        const double ar = zr[k] - zr[j], ai = zi[k] - zi[j], tr = dr * ar - di * ai, ti = dr * ai + di * ar;
        dr = tr; di = ti;
      }
      const double den = dr * dr + di * di;
      if (den == 0.0) continue;
      const double cr = (pr * dr + pi * di) / den, ci = (pi * dr - pr * di) / den;
      zr[k] -= cr; zi[k] -= ci;
      change += fabs(cr) + fabs(ci);
    }
    if (change < 1e-15 * rad) break;
  }
  for (int k = 0; k < deg; ++k) re[k] = zr[k];
  return deg;
}
CTV_LS_DF double ls_minimize_interpolating(const LsSample *s, int ns, double x_min, double x_max, LsWork &ws) {
  const int nc = 2 * ns, deg = nc - 1;
  double (*A)[7] = ws.A, *coef = ws.coef, *der = ws.der, *roots = ws.roots;
  for (int i = 0; i < ns; ++i) {
    for (int j = 0; j <= deg; ++j) A[2 * i][j] = ls_ipow(s[i].x, deg - j);
    A[2 * i][nc] = s[i].v;
    for (int j = 0; j < deg; ++j) A[2 * i + 1][j] = (deg - j) * ls_ipow(s[i].x, deg - j - 1);
    A[2 * i + 1][deg] = 0.0;
    A[2 * i + 1][nc] = s[i].g;
  }
  for (int c = 0; c < nc; ++c) {
    int piv = c;
    for (int r = c + 1; r < nc; ++r) if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
    if (A[piv][c] == 0.0) return 0.5 * (x_min + x_max);
    if (piv != c) for (int j = 0; j <= nc; ++j) { const double t = A[c][j]; A[c][j] = A[piv][j]; A[piv][j] = t; }
    for (int r = 0; r < nc; ++r) {
      if (r == c) continue;
      const double f = A[r][c] / A[c][c];
      for (int j = c; j <= nc; ++j) A[r][j] -= f * A[c][j];
    }
  }
  for (int c = 0; c < nc; ++c) coef[c] = A[c][nc] / A[c][c];
  double best_x = 0.5 * (x_min + x_max), best = ls_poly_eval(coef, nc, best_x), v;
  v = ls_poly_eval(coef, nc, x_min); if (v < best) { best = v; best_x = x_min; }
  v = ls_poly_eval(coef, nc, x_max); if (v < best) { best = v; best_x = x_max; }
  for (int i = 0; i < nc - 1; ++i) der[i] = (nc - 1 - i) * coef[i];
  const int nr = ls_root_real_parts(der, nc - 1, roots, ws);
  for (int i = 0; i < nr; ++i) {
    if (roots[i] < x_min || roots[i] > x_max) continue;
    v = ls_poly_eval(coef, nc, roots[i]);
    if (v < best) { best = v; best_x = roots[i]; }
  }
  for (int i = 0; i < ns; ++i) {
    if (s[i].x < x_min || s[i].x > x_max) continue;
    v = ls_poly_eval(coef, nc, s[i].x);
    if (v < best) { best = v; best_x = s[i].x; }
  }
  return best_x;
}

}  // namespace ctv
