// kernels_tri.hpp -- Landmark depths outside the solve: k_triangulate (FeatureManager::triangulate / triangulateRS, reference
// feature_manager.cpp:226-339) and k_shift_anchor (removeBackShiftDepth, :341-381), both at the CURRENT device state, all fp64.
// Part of kernels.hpp (included from there, in order; not a stand-alone header).
#pragma once

namespace ctv {

// device twin of ctvio_triangulate_options (include/ctvio.h)
struct TriOpts {
  int32_t row_times, only_unset, apply, pad;
  double min_depth, init_depth;
};
enum { TRI_SKIPPED = 0, TRI_OK = 1, TRI_INIT = 2, TRI_NONE = 3 };   // the flags of both entries (ctvio.h)

// One-sided Jacobi of k_triangulate: a column pair is rotated while |a_p . a_q| > TRI_ORTH_TOL |a_p| |a_q|; the iteration ends with the first
// sweep that rotates no pair, or after TRI_MAX_SWEEPS sweeps.  (Python model with the same constants: tests/tri_helpers.py.)
constexpr double TRI_ORTH_TOL = 1e-15;
constexpr int TRI_MAX_SWEEPS = 30;

// Camera pose of an observation (t_rel, row): the spline pose at t_rel + row * line delay (row_times; the time exactly as the factors take
// it: vis_times) or at t_rel, times the window's camera extrinsic (Trajectory::GetSensorPose, trajectory.cpp:39-56).  The evaluation is
// k_spline_eval's.  false: the time falls outside the spline.
__device__ __forceinline__ bool tri_cam_pose(const Dev &d, const WinMeta &m, long long t_rel, int row, bool row_times, double ld, M3 &R, V3 &p) {
  int s;
  double u;
  vis_times(m, t_rel, row_times ? row : 0, row_times ? ld : 0.0, s, u);
  const bool inside = s >= 0 && u >= 0.0 && s <= m.K - 4;   // (a negative time truncates towards zero: s <= 0 and u <= 0)
  s = max(0, min(s, m.K - 4));                              // the loads stay in range either way
  const double zero3[3] = {0, 0, 0};
  Knots4 k;
  load_knots(d.quat, d.pos, m.knot0 + s, zero3, k);
  SegConst sc;
  seg_const(k, sc, false);
  double c[4];
  basis<false, 0>(u, 1.0, c);
  p = mk(0, 0, 0);
  for (int j = 0; j < 4; ++j) p = p + c[j] * k.p[j];
  Q4 q = eval_R(k.q, sc, u);
  p = p + qrot(q, mk(m.p_CI[0], m.p_CI[1], m.p_CI[2]));
  q = qmul(q, qmk(m.q_CI[0], m.q_CI[1], m.q_CI[2], m.q_CI[3]));
  R = q2R(q);
  return inside;
}

// The two rows an observation of the unit ray f = (x, y, 1) / |.| adds to A (feature_manager.cpp:249-258): with the pose relative to the
// anchor camera, R = R0^T Rk, t = R0^T (tk - t0), P = [R^T | -R^T t]: f0 P.row(2) - f2 P.row(0) and f1 P.row(2) - f2 P.row(1).
__device__ __forceinline__ void tri_rows(const M3 &R0, V3 t0, const M3 &Rk, V3 tk, double x, double y, double r0[4], double r1[4]) {
  M3 R0T, R;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R0T.m[3 * i + j] = R0.m[3 * j + i];
  const V3 t = mul(R0T, tk - t0);
  R = mul(R0T, Rk);
  double P[3][4];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) P[i][j] = R.m[3 * j + i];
    P[i][3] = -(R.m[i] * t.x + R.m[3 + i] * t.y + R.m[6 + i] * t.z);
  }
  const double n = sqrt(x * x + y * y + 1.0), f0 = x / n, f1 = y / n, f2 = 1.0 / n;
  for (int j = 0; j < 4; ++j) { r0[j] = f0 * P[2][j] - f2 * P[0][j]; r1[j] = f1 * P[2][j] - f2 * P[1][j]; }
}

// the sum of x over the wave, the same bits in every lane (a + b is commutative: both partners of every butterfly step form the same sum)
__device__ __forceinline__ double tri_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// One WAVE per landmark l_begin + (wave index) < l_begin + l_count (landmarks are numbered through the batch: lm0 + l): observation 0 is
// the landmark's anchor, observations 1..n its blocks in slot order (one landmark's slots are consecutive inside one group of 64:
// device_types.hpp, WinMeta::Vp).  Lane j < n evaluates block j's pose and keeps its two rows of A; the anchor's pose is evaluated by every
// lane alike (one evaluation for the wave) and its two rows are kept by lane 0 alone.  The right singular vector of the smallest singular
// value comes from one-sided (Hestenes) Jacobi on the four columns of A -- never A^T A: a new landmark is a low-parallax one, and the squared
// condition number would cost it half its digits.  Per column pair the three dot products are summed over the wave in a fixed butterfly;
// V (4 x 4) is replicated in every lane.  No atomics, no LDS: a call repeats its bits, and any launch geometry gives the same ones.
// depth / flag: [l_count] (either may be null); with o.apply, rho = 1 / depth is written for the flags TRI_OK and TRI_INIT.
__global__ __launch_bounds__(256) void k_triangulate(Dev d, int l_begin, int l_count, TriOpts o, double *depth, int32_t *flag) {
  const int lane = threadIdx.x & 63, li = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (li >= l_count) return;                       // (wave-uniform)
  const int l = l_begin + li, w = d.lm_win[l];
  const WinMeta &m = d.wins[w];
  const double rho = d.rho[l];
  const int first = d.lm_vfirst[l], n = d.lm_vcnt[l];
  auto finish = [&](int fl, double dep) {
    if (lane != 0) return;
    if (depth) depth[li] = dep;
    if (flag) flag[li] = fl;
    if (o.apply && (fl == TRI_OK || fl == TRI_INIT)) d.rho[l] = 1.0 / dep;
  };
  if (o.only_unset && rho > 0.0) { finish(TRI_SKIPPED, 1.0 / rho); return; }
  if (n <= 0) { finish(TRI_NONE, 1.0 / rho); return; }
  const bool row_times = o.row_times != 0;
  const double ld = d.ld[w];
  // ---- rows of A: a[0], a[1] this lane's block; a[2], a[3] the anchor (lane 0)
  const int a0 = d.v_anc[first];
  const bool mine = lane < n;
  const int e = first + (mine ? lane : 0);
  bool ok = d.v_anc[e] == a0;
  M3 R0, Rk;
  V3 t0, tk;
  ok = tri_cam_pose(d, m, d.a_t[a0], d.a_row[a0], row_times, ld, R0, t0) && ok;
  ok = tri_cam_pose(d, m, d.v_tj[e], d.v_rowj[e], row_times, ld, Rk, tk) && ok;
  if (__ballot(!ok) != 0ull) { finish(TRI_NONE, 1.0 / rho); return; }   // several anchors, or a time outside the spline (wave-uniform)
  double a[4][4];
  tri_rows(R0, t0, Rk, tk, d.v_obs[e], d.v_obs[(size_t)d.Vtot + e], a[0], a[1]);
  tri_rows(R0, t0, R0, t0, d.a_obs[a0], d.a_obs[(size_t)d.Atot + a0], a[2], a[3]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!mine) a[0][j] = a[1][j] = 0.0;
    if (lane != 0) a[2][j] = a[3][j] = 0.0;
  }
  // ---- one-sided Jacobi: columns p < q in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
  double V[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < TRI_MAX_SWEEPS; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) { al += a[r][p] * a[r][p]; be += a[r][q] * a[r][q]; ga += a[r][p] * a[r][q]; }
        al = tri_wave_sum(al); be = tri_wave_sum(be); ga = tri_wave_sum(ga);
        if (fabs(ga) > TRI_ORTH_TOL * sqrt(al * be)) {   // (wave-uniform: the sums are; false for a zero column and for NaN)
          rotated = true;
          const double zeta = (be - al) / (2.0 * ga);
          const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double ap = a[r][p], aq = a[r][q];
            a[r][p] = c * ap - s * aq; a[r][q] = s * ap + c * aq;
            const double vp = V[r][p], vq = V[r][q];
            V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
          }
        }
      }
    if (!rotated) break;
  }
  // ---- the column of the smallest norm (the first one among equals)
  double best = 0.0, v2 = 0.0, v3 = 0.0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    double al = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) al += a[r][p] * a[r][p];
    al = tri_wave_sum(al);
    if (p == 0 || al < best) { best = al; v2 = V[2][p]; v3 = V[3][p]; }
  }
  const double dep = v2 / v3;
  // (a non-finite depth takes init_depth as well: the reference's `depth < 0.1` lets NaN through)
  if (dep >= o.min_depth && isfinite(dep)) finish(TRI_OK, dep);
  else finish(TRI_INIT, o.init_depth);
}

// One lane per query: the depth of landmark lm[i] of window win[i] in the frame of a new anchor observation at (t_new[i] relative to the
// window's t0, row_new[i] or 0) -- z(R_new^T (R_old (p_i / rho) + P_old - P_new)) with camera poses (feature_manager.cpp:370-377).  The
// state is only read.
__global__ void k_shift_anchor(Dev d, int n, const int32_t *win, const int32_t *lm, const long long *t_new, const int32_t *row_new, TriOpts o,
                               double *depth_new, int32_t *flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int w = win[i];
  const WinMeta &m = d.wins[w];
  const int l = m.lm0 + lm[i], first = d.lm_vfirst[l], cnt = d.lm_vcnt[l];
  const double rho = d.rho[l];
  bool ok = rho > 0.0 && cnt > 0;
  int a0 = m.anc0;
  if (cnt > 0) {
    a0 = d.v_anc[first];
    for (int j = 1; j < cnt; ++j) ok = ok && d.v_anc[first + j] == a0;
  }
  int fl = TRI_NONE;
  double dep = qnan();
  if (ok) {
    const bool row_times = o.row_times != 0;
    const double ld = d.ld[w];
    M3 Ro, Rn;
    V3 Po, Pn;
    ok = tri_cam_pose(d, m, d.a_t[a0], d.a_row[a0], row_times, ld, Ro, Po);
    ok = tri_cam_pose(d, m, t_new[i], row_new ? row_new[i] : 0, row_times, ld, Rn, Pn) && ok;
    if (ok) {
      const double z = 1.0 / rho;
      const V3 wp = mul(Ro, mk(d.a_obs[a0] * z, d.a_obs[(size_t)d.Atot + a0] * z, z)) + Po - Pn;
      dep = Rn.m[2] * wp.x + Rn.m[5] * wp.y + Rn.m[8] * wp.z;
      fl = TRI_OK;
      if (!(dep > 0.0)) { dep = o.init_depth; fl = TRI_INIT; }
    }
  }
  if (depth_new) depth_new[i] = dep;
  if (flag) flag[i] = fl;
}

}  // namespace ctv
