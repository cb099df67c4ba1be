// host_imufactored_check.cpp -- TEST-ONLY g++ build of the staged IMU functions of ctrl-vio_amd/csrc/factors.hpp (the fast body of
// k_imu_linearize_f64): compact rows in pair-log coordinates, accelerometer rows rotated into the world frame, the group transform T^T G^ T
// and the lamA-weighted sums for the position columns, put together into the 32 x 32 group tile the way the kernel's combine stage does,
// and compared with the tile accumulated directly from imu_eval_core's Jacobian.  Never loaded by the product.
// Built with -DIMUFACTORED_MAIN (and -fsanitize=address,undefined) it is a stand-alone program that runs its own cases.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../ctrl-vio_amd/csrc/factors.hpp"

using namespace ctv;

namespace {

struct Rng {   // splitmix64: the cases do not depend on a library's generator
  uint64_t s;
  double uni() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
  }
  double sym(double a) { return a * (2.0 * uni() - 1.0); }
};

struct ColSink {
  double J[6][32];
  void put_col(int col, const double v[6]) {
    for (int a = 0; a < 6; ++a) J[a][col] = v[a];
  }
};

// local column of index t of a 16-wide compact tile [rot 12 | bias 3 | r]: bias_at = 24 (gyro) or 27 (accelerometer)
int tile_col(int t, int bias_at) { return t < 12 ? t : (t < 15 ? bias_at + t - 12 : 30); }

void congruence(const double *G, const double *T, double *H) {   // H = T^T G T, 16 x 16 row major
  double Z[256];
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 16; ++j) {
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += G[16 * i + k] * T[16 * k + j];
      Z[16 * i + j] = s;
    }
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 16; ++j) {
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += T[16 * k + i] * Z[16 * k + j];
      H[16 * i + j] = s;
    }
}

}  // namespace

extern "C" {
// One random group of n samples whose knot-pair logs have length max_log * (0.5 .. 1): both tiles (row-major 32 x 32, local column order
// [rot 12 | pos 12 | bg 3 | ba 3 | r | -]) and the worst |new - ref| / sqrt(H_ii H_jj) over the entries whose diagonal scale is non-zero.
double hm_imufactored_case(uint64_t seed, int n, double max_log, double *tile_new, double *tile_ref) {
  Rng rng{seed};
  Knots4 k;
  SegConstS sc;
  {
    const V3 a0 = mk(rng.sym(2.0), rng.sym(2.0), rng.sym(2.0));
    k.q[0] = so3_exp(a0);
    for (int i = 0; i < 3; ++i) {
      V3 d = mk(rng.sym(1.0), rng.sym(1.0), rng.sym(1.0));
      const double len = std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z) + 1e-300, want = max_log * (0.5 + 0.5 * rng.uni());
      d = (want / len) * d;
      k.q[i + 1] = qmul(k.q[i], so3_exp(d));
    }
    k.p[0] = mk(0, 0, 0);
    for (int i = 1; i < 4; ++i) k.p[i] = k.p[i - 1] + mk(rng.sym(0.1), rng.sym(0.1), rng.sym(0.1));
    SegConst s0;
    seg_const(k, s0, true);
    for (int i = 0; i < 3; ++i) { sc.d[i] = s0.d[i]; sc.JrI[i] = s0.JrI[i]; }
  }
  const double idt = 20.0;
  const V3 grav = mk(rng.sym(0.5), rng.sym(0.5), 9.81);
  double bias[6], w[6];
  for (int i = 0; i < 3; ++i) { bias[i] = rng.sym(0.01); bias[3 + i] = rng.sym(0.1); }
  for (int i = 0; i < 3; ++i) w[i] = 50.0 + 100.0 * rng.uni();   // gyro weights may differ per axis
  w[3] = w[4] = w[5] = 5.0 + 20.0 * rng.uni();                   // isotropic accelerometer weights (imu_fast_pred)
  double gc[36];
  {
    const M3 R0 = q2R(k.q[0]);
    for (int i = 0; i < 4; ++i) { gc[3 * i] = k.p[i].x; gc[3 * i + 1] = k.p[i].y; gc[3 * i + 2] = k.p[i].z; }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) gc[12 + 3 * i + j] = R0.m[3 * j + i];
    gc[21] = grav.x; gc[22] = grav.y; gc[23] = grav.z;
    for (int i = 0; i < 6; ++i) { gc[24 + i] = bias[i]; gc[30 + i] = w[i]; }
  }
  std::vector<double> Gg(256, 0.0), G00(256, 0.0), X(12 * 16, 0.0), ref(1024, 0.0);
  double spp[4][4] = {};
  for (int s = 0; s < n; ++s) {
    const double u = rng.uni();
    double gy[3], ac[3], r[6];
    for (int i = 0; i < 3; ++i) { gy[i] = rng.sym(1.0); ac[i] = rng.sym(3.0) + (i == 2 ? 9.81 : 0.0); }
    // ---- reference: the general form's Jacobian, accumulated entry by entry
    {
      ColSink sink = {};
      ImuJac J;
      imu_eval_core(k, sc, u, idt, grav, bias, gy, ac, w, m3_id(), r, true, J);
      imu_emit_cols(J, w, sink);
      for (int a = 0; a < 6; ++a) {
        sink.J[a][30] = r[a];
        for (int i = 0; i < 31; ++i)
          for (int j = 0; j < 31; ++j) ref[32 * i + j] += sink.J[a][i] * sink.J[a][j];
      }
    }
    // ---- staged form
    ImuMid3 md;
    imu_eval_values3(gc, sc, u, idt, gy, ac, w, r, md);
    M3 M[3];
    imu_pair_gyro3(md, M);
    for (int a = 0; a < 3; ++a) {
      double row[16];
      imu_row_gyro_pl(M, w, r, a, row);
      for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) Gg[16 * i + j] += row[i] * row[j];
    }
    double Y[3][16];
    imu_world_accel3(md, gc, w, r, Y);
    for (int b = 0; b < 3; ++b) {
      for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) G00[16 * i + j] += Y[b][i] * Y[b][j];
      for (int kk = 0; kk < 4; ++kk)
        for (int c = 0; c < 16; ++c) X[(3 * kk + b) * 16 + c] += w[3] * md.lamA[kk] * Y[b][c];
    }
    for (int ka = 0; ka < 4; ++ka)
      for (int kb = 0; kb < 4; ++kb) spp[ka][kb] += (w[3] * md.lamA[ka]) * (w[3] * md.lamA[kb]);
  }
  // ---- the group's transform and the tile
  double T[256], Hg[256], Ha[256];
  imu_pairlog_T(sc, T);
  congruence(Gg.data(), T, Hg);
  congruence(G00.data(), T, Ha);
  for (int e = 0; e < 1024; ++e) tile_new[e] = 0.0;
  for (int t = 0; t < 16; ++t)
    for (int c = 0; c <= t; ++c) {   // (T^T (G^ T) is symmetric up to rounding: the lower triangle goes to both sides, as in the kernel)
      for (int side = 0; side < (t == c ? 1 : 2); ++side) {
        const int i = side ? c : t, j = side ? t : c;
        tile_new[32 * tile_col(i, 24) + tile_col(j, 24)] += Hg[16 * t + c];
        tile_new[32 * tile_col(i, 27) + tile_col(j, 27)] += Ha[16 * t + c];
      }
    }
  for (int t = 0; t < 12; ++t)
    for (int c = 0; c < 16; ++c) {
      double s = 0.0;
      for (int j = 0; j < 16; ++j) s += X[16 * t + j] * T[16 * j + c];
      tile_new[32 * (12 + t) + tile_col(c, 27)] = s;
      tile_new[32 * tile_col(c, 27) + 12 + t] = s;
    }
  for (int ka = 0; ka < 4; ++ka)
    for (int kb = 0; kb < 4; ++kb)
      for (int b = 0; b < 3; ++b) tile_new[32 * (12 + 3 * ka + b) + 12 + 3 * kb + b] = spp[ka][kb];
  double worst = 0.0;
  for (int i = 0; i < 31; ++i)
    for (int j = 0; j < 31; ++j) {
      const double sc2 = std::sqrt(ref[33 * i] * ref[33 * j]);
      if (tile_ref) tile_ref[32 * i + j] = ref[32 * i + j];
      if (sc2 > 0.0) worst = std::fmax(worst, std::fabs(tile_new[32 * i + j] - ref[32 * i + j]) / sc2);
      else if (tile_new[32 * i + j] != 0.0 || ref[32 * i + j] != 0.0) worst = INFINITY;
    }
  return worst;
}
}

#ifdef IMUFACTORED_MAIN
int main() {
  const int counts[] = {1, 3, 4, 5, 63, 64, 65, 100, 128, 129, 130};
  const double logs[] = {1e-9, 0.05, 0.3, 0.49};
  std::vector<double> a(1024), b(1024);
  double worst = 0.0;
  uint64_t seed = 1;
  for (int n : counts)
    for (double ml : logs) worst = std::fmax(worst, hm_imufactored_case(seed++, n, ml, a.data(), b.data()));
  std::printf("worst scaled difference %.3g\n", worst);
  return worst <= 1e-10 ? 0 : 1;
}
#endif
