// Test program (CPU): the host-buildable parts of ctvio_imu_gate_batch compiled with g++ (no device code, nothing is launched) -- the
// 6 x 6 step of the epilogue (ctrl-vio_amd/csrc/imugate6.hpp, the function the device runs), the slot map and the tile / slice planning
// (ctrl-vio_amd/csrc/host_pack.hpp: imu_slot_map, plan_gate_slices, plan_imugate_tiles).
//   host_imugate_check step a21 (21) r (6) redundancy chi2 cov36 (36)
//     runs imugate6 on the lower triangle a21 of A and the residual r and compares with the expected values (NumPy's, from
//     tests/test_imugate_host.py) at the step's own rounding: redundancy absolute 64 * 2^-53; where redundancy >= 0.01, chi2 relative and
//     cov36 (Frobenius norm of the difference, relative to 1 / redundancy = |cov36 + I|_2) 64 * 2^-53 / redundancy; cov36 symmetric to the bit.
//   host_imugate_check tiles budget M0 M1 ...
//     prints "wbeg wend samples tiles" per slice and, per window, "w first_tile", then walks every tile of every slice through the
//     device's lookup (bisection over the descriptors) and checks that every packed sample is covered exactly once, by a tile of its own window.
//   host_imugate_check
//     its own cases: A = 0 (exact), repeated eigenvalues, the slot map of a shuffled window, odd M, M = 0, an oversize window.
// tests/test_imugate_host.py drives all three, the last one also built with -fsanitize=address,undefined.
#define __HIP_PLATFORM_AMD__ 1
#include "../ctrl-vio_amd/csrc/host_pack.hpp"
#include "../ctrl-vio_amd/csrc/imugate6.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static const double EPS = 1.1102230246251565e-16;   // 2^-53
static const int PER_TILE = 2;

// the device's tile lookup (kernels_cov.hpp: cov_imugate_tile) restated on the host
static void tile_of(const std::vector<int32_t> &first, int b, int &win_local, int &lt) {
  int lo = 0, hi = (int)first.size() - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[(size_t)mid] <= b) lo = mid; else hi = mid;
  }
  win_local = lo;
  lt = b - first[(size_t)lo];
}

static int check_tiles(const std::vector<int32_t> &M, size_t budget, bool print) {
  const int nw = (int)M.size();
  const std::vector<ctv::GateSlice> slices = ctv::plan_gate_slices(M.data(), 0, nw, budget);
  std::vector<std::vector<int>> seen((size_t)nw);
  for (int w = 0; w < nw; ++w) seen[(size_t)w].assign((size_t)M[(size_t)w], 0);
  int next = 0;
  for (const ctv::GateSlice &sl : slices) {
    if (sl.wbeg != next || sl.wend <= sl.wbeg) return 1;
    next = sl.wend;
    const std::vector<int32_t> first = ctv::plan_imugate_tiles(M.data(), sl.wbeg, sl.wend, PER_TILE);
    if ((int)first.size() != sl.wend - sl.wbeg + 1 || first[0] != 0) return 2;
    const int ntiles = first.back();
    if (print) {
      std::printf("%d %d %lld %d\n", sl.wbeg, sl.wend, (long long)sl.slots, ntiles);
      for (int w = sl.wbeg; w < sl.wend; ++w) std::printf("w %d %d\n", w, first[(size_t)(w - sl.wbeg)]);
    }
    int64_t samples = 0;
    for (int w = sl.wbeg; w < sl.wend; ++w) samples += M[(size_t)w];
    if (samples != sl.slots) return 3;
    for (int b = 0; b < ntiles; ++b) {
      int wl, lt;
      tile_of(first, b, wl, lt);
      const int w = sl.wbeg + wl;
      if (w < sl.wbeg || w >= sl.wend) return 4;
      const int count = std::min(PER_TILE, M[(size_t)w] - PER_TILE * lt);
      if (lt < 0 || count < 1) return 5;                                   // (never a window without samples, never past its last sample)
      for (int q = 0; q < count; ++q) seen[(size_t)w][(size_t)(PER_TILE * lt + q)]++;
    }
  }
  if (next != nw && !(slices.empty() && nw == 0)) return 6;
  for (int w = 0; w < nw; ++w)
    for (int v : seen[(size_t)w]) if (v != 1) return 7;
  return 0;
}

static int run_step(const double *a21, const double *r, double &red, double &chi2, double *cov36) {
  double work[ctv::IMUGATE6_WORK];
  ctv::imugate6(a21, r, true, work, red, chi2, cov36);
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < i; ++j) if (std::memcmp(&cov36[6 * i + j], &cov36[6 * j + i], sizeof(double)) != 0) return 1;   // (to the bit; NaN where I - A is not positive definite)
  double red2, chi2b;
  ctv::imugate6(a21, r, false, work, red2, chi2b, nullptr);               // (without the covariance: the same bits)
  return red2 == red && (chi2b == chi2 || (chi2b != chi2b && chi2 != chi2)) ? 0 : 2;
}

int main(int argc, char **argv) {
  if (argc >= 2 && std::string(argv[1]) == "step") {
    if (argc != 2 + 21 + 6 + 2 + 36) return 2;
    double a21[21], r[6], cov_ref[36], cov[36], red, chi2;
    int at = 2;
    for (double &v : a21) v = std::strtod(argv[at++], nullptr);
    for (double &v : r) v = std::strtod(argv[at++], nullptr);
    const double red_ref = std::strtod(argv[at++], nullptr), chi_ref = std::strtod(argv[at++], nullptr);
    for (double &v : cov_ref) v = std::strtod(argv[at++], nullptr);
    if (const int rc = run_step(a21, r, red, chi2, cov)) { std::printf("symmetry / repeat: %d\n", rc); return 1; }
    std::printf("redundancy %.17g (expected %.17g) chi2 %.17g (expected %.17g)\n", red, red_ref, chi2, chi_ref);
    if (!(std::fabs(red - red_ref) <= 64 * EPS)) { std::printf("redundancy off by %.3g\n", red - red_ref); return 1; }
    if (red_ref < 0.01) return 0;                                          // (status 4: chi2 and cov36 are not reported)
    const double rel = 64 * EPS / red_ref;
    if (!(std::fabs(chi2 - chi_ref) <= rel * chi_ref)) { std::printf("chi2 off by %.3g relative, margin %.3g\n", (chi2 - chi_ref) / chi_ref, rel); return 1; }
    double fro = 0.0;
    for (int e = 0; e < 36; ++e) fro += (cov[e] - cov_ref[e]) * (cov[e] - cov_ref[e]);
    fro = std::sqrt(fro);
    if (!(fro <= rel / red_ref)) { std::printf("cov36 off by %.3g, margin %.3g\n", fro, rel / red_ref); return 1; }
    std::printf("IMUGATE_STEP_OK %.3g %.3g %.3g\n", std::fabs(red - red_ref) / (64 * EPS), chi_ref > 0 ? std::fabs(chi2 - chi_ref) / (rel * chi_ref) : 0.0, fro / (rel / red_ref));
    return 0;
  }
  if (argc >= 3 && std::string(argv[1]) == "tiles") {
    const size_t budget = (size_t)std::atoll(argv[2]);
    std::vector<int32_t> M;
    for (int i = 3; i < argc; ++i) M.push_back(std::atoi(argv[i]));
    const int rc = check_tiles(M, budget, true);
    if (rc) { std::printf("tiles: %d\n", rc); return 1; }
    return 0;
  }
  int nc = 0;
  {   // A = 0: chi2 = |r|^2 summed in index order, a zero covariance, redundancy 1, all exact
    double a21[21] = {0}, r[6] = {0.3, -1.7, 2.9, 0.01, -4.0, 1.1}, cov[36], red, chi2, want = 0.0;
    for (double v : r) want += v * v;
    if (run_step(a21, r, red, chi2, cov) || red != 1.0 || chi2 != want) { std::printf("A = 0: %.17g %.17g\n", red, chi2); return 1; }
    for (double v : cov) if (v != 0.0) { std::printf("A = 0: cov36 %.17g\n", v); return 1; }
    ++nc;
  }
  for (double c : {0.25, 0.5, 0.99, 0.9999}) {   // A = c I: a six-fold eigenvalue, nothing to rotate
    double a21[21] = {0}, r[6] = {1, 2, 3, 4, 5, 6}, cov[36], red, chi2;
    for (int i = 0; i < 6; ++i) a21[i * (i + 1) / 2 + i] = c;
    if (run_step(a21, r, red, chi2, cov) || red != 1.0 - c) { std::printf("A = c I: %.17g\n", red); return 1; }
    if (!(std::fabs(chi2 - 91.0 / (1.0 - c)) <= 16 * EPS * 91.0 / (1.0 - c))) { std::printf("A = c I: chi2 %.17g\n", chi2); return 1; }
    if (!(std::fabs(cov[0] - c / (1.0 - c)) <= 16 * EPS / (1.0 - c)) || cov[1] != 0.0) { std::printf("A = c I: cov %.17g\n", cov[0]); return 1; }
    ++nc;
  }
  {   // the slot map: packed position i holds the caller's sample iorder[i]; slot[caller's sample] = imu0 + position
    const std::vector<int32_t> iorder = {4, 0, 3, 1, 2};
    std::vector<int32_t> slot(5, -1);
    ctv::imu_slot_map(iorder.data(), 5, 100, slot.data());
    for (int i = 0; i < 5; ++i) if (slot[(size_t)iorder[(size_t)i]] != 100 + i) { std::printf("slot map\n"); return 1; }
    ctv::imu_slot_map(iorder.data(), 0, 100, nullptr);   // (M = 0: nothing is written)
    ++nc;
  }
  struct Case { std::vector<int32_t> M; size_t budget; };
  const Case cases[] = {
      {{80, 500, 0}, 49152}, {{7}, 49152}, {{1}, 1}, {{0}, 64}, {{0, 0, 0}, 64}, {{5, 0, 3, 0, 0, 9}, 8}, {{64, 1001, 64}, 128},
      {{0, 3}, 64}, {{3, 0}, 64}, {{2, 2, 2, 2}, 4}, {{}, 64},
  };
  for (const Case &c : cases) {
    const int rc = check_tiles(c.M, c.budget, false);
    if (rc) { std::printf("tile case %d: %d\n", nc, rc); return 1; }
    ++nc;
  }
  unsigned long long x = 88172645463325252ull;      // xorshift: random shapes against the invariants
  for (int it = 0; it < 1000; ++it) {
    std::vector<int32_t> M;
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    const int nw = 1 + (int)(x % 20);
    for (int w = 0; w < nw; ++w) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; M.push_back((x % 4 == 0) ? 0 : (int32_t)(1 + x % 41)); }
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    const int rc = check_tiles(M, 1 + (size_t)(x % 60), false);
    if (rc) { std::printf("random tile case %d: %d\n", it, rc); return 1; }
    ++nc;
  }
  std::printf("IMUGATE_HOST_OK %d cases\n", nc);
  return 0;
}
