// Test program (CPU): the slice planner of ctvio_visual_gate_batch (ctrl-vio_amd/csrc/host_pack.hpp: plan_gate_slices) compiled with g++
// against the HIP headers (no device code, nothing is launched).  `host_gateslice_check budget wbeg wend n0 n1 ...` prints one line
// "wbeg wend slots" per slice for the windows' slot counts n0, n1, ...; without arguments it runs its own cases -- budgets that give one
// slice, many slices, one window per slice, an oversize window, empty windows -- and checks that every window lands in exactly one slice,
// in order, and that a slice beyond the budget holds a single window with slots.  tests/test_visgate_host.py drives both uses, the second
// one also built with -fsanitize=address,undefined.
#define __HIP_PLATFORM_AMD__ 1
#include "../ctrl-vio_amd/csrc/host_pack.hpp"

#include <cstdio>
#include <cstdlib>

static int check(const std::vector<int32_t> &n, int wbeg, int wend, size_t budget, size_t want_slices) {
  const std::vector<ctv::GateSlice> s = ctv::plan_gate_slices(n.data(), wbeg, wend, budget);
  int next = wbeg;
  for (const ctv::GateSlice &x : s) {
    if (x.wbeg != next || x.wend <= x.wbeg) return 1;                 // in order, no gap, no empty slice
    int64_t sum = 0;
    int with_slots = 0;
    for (int w = x.wbeg; w < x.wend; ++w) { sum += n[(size_t)w]; with_slots += n[(size_t)w] > 0; }
    if (sum != x.slots) return 2;
    if ((size_t)sum > budget && with_slots != 1) return 3;             // beyond the budget: one oversize window (and empty ones)
    next = x.wend;
  }
  if (next != wend && !(s.empty() && wbeg == wend)) return 4;
  for (size_t i = 0; i + 1 < s.size(); ++i)                            // greedy: the next window with slots would not have fitted
    for (int w = s[i + 1].wbeg; w < s[i + 1].wend; ++w)
      if (n[(size_t)w] > 0) { if ((size_t)(s[i].slots + n[(size_t)w]) <= budget && s[i].slots > 0) return 5; break; }
  if (want_slices && s.size() != want_slices) return 6;
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 4) {
    const size_t budget = (size_t)std::atoll(argv[1]);
    const int wbeg = std::atoi(argv[2]), wend = std::atoi(argv[3]);
    std::vector<int32_t> n;
    for (int i = 4; i < argc; ++i) n.push_back(std::atoi(argv[i]));
    if (wbeg < 0 || wend < wbeg || (size_t)wend > n.size()) return 2;
    for (const ctv::GateSlice &x : ctv::plan_gate_slices(n.data(), wbeg, wend, budget)) std::printf("%d %d %lld\n", x.wbeg, x.wend, (long long)x.slots);
    return 0;
  }
  struct Case { std::vector<int32_t> n; int wbeg, wend; size_t budget, slices; };
  const Case cases[] = {
      {{64, 128, 64, 256}, 0, 4, 65536, 1},          // one slice
      {{64, 128, 64, 256}, 0, 4, 192, 3},            // many slices: 64 + 128 | 64 | 256 (oversize, alone)
      {{64, 64, 64, 64}, 0, 4, 64, 4},               // one window per slice
      {{64, 1024, 64}, 0, 3, 128, 3},                // an oversize window between two small ones
      {{0, 0, 64, 0, 64, 0}, 0, 6, 64, 2},           // empty windows ride along
      {{0, 0, 0}, 0, 3, 64, 1},                      // nothing but empty windows
      {{64, 128, 64, 256}, 1, 3, 128, 2},            // a sub-range (the single-window entry is wbeg + 1 == wend)
      {{64, 128, 64, 256}, 2, 3, 1, 1},
      {{64}, 0, 0, 64, 0},                           // no windows: no slices
  };
  int nc = 0;
  for (const Case &c : cases) {
    const int rc = check(c.n, c.wbeg, c.wend, c.budget, c.slices);
    if (rc) { std::printf("case %d: %d\n", nc, rc); return 1; }
    ++nc;
  }
  unsigned long long x = 88172645463325252ull;      // xorshift: random shapes against the invariants
  for (int it = 0; it < 2000; ++it) {
    std::vector<int32_t> n;
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    const int nw = 1 + (int)(x % 40);
    for (int w = 0; w < nw; ++w) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; n.push_back((x % 5 == 0) ? 0 : 64 * (int32_t)(1 + x % 9)); }
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    const size_t budget = 64 * (size_t)(1 + x % 24);
    const int rc = check(n, 0, nw, budget, 0);
    if (rc) { std::printf("random case %d: %d\n", it, rc); return 1; }
    ++nc;
  }
  std::printf("GATESLICE_OK %d cases\n", nc);
  return 0;
}
