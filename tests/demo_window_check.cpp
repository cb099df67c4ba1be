// demo_window_check.cpp -- tests/demo_window.hpp on the host alone (tests/test_demo_window_host.py): read a dump, hand its factors to a
// TrajectoryEstimator without solving (nothing on that path touches a device), write the state back with a default summary, then one line
// `kind index` per prior block: what its pointer resolves to among the window's own parameter blocks (kinds as in the dump: 0 knot
// rotation, 1 knot position, 2 gyro bias, 3 accelerometer bias, 4 line delay; -1 -1: none of them).
#include <cstdio>
#include <fstream>

#include "demo_window.hpp"

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s in.txt out.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  const DemoWindow w = DemoWindow::read(in);
  if (!in) { std::fprintf(stderr, "short or malformed dump\n"); return 1; }
  ctvio::TrajectoryEstimator estimator(w.traj.get(), w.options());
  w.add_factors(estimator);
  std::ofstream out(argv[2]);
  w.write_state(out, ctvio::SolveSummary());
  for (const double *p : w.marg_blocks) {
    int kind = -1, index = -1;
    for (int k = 0; k < w.K; ++k) {
      if (p == w.traj->getKnotSO3(k).data()) { kind = 0; index = k; }
      if (p == w.traj->getKnotPos(k).data()) { kind = 1; index = k; }
    }
    for (int f = 0; f < w.F; ++f) {
      if (p == w.bg[f].data()) { kind = 2; index = f; }
      if (p == w.ba[f].data()) { kind = 3; index = f; }
    }
    if (p == &w.traj->line_delay) { kind = 4; index = 0; }
    out << kind << " " << index << "\n";
  }
  return 0;
}
