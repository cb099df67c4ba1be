// cull_adaptor_demo.cpp -- TrajectoryEstimator::SolveWithCulling (include/ctvio_estimator.hpp): one upload, one round of (solve, cull at the
// 99 % point), a final solve.  Input as tests/cull_demo.cpp: a dumped window, a shift and the blocks whose observation p_j is moved by it.
// Output: the solved state (DemoWindow::write_state), `n_culled` and the culled factors in the order of the AddImageFeatureDelayAnalytic
// calls.  Built and run by the GPU test only.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include "demo_window.hpp"

int main(int argc, char **argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters shift block...\n", argv[0]); return 2; }
  const int iters = std::atoi(argv[3]);
  const double shift = std::atof(argv[4]);
  std::ifstream in(argv[1]);
  DemoWindow w = DemoWindow::read(in);
  for (int a = 5; a < argc; ++a) {
    const int v = std::atoi(argv[a]);
    if (v < 0 || v >= w.V) return 2;
    w.blocks[(size_t)v].pj[0] += shift;
    w.blocks[(size_t)v].pj[1] -= 0.5 * shift;
  }
  ctvio::TrajectoryEstimator estimator(w.traj.get(), w.options());
  w.add_factors(estimator);
  ctvio_cull_options o;
  ctvio_default_cull_options(&o);
  std::vector<int> culled;
  const ctvio::SolveSummary sm = estimator.SolveWithCulling(iters, o, 1, &culled);
  std::cout << "culled " << culled.size() << " of " << w.V << " image factors; re-solve: " << sm.BriefReport() << std::endl;
  std::ofstream out(argv[2]);
  out.precision(17);
  w.write_state(out, sm);
  out << culled.size() << "\n";
  for (int v : culled) out << v << " ";
  out << "\n";
  return 0;
}
