// visual_gate_demo.cpp -- TrajectoryEstimator::GateVisualBlocks through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp): after
// the solve, cull outliers.  Input: a window dumped as text by tests/test_gpu_visual_gate_demo.py (the layout tests/demo_window.hpp reads), the
// index of one visual block and a shift in normalised image units.  The window is solved; then that block's observation p_j is moved by the
// shift (a few tens of pixel-equivalents: a wrong match), the window is solved again from the first solution with the same factors, and every
// block goes through the leave-one-out test.
// Output: `ok V`, the V gates chi2, the V statuses, the V x 2 residuals, then `L` and per inverse-depth pointer (in landmark order) its count,
// mean reprojection error, largest chi2 and smallest redundancy; then `ok V` and the V x 2 residuals of the values-only call.  Built and run
// by the GPU test only.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <vector>

#include "demo_window.hpp"

int main(int argc, char **argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters block shift\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  DemoWindow w = DemoWindow::read(in);
  const int iters = std::atoi(argv[3]), bad = std::atoi(argv[4]);
  const double shift = std::atof(argv[5]);
  if (bad < 0 || bad >= w.V) return 2;
  {
    ctvio::TrajectoryEstimator clean(w.traj.get(), w.options());
    w.add_factors(clean);
    std::cout << clean.Solve(iters, false).BriefReport() << std::endl;
  }
  w.blocks[(size_t)bad].pj[0] += shift;      // the wrong match
  w.blocks[(size_t)bad].pj[1] -= 0.5 * shift;
  ctvio::TrajectoryEstimator estimator(w.traj.get(), w.options());
  w.add_factors(estimator);
  std::cout << estimator.Solve(iters, false).BriefReport() << std::endl;

  ctvio::TrajectoryEstimator::VisualGate gate, values;
  std::map<const double *, ctvio::TrajectoryEstimator::LandmarkGate> lms;
  const bool ok = estimator.GateVisualBlocks(gate, &lms);
  std::ofstream out(argv[2]);
  out.precision(17);
  out << (ok ? 1 : 0) << " " << w.V << "\n";
  for (double v : gate.chi2) out << v << " ";
  out << "\n";
  for (int32_t v : gate.status) out << v << " ";
  out << "\n";
  for (double v : gate.res2) out << v << " ";
  out << "\n" << w.L << "\n";
  for (int l = 0; l < w.L; ++l) {
    const auto it = lms.find(&w.para_Feature[l]);
    if (it == lms.end()) out << "-1 0 0 0\n";
    else out << it->second.count << " " << it->second.mean_error << " " << it->second.max_chi2 << " " << it->second.min_redundancy << "\n";
  }
  const bool ok_values = estimator.GateVisualBlocks(values, nullptr, 0.01, false);
  out << (ok_values ? 1 : 0) << " " << w.V << "\n";
  for (double v : values.res2) out << v << " ";
  out << "\n";
  return 0;
}
