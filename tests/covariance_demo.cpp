// covariance_demo.cpp -- TrajectoryEstimator::GetCovarianceInTangentSpace through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp).
// Input: a window dumped as text by tests/test_gpu_covariance.py (the layout tests/demo_window.hpp reads); the window is solved, then the
// covariance of knot `knot` (rotation, position) and of the last bias state (gyro, accel) is asked for.  Output: the solved state in the same
// text layout, then `ok n` and the n x n covariance, then the variances of the first two inverse depths.  Built and run by the GPU test only.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <vector>

#include "demo_window.hpp"

int main(int argc, char **argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters knot\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  const DemoWindow w = DemoWindow::read(in);
  ctvio::TrajectoryEstimator estimator(w.traj.get(), w.options());
  w.add_factors(estimator);
  ctvio::SolveSummary summary = estimator.Solve(std::atoi(argv[3]), false);
  std::cout << summary.BriefReport() << std::endl;

  std::ofstream out(argv[2]);
  w.write_state(out, summary);

  const int knot = std::atoi(argv[4]);
  std::vector<double> cov;
  const bool ok = estimator.GetCovarianceInTangentSpace(
      {w.traj->getKnotSO3(knot).data(), w.traj->getKnotPos(knot).data(), w.bg[w.F - 1].data(), w.ba[w.F - 1].data()}, cov);
  out << (ok ? 1 : 0) << " " << 12 << "\n";
  for (double v : cov) out << v << " ";
  out << "\n";
  std::vector<double> var;
  const bool ok2 = estimator.GetCovarianceInTangentSpace({&w.para_Feature[0], &w.para_Feature[1]}, var);
  out << (ok2 ? 1 : 0) << " " << var[0] << " " << var[3] << "\n";
  bool refused = false;   // a depth next to a trajectory block: the cross terms are not computed
  try { estimator.GetCovarianceInTangentSpace({&w.para_Feature[0], &w.traj->line_delay}, var); } catch (const std::invalid_argument &) { refused = true; }
  out << (refused ? 1 : 0) << "\n";
  return 0;
}
