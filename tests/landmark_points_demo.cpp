// landmark_points_demo.cpp -- TrajectoryEstimator::GetLandmarkPoints through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp).
// Input: a window dumped as text by tests/test_gpu_landmark_points.py (the layout tests/demo_window.hpp reads); the window is solved, then the
// world points of its landmarks are asked for with their 3 x 3 covariances, and once more as points only.
// Output: the solved state in the same text layout, then `ok L`, the L x 3 points, the L x 9 covariances and the L statuses, then `ok L` and the
// L x 3 points of the points-only call.  Built and run by the GPU test only.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <vector>

#include "demo_window.hpp"

int main(int argc, char **argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  const DemoWindow w = DemoWindow::read(in);
  ctvio::TrajectoryEstimator estimator(w.traj.get(), w.options());
  w.add_factors(estimator);
  ctvio::SolveSummary summary = estimator.Solve(std::atoi(argv[3]), false);
  std::cout << summary.BriefReport() << std::endl;

  std::ofstream out(argv[2]);
  w.write_state(out, summary);

  std::vector<double> points, cov, points_only;
  std::vector<int32_t> status;
  const bool ok = estimator.GetLandmarkPoints(points, &cov, &status);
  out << (ok ? 1 : 0) << " " << w.L << "\n";
  for (double v : points) out << v << " ";
  out << "\n";
  for (double v : cov) out << v << " ";
  out << "\n";
  for (int32_t v : status) out << v << " ";
  out << "\n";
  const bool ok_points = estimator.GetLandmarkPoints(points_only);
  out << (ok_points ? 1 : 0) << " " << w.L << "\n";
  for (double v : points_only) out << v << " ";
  out << "\n";
  return 0;
}
