// project_landmarks_demo.cpp -- TrajectoryEstimator::ProjectLandmarks through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp).
// Input: a window dumped as text by tests/test_gpu_project_landmarks.py (the layout tests/demo_window.hpp reads); the window is solved, then
// every visual block's landmark is projected into the block's own observation (t_j, row_j) with its 2 x 2 covariance and the gate of the
// observed point, and once more as values only.
// Output: the solved state in the same text layout, then `ok V`, the V x 3 predictions, the V x 4 covariances, the V gates and the V statuses,
// then `ok V` and the V x 3 predictions of the values-only call.  Built and run by the GPU test only.
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

  // every image block again, at its own frame time and row, with its observation as the candidate
  std::vector<ctvio::TrajectoryEstimator::ProjectionQuery> queries;
  std::vector<double> obs;
  for (const DemoWindow::Block &b : w.blocks) {
    queries.push_back({&w.para_Feature[b.lm], (int64_t)b.tj, (int32_t)b.rowj});
    obs.push_back(b.pj[0]); obs.push_back(b.pj[1]);
  }
  std::vector<double> proj, cov, chi2, proj_only;
  std::vector<int32_t> status;
  const bool ok = estimator.ProjectLandmarks(queries, proj, &cov, &obs, &chi2, nullptr, nullptr, &status);
  out << (ok ? 1 : 0) << " " << w.V << "\n";
  for (double v : proj) out << v << " ";
  out << "\n";
  for (double v : cov) out << v << " ";
  out << "\n";
  for (double v : chi2) out << v << " ";
  out << "\n";
  for (int32_t v : status) out << v << " ";
  out << "\n";
  const bool ok_values = estimator.ProjectLandmarks(queries, proj_only);
  out << (ok_values ? 1 : 0) << " " << w.V << "\n";
  for (double v : proj_only) out << v << " ";
  out << "\n";
  return 0;
}
