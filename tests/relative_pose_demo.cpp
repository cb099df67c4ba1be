// relative_pose_demo.cpp -- TrajectoryEstimator::GetRelativePoseCovariance through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp).
// Input: a window dumped as text by tests/test_gpu_relative_pose.py (the layout tests/demo_window.hpp reads); the window is solved, then the
// pose increment and its 6 x 6 covariance are asked for between the consecutive ones of n times spread over the spline,
// t_i = t0 + (i + 1) (K - 4) dt / (n + 1): the pairs (t_i, t_i+1), i < n - 1, and (t_n-1, t_0), for the body and for the camera.
// Output: the solved state in the same text layout, then `ok n`, the n x 7 increments and the n x 36 covariances of the body, then the same for
// the camera, then whether a time outside the spline was reported (false, not thrown).  Built and run by the GPU test only.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <vector>

#include "demo_window.hpp"

int main(int argc, char **argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters n_times\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  const DemoWindow w = DemoWindow::read(in);
  ctvio::TrajectoryEstimator estimator(w.traj.get(), w.options());
  w.add_factors(estimator);
  ctvio::SolveSummary summary = estimator.Solve(std::atoi(argv[3]), false);
  std::cout << summary.BriefReport() << std::endl;

  std::ofstream out(argv[2]);
  w.write_state(out, summary);

  const int n = std::atoi(argv[4]);
  std::vector<int64_t> times;
  for (int i = 0; i < n; ++i) times.push_back((int64_t)(w.t0 + (long long)(i + 1) * (w.K - 4) * w.dt / (n + 1)));
  std::vector<std::pair<int64_t, int64_t>> pairs;
  for (int i = 0; i < n; ++i) pairs.emplace_back(times[i], times[(i + 1) % n]);
  std::vector<double> rel, cov;
  auto write = [&](bool ok) {
    out << (ok ? 1 : 0) << " " << n << "\n";
    for (double v : rel) out << v << " ";
    out << "\n";
    for (double v : cov) out << v << " ";
    out << "\n";
  };
  write(estimator.GetRelativePoseCovariance(pairs, rel, cov));
  write(estimator.GetRelativePoseCovariance(pairs, rel, cov, w.traj->q_CI, w.traj->p_CI));
  const bool ok_outside = estimator.GetRelativePoseCovariance({{times[0], (int64_t)(w.t0 - 1)}}, rel, cov);
  out << (ok_outside ? 1 : 0) << "\n";
  return 0;
}
