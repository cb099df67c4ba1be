// pose_covariance_demo.cpp -- TrajectoryEstimator::GetPoseCovariance through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp).
// Input: a window dumped as text by tests/test_gpu_pose_covariance.py (the layout tests/demo_window.hpp reads); the window is solved, then the
// 6 x 6 covariance of the pose is asked for at n times spread over the spline, t0 + (i + 1) (K - 4) dt / (n + 1), for the body and for the camera.
// Output: the solved state in the same text layout, then `ok n` and the n x 36 body-pose covariances, then the same for the camera pose, then
// whether a time outside the spline was reported (false, not thrown).  Built and run by the GPU test only.
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
  std::vector<double> cov;
  const bool ok = estimator.GetPoseCovariance(times, cov);
  out << (ok ? 1 : 0) << " " << n << "\n";
  for (double v : cov) out << v << " ";
  out << "\n";
  const bool ok_cam = estimator.GetPoseCovariance(times, cov, w.traj->q_CI, w.traj->p_CI);
  out << (ok_cam ? 1 : 0) << " " << n << "\n";
  for (double v : cov) out << v << " ";
  out << "\n";
  const bool ok_outside = estimator.GetPoseCovariance({(int64_t)(w.t0 - 1)}, cov);
  out << (ok_outside ? 1 : 0) << "\n";
  return 0;
}
