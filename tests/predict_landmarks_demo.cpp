// predict_landmarks_demo.cpp -- TrajectoryEstimator::PredictLandmarks through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp).
// Input: a window as text in the layout of tests/estimator_demo.cpp; the window is solved, then 21 IMU samples at 200 Hz from the newest
// frame time (a constant body rate, the accelerometer reading gravity) carry the state 100 ms past it, to where the next image arrives, and
// every landmark is predicted into that image at row 240 with its 2 x 2 covariance and the gate of a candidate point, and once more as
// values only.
// Output: the solved state in the same text layout, then `ok L`, the L x 3 predictions, the L x 4 covariances, the L gates and the L statuses,
// then `ok L` and the L x 3 predictions of the values-only call.  The tests compile it (-fsyntax-only); it links against libctvio.so.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
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

  long long t_new = w.t0;   // the newest frame time
  for (const DemoWindow::Block &b : w.blocks) t_new = std::max(t_new, std::max(b.ti, b.tj));
  // the samples between the newest frame and the next image; the newest bias state
  std::vector<ctvio::IMUData> next(21);
  for (int j = 0; j < 21; ++j) {
    next[j].timestamp = t_new + 5000000ll * j;
    const double omega[3] = {0.1, -0.2, 0.05};
    for (int c = 0; c < 3; ++c) { next[j].gyro[c] = omega[c]; next[j].accel[c] = w.gravity[c]; }
  }
  ctvio_imu_noise noise;
  ctvio_default_imu_noise(&noise);
  std::vector<ctvio::TrajectoryEstimator::PredictionPoint> points;
  std::vector<double> obs(2 * (size_t)w.L, 0.0);
  for (int l = 0; l < w.L; ++l) points.push_back({&w.para_Feature[l], 240});
  std::vector<double> proj, cov, chi2, proj_only;
  std::vector<int32_t> status;
  ctvio::IMUState end;
  const bool ok = estimator.PredictLandmarks(next, nullptr, noise, points, proj, &cov, &obs, &chi2, nullptr, nullptr, &status, &end);
  out << (ok ? 1 : 0) << " " << w.L << "\n";
  for (double v : proj) out << v << " ";
  out << "\n";
  for (double v : cov) out << v << " ";
  out << "\n";
  for (double v : chi2) out << v << " ";
  out << "\n";
  for (int32_t v : status) out << v << " ";
  out << "\n";
  const bool ok_values = estimator.PredictLandmarks(next, nullptr, noise, points, proj_only);
  out << (ok_values ? 1 : 0) << " " << w.L << "\n";
  for (double v : proj_only) out << v << " ";
  out << "\n";
  return 0;
}
