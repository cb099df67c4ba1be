// body_rates_demo.cpp -- TrajectoryEstimator::GetBodyRatesCovariance through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp).
// Input: a window dumped as text by tests/test_gpu_body_rates.py (the layout tests/demo_window.hpp reads); the window is solved, then the
// twist of an odometry message -- child-frame linear velocity v_B and angular velocity omega with their joint 6 x 6 covariance -- is filled
// at n times spread over the spline, t0 + (i + 1) (K - 4) dt / (n + 1), with the newest bias state, and one IMU sample (the window's own
// sample number `gate_sample`, with its own bias state) is gated against the prediction at its time.
// Output: the solved state in the same text layout, then `ok n`, the n x 9 rates and the n x 225 covariances, the n twists (v_B, omega) with
// their 6 x 6 covariances, then `ok chi2` of the gated sample.  Built and run by the GPU test only.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include "demo_window.hpp"

// geometry_msgs/TwistWithCovariance: (linear, angular) and the row-major 6 x 6 covariance in that order
struct Twist { double linear[3], angular[3], covariance[36]; };

// rows / columns 6..8 (v_B) and 0..2 (omega) of the 15 x 15 block
static Twist twist_of(const double *rates9, const double *cov225) {
  static const int pick[6] = {6, 7, 8, 0, 1, 2};
  Twist tw;
  for (int a = 0; a < 3; ++a) { tw.linear[a] = rates9[6 + a]; tw.angular[a] = rates9[a]; }
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) tw.covariance[6 * a + b] = cov225[15 * pick[a] + pick[b]];
  return tw;
}

int main(int argc, char **argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters n_times gate_sample\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  const DemoWindow w = DemoWindow::read(in);
  ctvio::TrajectoryEstimator estimator(w.traj.get(), w.options());
  w.add_factors(estimator);
  ctvio::SolveSummary summary = estimator.Solve(std::atoi(argv[3]), false);
  std::cout << summary.BriefReport() << std::endl;

  std::ofstream out(argv[2]);
  w.write_state(out, summary);

  // [1] the twist half of an odometry message at n times
  const int n = std::atoi(argv[4]);
  std::vector<int64_t> times;
  for (int i = 0; i < n; ++i) times.push_back((int64_t)(w.t0 + (long long)(i + 1) * (w.K - 4) * w.dt / (n + 1)));
  std::vector<double> rates, cov;
  const bool ok = estimator.GetBodyRatesCovariance(times, nullptr, rates, cov);
  out << (ok ? 1 : 0) << " " << n << "\n";
  for (double v : rates) out << v << " ";
  out << "\n";
  for (double v : cov) out << v << " ";
  out << "\n";
  for (int i = 0; i < n; ++i) {
    const Twist tw = twist_of(rates.data() + 9 * i, cov.data() + 225 * i);
    for (double v : tw.linear) out << v << " ";
    for (double v : tw.angular) out << v << " ";
    for (double v : tw.covariance) out << v << " ";
    out << "\n";
  }
  // [2] one IMU sample against the prediction at its time, with its own bias state and the window's weights as the noise
  const int g = std::atoi(argv[5]);
  const double meas6[6] = {w.imu[g].gyro[0], w.imu[g].gyro[1], w.imu[g].gyro[2], w.imu[g].accel[0], w.imu[g].accel[1], w.imu[g].accel[2]};
  std::vector<double> chi2;
  const bool ok_gate = estimator.GetBodyRatesCovariance({w.imu[g].timestamp}, w.bg[w.imu_bias[g]].data(), rates, cov, meas6, nullptr, &chi2);
  out << (ok_gate ? 1 : 0) << " " << chi2[0] << "\n";
  return 0;
}
