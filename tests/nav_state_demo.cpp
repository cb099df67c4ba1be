// nav_state_demo.cpp -- TrajectoryEstimator::GetIMUStateCovariance through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp).
// Input: a window dumped as text by tests/test_gpu_nav_state.py (the layout tests/demo_window.hpp reads); the window is solved, then the
// navigation state and its 15 x 15 covariance are asked for at n times spread over the spline, t0 + (i + 1) (K - 4) dt / (n + 1), with the
// newest bias state (nullptr) and with bias state 1 (by its gyro-bias pointer).
// Output: the solved state in the same text layout, then `ok n`, the n states (16 numbers each, the layout of ctvio_nav_state's state16) and the
// n x 225 covariances, then the same for bias state 1, then whether a time outside the spline was reported (false, not thrown).  Built and
// run by the GPU test only.
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
  std::vector<ctvio::IMUState> states;
  std::vector<double> bias6, cov;
  auto write = [&](bool ok) {
    out << (ok ? 1 : 0) << " " << n << "\n";
    for (size_t i = 0; i < states.size(); ++i) {
      const ctvio::IMUState &st = states[i];
      out << st.p[0] << " " << st.p[1] << " " << st.p[2] << " " << st.q[0] << " " << st.q[1] << " " << st.q[2] << " " << st.q[3] << " " << st.v[0] << " "
          << st.v[1] << " " << st.v[2];
      for (int c = 0; c < 6; ++c) out << " " << bias6[6 * i + c];
      out << "\n";
    }
    for (double v : cov) out << v << " ";
    out << "\n";
  };
  write(estimator.GetIMUStateCovariance(times, nullptr, states, bias6, cov));
  write(estimator.GetIMUStateCovariance(times, w.bg[1].data(), states, bias6, cov));
  const bool ok_outside = estimator.GetIMUStateCovariance({(int64_t)(w.t0 - 1)}, nullptr, states, bias6, cov);
  out << (ok_outside ? 1 : 0) << "\n";
  return 0;
}
