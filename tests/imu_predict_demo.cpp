// imu_predict_demo.cpp -- TrajectoryEstimator::PredictIMUStates through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp).
// Input: a window dumped as text by tests/test_gpu_imu_predict.py (the layout tests/demo_window.hpp reads) and a file of IMU samples: m, then
// m lines `t_ns gx gy gz ax ay az`.  The window is solved, then the state is carried through the samples with the reference's default noise,
// with the newest bias state (nullptr) and with bias state 1 (by its gyro-bias pointer).
// Output: the solved state in the same text layout, then `ok m`, the m states (px py pz qx qy qz qw vx vy vz) and the m x 225 covariances,
// then the same for bias state 1.  Built and run by the GPU test only.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <vector>

#include "demo_window.hpp"

int main(int argc, char **argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters samples.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  const DemoWindow w = DemoWindow::read(in);
  ctvio::TrajectoryEstimator estimator(w.traj.get(), w.options());
  w.add_factors(estimator);
  ctvio::SolveSummary summary = estimator.Solve(std::atoi(argv[3]), false);
  std::cout << summary.BriefReport() << std::endl;

  std::ofstream out(argv[2]);
  w.write_state(out, summary);

  std::ifstream sin(argv[4]);
  int m = 0;
  sin >> m;
  std::vector<ctvio::IMUData> samples((size_t)m);
  for (auto &d : samples) {
    long long t; sin >> t; d.timestamp = t;
    sin >> d.gyro[0] >> d.gyro[1] >> d.gyro[2] >> d.accel[0] >> d.accel[1] >> d.accel[2];
  }
  ctvio_imu_noise noise;
  ctvio_default_imu_noise(&noise);
  std::vector<ctvio::IMUState> states;
  std::vector<double> cov;
  auto write = [&](bool ok) {
    out << (ok ? 1 : 0) << " " << m << "\n";
    for (const ctvio::IMUState &st : states)
      out << st.p[0] << " " << st.p[1] << " " << st.p[2] << " " << st.q[0] << " " << st.q[1] << " " << st.q[2] << " " << st.q[3] << " " << st.v[0] << " "
          << st.v[1] << " " << st.v[2] << "\n";
    for (double v : cov) out << v << " ";
    out << "\n";
  };
  write(estimator.PredictIMUStates(samples, nullptr, noise, states, cov));
  write(estimator.PredictIMUStates(samples, w.bg[1].data(), noise, states, cov));
  return 0;
}
