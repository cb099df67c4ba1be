// imu_gate_demo.cpp -- TrajectoryEstimator::GateIMUSamples through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp): after the
// solve, check the IMU samples.  Input: a window dumped as text by tests/test_gpu_imu_gate_demo.py (the layout tests/demo_window.hpp reads),
// the index of one IMU sample and an offset in rad/s.  That sample's gyro x reading is raised by the offset (0.04 rad/s is 10 sigma at
// imu_w = 250: a glitch), the window is solved with the corrupted sample in it -- the IMU factor has no robust loss --, and every sample
// goes through the leave-one-out test.  Prints the sample with the largest chi2 and exits non-zero unless that is the corrupted one with
// chi2 > 16.81, the 99 % point of chi-square with 6 degrees of freedom.
// Output: `ok M`, the M gates chi2, the M statuses, the M x 6 residuals, then `F` and per gyro-bias pointer (in bias-state order) its count,
// mean chi2, largest chi2 and smallest redundancy; then `ok M` and the M x 6 residuals of a second call with the covariances.  Built and
// run by the GPU test only.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <vector>

#include "demo_window.hpp"

int main(int argc, char **argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters sample offset\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  DemoWindow w = DemoWindow::read(in);
  const int iters = std::atoi(argv[3]), bad = std::atoi(argv[4]);
  const double offset = std::atof(argv[5]);
  if (bad < 0 || bad >= w.M) return 2;
  w.imu[(size_t)bad].gyro[0] += offset;      // the glitch
  ctvio::TrajectoryEstimator estimator(w.traj.get(), w.options());
  w.add_factors(estimator);
  std::cout << estimator.Solve(iters, false).BriefReport() << std::endl;

  ctvio::TrajectoryEstimator::IMUGate gate, again;
  std::map<const double *, ctvio::TrajectoryEstimator::FrameGate> frames;
  const bool ok = estimator.GateIMUSamples(gate, &frames);
  std::ofstream out(argv[2]);
  out.precision(17);
  out << (ok ? 1 : 0) << " " << w.M << "\n";
  for (double v : gate.chi2) out << v << " ";
  out << "\n";
  for (int32_t v : gate.status) out << v << " ";
  out << "\n";
  for (double v : gate.res6) out << v << " ";
  out << "\n" << w.F << "\n";
  for (int f = 0; f < w.F; ++f) {
    const auto it = frames.find(w.bg[f].data());
    if (it == frames.end()) out << "-1 0 0 0\n";
    else out << it->second.count << " " << it->second.mean_chi2 << " " << it->second.max_chi2 << " " << it->second.min_redundancy << "\n";
  }
  const bool ok_cov = estimator.GateIMUSamples(again, nullptr, 0.01, true);
  out << (ok_cov ? 1 : 0) << " " << w.M << "\n";
  for (double v : again.res6) out << v << " ";
  out << "\n";
  int worst = 0;
  for (int m = 1; m < w.M; ++m) if (gate.chi2[(size_t)m] > gate.chi2[(size_t)worst]) worst = m;
  std::printf("largest chi2: sample %d, %.6g (corrupted: sample %d, %.6g)\n", worst, gate.chi2[(size_t)worst], bad, gate.chi2[(size_t)bad]);
  return worst == bad && gate.chi2[(size_t)bad] > 16.81 ? 0 : 1;
}
