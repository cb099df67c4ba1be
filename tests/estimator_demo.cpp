// estimator_demo.cpp -- drives libctvio.so through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp)
// the way TrajectoryManager::UpdateTrajectory drives TrajectoryEstimator (reference
// src/estimator/trajectory_manager.cpp:350-463).  Input: a window dumped as text by tests/test_gpu_adaptor.py;
// output: the solved state, same text layout.  Built and run by the GPU test only.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <vector>

#include "demo_window.hpp"

int main(int argc, char **argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters [fp64]\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  const DemoWindow w = DemoWindow::read(in);
  ctvio::TrajectoryEstimatorOptions option = w.options();
  if (argc > 4) option.precision = CTVIO_FP64;
  ctvio::TrajectoryEstimator estimator(w.traj.get(), option);
  w.add_factors(estimator);
  ctvio::SolveSummary summary = estimator.Solve(std::atoi(argv[3]), false);
  std::cout << summary.BriefReport() << std::endl;

  std::ofstream out(argv[2]);
  w.write_state(out, summary);
  return 0;
}
