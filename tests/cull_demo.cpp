// cull_demo.cpp -- solve -> cull -> solve on ONE upload, through the C ABI (include/ctvio.h).  Input: a window dumped as text by
// tests/test_gpu_cull_demo.py (the layout tests/demo_window.hpp reads), a shift in normalised image units and the indices of the visual
// blocks whose observation p_j is moved by it (wrong matches).  The adaptor packs and solves the corrupted window (TrajectoryEstimator::Solve:
// ctvio_set_batch + ctvio_solve on the cached handle); the rest is the C entries on that handle, which still holds the window at its solved
// state: ctvio_cull_visual_batch at the 99 % point, ctvio_get_visual_active, ctvio_solve again, ctvio_get_state; then one block is re-admitted
// with ctvio_set_visual_active and read back.
// Output: the solved state (DemoWindow::write_state's layout) with `iterations final_cost` of the re-solve, `n_culled`, the culled blocks
// (order of the AddImageFeatureDelayAnalytic calls), then the final cost with the outliers, the re-solve's initial and final cost, and the
// number of inactive blocks after the re-admission.  Built and run by the GPU test only.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "demo_window.hpp"

static void chk(int rc) {
  if (rc) throw std::runtime_error(std::string(ctvio_status_string(rc)) + ": " + ctvio_last_error());
}

int main(int argc, char **argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters shift block...\n", argv[0]); return 2; }
  const int iters = std::atoi(argv[3]);
  const double shift = std::atof(argv[4]);
  std::ifstream in(argv[1]);
  DemoWindow w = DemoWindow::read(in);
  for (int a = 5; a < argc; ++a) {
    const int v = std::atoi(argv[a]);
    if (v < 0 || v >= w.V) return 2;
    w.blocks[(size_t)v].pj[0] += shift;
    w.blocks[(size_t)v].pj[1] -= 0.5 * shift;
  }
  const ctvio::TrajectoryEstimatorOptions opt = w.options();
  ctvio::TrajectoryEstimator estimator(w.traj.get(), opt);
  w.add_factors(estimator);
  const ctvio::SolveSummary first = estimator.Solve(iters, false);
  std::cout << "with the outliers: " << first.BriefReport() << std::endl;

  ctvio_solver *s = ctvio::SolverCache::get(opt.device, opt.precision);   // the handle Solve uploaded to
  if (ctvio_num_windows(s) != 1) return 3;
  ctvio_cull_options o;
  ctvio_default_cull_options(&o);
  int32_t n_culled = -1;
  std::vector<uint8_t> active((size_t)w.V, 2), now((size_t)w.V, 2);
  chk(ctvio_cull_visual_batch(s, &o, &n_culled, active.data()));
  chk(ctvio_get_visual_active(s, 0, now.data()));
  if (now != active) return 4;
  ctvio::SolveSummary second;
  chk(ctvio_solve(s, iters, &second.s));
  std::cout << "culled " << n_culled << " of " << w.V << " image blocks; re-solve: " << second.BriefReport() << std::endl;
  std::vector<double> quat(4 * (size_t)w.K), pos(3 * (size_t)w.K), bias(6 * (size_t)w.F), rho((size_t)w.L);
  double ld = 0.0;
  chk(ctvio_get_state(s, 0, quat.data(), pos.data(), bias.data(), rho.data(), &ld));

  std::vector<int> culled;
  for (int v = 0; v < w.V; ++v) if (!active[(size_t)v]) culled.push_back(v);
  int inactive_after = -1;
  if (!culled.empty()) {                         // re-admission: the first culled block is switched on again
    now[(size_t)culled[0]] = 1;
    chk(ctvio_set_visual_active(s, 0, now.data()));
    chk(ctvio_get_visual_active_batch(s, active.data()));
    inactive_after = 0;
    for (uint8_t a : active) inactive_after += a ? 0 : 1;
  }

  std::ofstream out(argv[2]);
  out.precision(17);
  for (int k = 0; k < w.K; ++k) {
    for (int c = 0; c < 4; ++c) out << quat[4 * (size_t)k + c] << " ";
    for (int c = 0; c < 3; ++c) out << pos[3 * (size_t)k + c] << " ";
    out << "\n";
  }
  for (int f = 0; f < w.F; ++f) { for (int c = 0; c < 6; ++c) out << bias[6 * (size_t)f + c] << " "; out << "\n"; }
  for (double r : rho) out << r << "\n";
  out << ld << "\n" << second.s.iterations << " " << second.s.final_cost << "\n";
  out << n_culled << "\n";
  for (int v : culled) out << v << " ";
  out << "\n" << first.s.final_cost << " " << second.s.initial_cost << " " << second.s.final_cost << " " << inactive_after << "\n";
  return 0;
}
