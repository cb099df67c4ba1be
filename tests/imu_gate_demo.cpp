// imu_gate_demo.cpp -- TrajectoryEstimator::GateIMUSamples through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp): after the
// solve, check the IMU samples.  Input: a window dumped as text by tests/test_gpu_imu_gate_demo.py (the layout of tests/estimator_demo.cpp),
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

#include "ctvio_estimator.hpp"

int main(int argc, char **argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: %s in.txt out.txt max_iters sample offset\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  int K, F, L, M, NB, V, pn, pnb;
  long long t0, dt;
  in >> K >> F >> L >> M >> NB >> V >> pn >> pnb >> t0 >> dt;
  ctvio::Trajectory traj(dt, t0);
  for (int k = 0; k < K; ++k) { double q[4], p[3]; in >> q[0] >> q[1] >> q[2] >> q[3] >> p[0] >> p[1] >> p[2]; traj.knots_push_back(q, p); }
  std::vector<std::array<double, 3>> bg(F), ba(F);   // the reference keeps these in a std::map<int64_t, IMUBias>
  for (int f = 0; f < F; ++f) in >> bg[f][0] >> bg[f][1] >> bg[f][2] >> ba[f][0] >> ba[f][1] >> ba[f][2];
  std::vector<double> para_Feature(L);               // para_Feature[NUM_OF_F][1], trajectory_manager.h:96
  for (int l = 0; l < L; ++l) in >> para_Feature[l];
  double ld, ld_lo, ld_hi; int fix_ld;
  in >> ld >> ld_lo >> ld_hi >> fix_ld;
  traj.SetLineDelay(ld, fix_ld != 0, ld_lo, ld_hi);
  for (int c = 0; c < 4; ++c) in >> traj.q_CI[c];
  for (int c = 0; c < 3; ++c) in >> traj.p_CI[c];
  double gravity[3], imu_w[6], img_w;
  for (int c = 0; c < 3; ++c) in >> gravity[c];
  for (int c = 0; c < 6; ++c) in >> imu_w[c];
  in >> img_w;


  ctvio::TrajectoryEstimatorOptions option;
  option.lock_ab = false; option.lock_wb = false; option.image_weight = img_w;

  // [1] prior
  ctvio::MarginalizationInfo marg;
  std::vector<double *> marg_blocks;
  if (pn > 0) {
    marg.n = pn;
    marg.linearized_jacobians.resize((size_t)pn * pn);
    marg.linearized_residuals.resize(pn);
    for (auto &v : marg.linearized_jacobians) in >> v;   // column-major
    for (auto &v : marg.linearized_residuals) in >> v;
    for (int b = 0; b < pnb; ++b) {
      int kind, index, off; std::array<double, 4> x0;
      in >> kind >> index >> off >> x0[0] >> x0[1] >> x0[2] >> x0[3];
      marg.keep_block_size.push_back(kind == 0 ? 4 : (kind == 4 ? 1 : 3));
      marg.keep_block_idx.push_back(off);
      marg.keep_block_data.push_back(x0);
      double *p = kind == 0 ? traj.getKnotSO3(index).data() : kind == 1 ? traj.getKnotPos(index).data()
                 : kind == 2 ? bg[index].data() : kind == 3 ? ba[index].data() : &traj.line_delay;
      marg_blocks.push_back(p);
    }
  }
  std::vector<ctvio::IMUData> imu(M); std::vector<int> imu_bias(M);
  for (int m = 0; m < M; ++m) {
    long long t; in >> t; imu[m].timestamp = t;
    in >> imu[m].gyro[0] >> imu[m].gyro[1] >> imu[m].gyro[2] >> imu[m].accel[0] >> imu[m].accel[1] >> imu[m].accel[2] >> imu_bias[m];
  }
  struct Link { int i, j; double w6[6]; };
  std::vector<Link> links(NB);
  for (Link &b : links) { in >> b.i >> b.j; for (int c = 0; c < 6; ++c) in >> b.w6[c]; }
  struct Block { int lm, rowi, rowj; long long ti, tj; double pi[3], pj[3]; };
  std::vector<Block> blocks(V);
  for (Block &b : blocks) { b.pi[2] = b.pj[2] = 1.0; in >> b.lm >> b.ti >> b.tj >> b.rowi >> b.rowj >> b.pi[0] >> b.pi[1] >> b.pj[0] >> b.pj[1]; }
  // the factors of one solve, in the order of tests/estimator_demo.cpp (bias chain first: registers the bias states in frame order)
  auto add_factors = [&](ctvio::TrajectoryEstimator &est) {
    for (const Link &b : links) est.AddBiasFactor(bg[b.i].data(), bg[b.j].data(), ba[b.i].data(), ba[b.j].data(), 1.0, b.w6);
    if (pn > 0) est.AddMarginalizationFactor(&marg, marg_blocks);
    for (int m = 0; m < M; ++m) est.AddIMUMeasurementAnalytic(imu[m], gravity, bg[imu_bias[m]].data(), ba[imu_bias[m]].data(), imu_w);
    for (const Block &b : blocks) est.AddImageFeatureDelayAnalytic(b.ti, b.rowi, b.pi, b.tj, b.rowj, b.pj, &para_Feature[b.lm], &traj.line_delay, false);
  };
  const int iters = std::atoi(argv[3]), bad = std::atoi(argv[4]);
  const double offset = std::atof(argv[5]);
  if (bad < 0 || bad >= M) return 2;
  imu[(size_t)bad].gyro[0] += offset;      // the glitch
  ctvio::TrajectoryEstimator estimator(&traj, option);
  add_factors(estimator);
  std::cout << estimator.Solve(iters, false).BriefReport() << std::endl;

  ctvio::TrajectoryEstimator::IMUGate gate, again;
  std::map<const double *, ctvio::TrajectoryEstimator::FrameGate> frames;
  const bool ok = estimator.GateIMUSamples(gate, &frames);
  std::ofstream out(argv[2]);
  out.precision(17);
  out << (ok ? 1 : 0) << " " << M << "\n";
  for (double v : gate.chi2) out << v << " ";
  out << "\n";
  for (int32_t v : gate.status) out << v << " ";
  out << "\n";
  for (double v : gate.res6) out << v << " ";
  out << "\n" << F << "\n";
  for (int f = 0; f < F; ++f) {
    const auto it = frames.find(bg[f].data());
    if (it == frames.end()) out << "-1 0 0 0\n";
    else out << it->second.count << " " << it->second.mean_chi2 << " " << it->second.max_chi2 << " " << it->second.min_redundancy << "\n";
  }
  const bool ok_cov = estimator.GateIMUSamples(again, nullptr, 0.01, true);
  out << (ok_cov ? 1 : 0) << " " << M << "\n";
  for (double v : again.res6) out << v << " ";
  out << "\n";
  int worst = 0;
  for (int m = 1; m < M; ++m) if (gate.chi2[(size_t)m] > gate.chi2[(size_t)worst]) worst = m;
  std::printf("largest chi2: sample %d, %.6g (corrupted: sample %d, %.6g)\n", worst, gate.chi2[(size_t)worst], bad, gate.chi2[(size_t)bad]);
  return worst == bad && gate.chi2[(size_t)bad] > 16.81 ? 0 : 1;
}
