// body_rates_demo.cpp -- TrajectoryEstimator::GetBodyRatesCovariance through the reference-shaped C++ adaptor (include/ctvio_estimator.hpp).
// Input: a window dumped as text by tests/test_gpu_body_rates.py (the layout of tests/estimator_demo.cpp); the window is solved, then the
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

#include "ctvio_estimator.hpp"

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
  int K, F, L, M, NB, V, pn, pnb;
  long long t0, dt;
  in >> K >> F >> L >> M >> NB >> V >> pn >> pnb >> t0 >> dt;
  ctvio::Trajectory traj(dt, t0);
  for (int k = 0; k < K; ++k) { double q[4], p[3]; in >> q[0] >> q[1] >> q[2] >> q[3] >> p[0] >> p[1] >> p[2]; traj.knots_push_back(q, p); }
  std::vector<std::array<double, 3>> bg(F), ba(F);
  for (int f = 0; f < F; ++f) in >> bg[f][0] >> bg[f][1] >> bg[f][2] >> ba[f][0] >> ba[f][1] >> ba[f][2];
  std::vector<double> para_Feature(L);
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
  ctvio::TrajectoryEstimator estimator(&traj, option);

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
  for (int b = 0; b < NB; ++b) {   // the bias chain first: it registers bias states 0..F-1 in order
    int i, j; double w6[6];
    in >> i >> j; for (int c = 0; c < 6; ++c) in >> w6[c];
    estimator.AddBiasFactor(bg[i].data(), bg[j].data(), ba[i].data(), ba[j].data(), 1.0, w6);
  }
  if (pn > 0) estimator.AddMarginalizationFactor(&marg, marg_blocks);
  for (int m = 0; m < M; ++m) estimator.AddIMUMeasurementAnalytic(imu[m], gravity, bg[imu_bias[m]].data(), ba[imu_bias[m]].data(), imu_w);
  for (int v = 0; v < V; ++v) {
    int lm, rowi, rowj; long long ti, tj; double pi[3] = {0, 0, 1}, pj[3] = {0, 0, 1};
    in >> lm >> ti >> tj >> rowi >> rowj >> pi[0] >> pi[1] >> pj[0] >> pj[1];
    estimator.AddImageFeatureDelayAnalytic(ti, rowi, pi, tj, rowj, pj, &para_Feature[lm], &traj.line_delay, false);
  }
  ctvio::SolveSummary summary = estimator.Solve(std::atoi(argv[3]), false);
  std::cout << summary.BriefReport() << std::endl;

  std::ofstream out(argv[2]);
  out.precision(17);
  for (int k = 0; k < K; ++k) {
    for (double v : traj.getKnotSO3(k)) out << v << " ";
    for (double v : traj.getKnotPos(k)) out << v << " ";
    out << "\n";
  }
  for (int f = 0; f < F; ++f) out << bg[f][0] << " " << bg[f][1] << " " << bg[f][2] << " " << ba[f][0] << " " << ba[f][1] << " " << ba[f][2] << "\n";
  for (int l = 0; l < L; ++l) out << para_Feature[l] << "\n";
  out << traj.line_delay << "\n" << summary.s.iterations << " " << summary.s.final_cost << "\n";

  // [1] the twist half of an odometry message at n times
  const int n = std::atoi(argv[4]);
  std::vector<int64_t> times;
  for (int i = 0; i < n; ++i) times.push_back((int64_t)(t0 + (long long)(i + 1) * (K - 4) * dt / (n + 1)));
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
  const double meas6[6] = {imu[g].gyro[0], imu[g].gyro[1], imu[g].gyro[2], imu[g].accel[0], imu[g].accel[1], imu[g].accel[2]};
  std::vector<double> chi2;
  const bool ok_gate = estimator.GetBodyRatesCovariance({imu[g].timestamp}, bg[imu_bias[g]].data(), rates, cov, meas6, nullptr, &chi2);
  out << (ok_gate ? 1 : 0) << " " << chi2[0] << "\n";
  return 0;
}
