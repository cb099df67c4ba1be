// slide_demo.cpp -- three consecutive sliding windows driven through the reference-shaped C++ adaptor
// (include/ctvio_estimator.hpp) exactly the way the reference's TrajectoryManager drives TrajectoryEstimator:
//   UpdateTrajectory   (src/estimator/trajectory_manager.cpp:317-483): prior + image + IMU + bias factors, Solve(15),
//   double2vector      (:485-516): 4-DoF gauge restore,
//   UpdateVIOPrior     (:122-286, MARGIN_OLD): PrepareMarginalizationInfo / marg_this_factor / SaveMarginalizationInfo.
// Input: the 13-frame world dumped by tests/test_gpu_slide.py (same text layout as tests/test_gpu_adaptor.py); output: the
// live state after the third window.  The protocol is the one of tests/slide_helpers.py, which runs it with the CPU oracle.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include "ctvio_packer.hpp"
#include "demo_window.hpp"

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s world.txt out.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  DemoWindow w = DemoWindow::read(in);   // the bias indices and the bias chain of the dump are not used: both are recomputed per window below
  ctvio::Trajectory &traj = *w.traj;
  // the initial (synthetic gauge) prior, blocks by pointer
  ctvio::MarginalizationInfo &last_marginalization_info = w.marg;
  std::vector<double *> &last_marginalization_parameter_blocks = w.marg_blocks;
  bool have_prior = w.pn > 0;
  std::vector<long long> anchor_t(w.L, -1);
  for (const DemoWindow::Block &o : w.blocks) anchor_t[o.lm] = o.ti;
  const long long FRAME_DT = 100000000LL;
  const int WIN = 11, WINDOW_SIZE = 10, NWIN = 3;

  for (int k = 0; k < NWIN; ++k) {
    int64_t timestamps[WIN];
    std::vector<int64_t> frame_t(WIN);
    for (int i = 0; i < WIN; ++i) timestamps[i] = frame_t[i] = (int64_t)(k + i) * FRAME_DT;
    const int min_idx = (int)traj.computeTIndexNs(timestamps[0]).second;
    const int64_t opt_min_time = (int64_t)min_idx * traj.getDtNs(), opt_max_time = timestamps[WIN - 1];
    const int last_knot = std::min((int)traj.numKnots() - 1, (int)traj.computeTIndexNs(timestamps[WIN - 1] + (int64_t)(0.039 * 1e9)).second + 3);
    std::vector<int64_t> imu_t_win;
    for (const auto &v : w.imu) if (ctvio::imu_in_window(v.timestamp, opt_min_time, opt_max_time)) imu_t_win.push_back(v.timestamp);
    const std::vector<int32_t> bias_idx = ctvio::imu_bias_index(imu_t_win, frame_t);
    const std::vector<double> sqrt_info_bias = ctvio::bias_chain_sqrt_info(imu_t_win, frame_t, 2.0e-5, 4.0e-4);
    double *para_bg[WIN], *para_ba[WIN];
    for (int i = 0; i < WIN; ++i) { para_bg[i] = w.bg[k + i].data(); para_ba[i] = w.ba[k + i].data(); }
    auto candidate = [&](int lm) { const int a = (int)(anchor_t[lm] / FRAME_DT); return a >= k && a - k < WINDOW_SIZE - 2; };

    // ---------------- UpdateTrajectory
    double q0[4], p0[3];
    for (int c = 0; c < 4; ++c) q0[c] = traj.getKnotSO3(min_idx)[c];
    for (int c = 0; c < 3; ++c) p0[c] = traj.getKnotPos(min_idx)[c];
    {
      ctvio::TrajectoryEstimatorOptions option;
      option.image_weight = w.img_w;
      ctvio::TrajectoryEstimator estimator(&traj, option);
      for (int i = 0; i + 1 < WIN; ++i)   // bias factors first: registers the bias states in frame order
        estimator.AddBiasFactor(para_bg[i], para_bg[i + 1], para_ba[i], para_ba[i + 1], 1.0, &sqrt_info_bias[6 * i]);
      if (have_prior) estimator.AddMarginalizationFactor(&last_marginalization_info, last_marginalization_parameter_blocks);
      for (const DemoWindow::Block &o : w.blocks)
        if (candidate(o.lm) && o.tj <= timestamps[WIN - 1])
          estimator.AddImageFeatureDelayAnalytic(o.ti, o.rowi, o.pi, o.tj, o.rowj, o.pj, &w.para_Feature[o.lm], &traj.line_delay, false);
      size_t n = 0;
      for (const auto &v : w.imu)
        if (ctvio::imu_in_window(v.timestamp, opt_min_time, opt_max_time)) {
          estimator.AddIMUMeasurementAnalytic(v, w.gravity, para_bg[bias_idx[n]], para_ba[bias_idx[n]], w.imu_w);
          ++n;
        }
      const ctvio::SolveSummary summary = estimator.Solve(15, false);
      std::cout << "window " << k << ": " << summary.BriefReport() << std::endl;
      if (k == 0) std::cout << estimator.GetResidualSummary("after solve").PrintSummary();
    }
    ctvio::gauge_restore_4dof(traj, min_idx, last_knot, q0, p0);   // double2vector
    if (k + 1 == NWIN) break;

    // ---------------- UpdateVIOPrior(MARGIN_OLD)
    {
      ctvio::TrajectoryEstimatorOptions option;
      option.image_weight = w.img_w;
      option.is_marg_state = true;
      // the selection rules of UpdateVIOPrior(MARGIN_OLD) come from include/ctvio_packer.hpp
      const ctvio::MargOldSelection sel = ctvio::marg_old_selection(traj, timestamps[0], timestamps[1], para_bg[0], para_ba[0],
                                                                    last_marginalization_parameter_blocks);
      option.ctrl_to_be_opt_now = sel.ctrl_to_be_opt_now;
      option.ctrl_to_be_opt_later = sel.ctrl_to_be_opt_later;
      ctvio::TrajectoryEstimator estimator(&traj, option);
      if (have_prior && !sel.drop_set.empty())   // [1] prior: drop the knots in [now, later) and the oldest bias
        estimator.PrepareMarginalizationInfo(&last_marginalization_info, last_marginalization_parameter_blocks, sel.drop_set);
      for (const DemoWindow::Block &o : w.blocks) {   // [2] image: features anchored at the oldest frame are marginalised
        if (!candidate(o.lm) || o.tj > timestamps[WIN - 1]) continue;
        const bool marg_this_factor = ctvio::marg_this_feature((int)(anchor_t[o.lm] / FRAME_DT) - k, w.para_Feature[o.lm]);
        estimator.AddImageFeatureDelayAnalytic(o.ti, o.rowi, o.pi, o.tj, o.rowj, o.pj, &w.para_Feature[o.lm], &traj.line_delay, false, marg_this_factor);
      }
      for (const auto &v : w.imu)   // [3] IMU before the second keyframe
        if (ctvio::imu_in_marg_old(v.timestamp, opt_min_time, timestamps[1]))
          estimator.AddIMUMeasurementAnalytic(v, w.gravity, para_bg[0], para_ba[0], w.imu_w, true);
      estimator.AddBiasFactor(para_bg[0], para_bg[1], para_ba[0], para_ba[1], 1.0, &sqrt_info_bias[0], true);   // [4]
      have_prior = estimator.SaveMarginalizationInfo(last_marginalization_info, last_marginalization_parameter_blocks);
      std::cout << "prior " << k << ": n = " << last_marginalization_info.n << ", blocks = " << last_marginalization_parameter_blocks.size() << std::endl;
    }
  }

  std::ofstream out(argv[2]);
  out.precision(17);
  for (int k = 0; k < w.K; ++k) {
    for (double v : traj.getKnotSO3(k)) out << v << " ";
    for (double v : traj.getKnotPos(k)) out << v << " ";
    out << "\n";
  }
  for (int f = 0; f < w.F; ++f) out << w.bg[f][0] << " " << w.bg[f][1] << " " << w.bg[f][2] << " " << w.ba[f][0] << " " << w.ba[f][1] << " " << w.ba[f][2] << "\n";
  for (int l = 0; l < w.L; ++l) out << w.para_Feature[l] << "\n";
  out << traj.line_delay << "\n";
  // the consumers' side of the solve (trajectory_manager.cpp:108-120, odometry_manager.cpp:287): queries on the optimised spline,
  // evaluated on the device through ctvio::Trajectory
  ctvio::ExtrinsicParam EP_CtoI;
  for (int c = 0; c < 4; ++c) EP_CtoI.q[c] = traj.q_CI[c];
  for (int c = 0; c < 3; ++c) EP_CtoI.p[c] = traj.p_CI[c];
  traj.SetSensorExtrinsics(ctvio::CameraSensor, EP_CtoI);
  traj.SetDataStartTime(12345);
  const int64_t tq = traj.maxTimeNs() - (int64_t)(0.05 * 1e9);
  const ctvio::SE3 cam = traj.GetCameraPose(tq);
  ctvio::IMUState ist;
  traj.GetIMUState(tq, ist);
  const ctvio::SE3 last = traj.getLastKnot();
  traj.setKnot(traj.getKnot(traj.numKnots() - 1), (int)traj.numKnots() - 1);
  out << tq << " " << traj.GetDataStartTime() << "\n";
  for (double v : cam.p) out << v << " ";
  for (double v : cam.q) out << v << " ";
  out << "\n";
  for (double v : ist.p) out << v << " ";
  for (double v : ist.q) out << v << " ";
  for (double v : ist.v) out << v << " ";
  out << "\n";
  for (double v : last.p) out << v << " ";
  for (double v : last.q) out << v << " ";
  out << "\n";
  return 0;
}
