// demo_window.hpp -- the text dump of one window (tests/query_harness.py: _dump) as the adaptor demos take it: test infrastructure, included
// by tests/*_demo.cpp only.  read() fills the trajectory and the parameter blocks a caller of the reference keeps (bias states, inverse
// depths), add_factors() hands them to a TrajectoryEstimator in the one order every demo uses, write_state() prints them back.
#pragma once
#include <array>
#include <istream>
#include <memory>
#include <ostream>
#include <vector>

#include "ctvio_estimator.hpp"

struct DemoWindow {
  struct Link { int i, j; double w6[6]; };
  struct Block { int lm, rowi, rowj; long long ti, tj; double pi[3], pj[3]; };

  int K = 0, F = 0, L = 0, M = 0, NB = 0, V = 0, pn = 0, pnb = 0;
  long long t0 = 0, dt = 0;
  std::unique_ptr<ctvio::Trajectory> traj;   // on the heap: the prior's block pointers survive a move of the window
  // parameter blocks: the estimator writes its solution through the pointers add_factors() gives it
  mutable std::vector<std::array<double, 3>> bg, ba;   // the reference keeps these in a std::map<int64_t, IMUBias>
  mutable std::vector<double> para_Feature;            // para_Feature[NUM_OF_F][1], trajectory_manager.h:96
  double gravity[3] = {0, 0, 0}, imu_w[6] = {0, 0, 0, 0, 0, 0}, img_w = 0;
  ctvio::MarginalizationInfo marg;
  std::vector<double *> marg_blocks;
  std::vector<ctvio::IMUData> imu;
  std::vector<int> imu_bias;
  std::vector<Link> links;
  std::vector<Block> blocks;

  static DemoWindow read(std::istream &in) {
    DemoWindow w;
    in >> w.K >> w.F >> w.L >> w.M >> w.NB >> w.V >> w.pn >> w.pnb >> w.t0 >> w.dt;
    w.traj.reset(new ctvio::Trajectory(w.dt, w.t0));
    ctvio::Trajectory &traj = *w.traj;
    for (int k = 0; k < w.K; ++k) { double q[4], p[3]; in >> q[0] >> q[1] >> q[2] >> q[3] >> p[0] >> p[1] >> p[2]; traj.knots_push_back(q, p); }
    w.bg.resize(w.F); w.ba.resize(w.F);
    for (int f = 0; f < w.F; ++f) in >> w.bg[f][0] >> w.bg[f][1] >> w.bg[f][2] >> w.ba[f][0] >> w.ba[f][1] >> w.ba[f][2];
    w.para_Feature.resize(w.L);
    for (double &v : w.para_Feature) in >> v;
    double ld, ld_lo, ld_hi; int fix_ld;
    in >> ld >> ld_lo >> ld_hi >> fix_ld;
    traj.SetLineDelay(ld, fix_ld != 0, ld_lo, ld_hi);
    for (int c = 0; c < 4; ++c) in >> traj.q_CI[c];
    for (int c = 0; c < 3; ++c) in >> traj.p_CI[c];
    for (int c = 0; c < 3; ++c) in >> w.gravity[c];
    for (int c = 0; c < 6; ++c) in >> w.imu_w[c];
    in >> w.img_w;
    if (w.pn > 0) {
      ctvio::MarginalizationInfo &marg = w.marg;
      marg.n = w.pn;
      marg.linearized_jacobians.resize((size_t)w.pn * w.pn);
      marg.linearized_residuals.resize(w.pn);
      for (auto &v : marg.linearized_jacobians) in >> v;   // column-major
      for (auto &v : marg.linearized_residuals) in >> v;
      for (int b = 0; b < w.pnb; ++b) {
        int kind, index, off; std::array<double, 4> x0;
        in >> kind >> index >> off >> x0[0] >> x0[1] >> x0[2] >> x0[3];
        marg.keep_block_size.push_back(kind == 0 ? 4 : (kind == 4 ? 1 : 3));
        marg.keep_block_idx.push_back(off);
        marg.keep_block_data.push_back(x0);
        double *p = kind == 0 ? traj.getKnotSO3(index).data() : kind == 1 ? traj.getKnotPos(index).data()
                   : kind == 2 ? w.bg[index].data() : kind == 3 ? w.ba[index].data() : &traj.line_delay;
        w.marg_blocks.push_back(p);
      }
    }
    w.imu.resize(w.M); w.imu_bias.resize(w.M);
    for (int m = 0; m < w.M; ++m) {
      ctvio::IMUData &d = w.imu[m];
      long long t; in >> t; d.timestamp = t;
      in >> d.gyro[0] >> d.gyro[1] >> d.gyro[2] >> d.accel[0] >> d.accel[1] >> d.accel[2] >> w.imu_bias[m];
    }
    w.links.resize(w.NB);
    for (Link &b : w.links) { in >> b.i >> b.j; for (int c = 0; c < 6; ++c) in >> b.w6[c]; }
    w.blocks.resize(w.V);
    for (Block &b : w.blocks) { b.pi[2] = b.pj[2] = 1.0; in >> b.lm >> b.ti >> b.tj >> b.rowi >> b.rowj >> b.pi[0] >> b.pi[1] >> b.pj[0] >> b.pj[1]; }
    return w;
  }

  ctvio::TrajectoryEstimatorOptions options() const {
    ctvio::TrajectoryEstimatorOptions option;
    option.lock_ab = false; option.lock_wb = false; option.image_weight = img_w;
    return option;
  }

  // the factors of one solve: the bias chain first (it registers bias states 0..F-1 in frame order, so that indices follow the frames),
  // then the prior, the IMU samples, the image blocks
  void add_factors(ctvio::TrajectoryEstimator &est) const {
    for (const Link &b : links) est.AddBiasFactor(bg[b.i].data(), bg[b.j].data(), ba[b.i].data(), ba[b.j].data(), 1.0, b.w6);
    if (pn > 0) est.AddMarginalizationFactor(&marg, marg_blocks);
    for (int m = 0; m < M; ++m) est.AddIMUMeasurementAnalytic(imu[m], gravity, bg[imu_bias[m]].data(), ba[imu_bias[m]].data(), imu_w);
    for (const Block &b : blocks) est.AddImageFeatureDelayAnalytic(b.ti, b.rowi, b.pi, b.tj, b.rowj, b.pj, &para_Feature[b.lm], &traj->line_delay, false);
  }

  // the state in the layout of the dump's state part, then `iterations final_cost`; 17 digits
  void write_state(std::ostream &out, const ctvio::SolveSummary &summary) const {
    out.precision(17);
    for (int k = 0; k < K; ++k) {
      for (double v : traj->getKnotSO3(k)) out << v << " ";
      for (double v : traj->getKnotPos(k)) out << v << " ";
      out << "\n";
    }
    for (int f = 0; f < F; ++f) out << bg[f][0] << " " << bg[f][1] << " " << bg[f][2] << " " << ba[f][0] << " " << ba[f][1] << " " << ba[f][2] << "\n";
    for (int l = 0; l < L; ++l) out << para_Feature[l] << "\n";
    out << traj->line_delay << "\n" << summary.s.iterations << " " << summary.s.final_cost << "\n";
  }
};
