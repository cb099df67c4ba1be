// host_pack.hpp -- host side of a batch upload: validation and packing of the caller's windows (the factor set of the
// reference's TrajectoryManager::UpdateTrajectory, src/estimator/trajectory_manager.cpp:331-451) into ONE pinned staging
// arena that mirrors the device input arena byte for byte, so that a whole batch reaches HBM with a single
// hipMemcpyAsync.  Windows are independent: both passes (validate + count, then fill) run over the windows with a pool
// of host threads.  No device code in this file.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <limits>
#include <mutex>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ctvio.h"
#include "device_types.hpp"

namespace ctv {

inline int host_threads(int requested) {
  if (requested > 0) return requested;
  const unsigned hw = std::thread::hardware_concurrency();
  return (int)std::max(1u, std::min(hw ? hw : 1u, 16u));
}

// f(i) for i in [0, n), dynamic distribution over `nthreads` threads (the calling thread included).  The threads belong to the solver handle and
// live as long as it does: a batch is packed in two passes, and a pass that creates and joins its threads pays for them every time -- for a batch of 8
// windows (BASELINE configs[3] as written: 8 windows per GPU) that was more than the packing itself.
class WorkerPool {
 public:
  ~WorkerPool() {
    { std::lock_guard<std::mutex> lk(mu_); quit_ = true; }
    cv_.notify_all();
    for (auto &t : th_) t.join();
  }
  template <class F> void run(int n, int nthreads, F &&f) {
    if (nthreads <= 1 || n <= 1) { for (int i = 0; i < n; ++i) f(i); return; }
    const int extra = std::min(nthreads, n) - 1;
    while ((int)th_.size() < extra) th_.emplace_back([this] { loop(); });
    {
      std::lock_guard<std::mutex> lk(mu_);
      job_ = [&f](int i) { f(i); };
      n_ = n; next_.store(0, std::memory_order_relaxed); wanted_ = extra; started_ = 0; running_ = 0; ++epoch_;
    }
    cv_.notify_all();
    work();                                  // the calling thread takes items too
    std::unique_lock<std::mutex> lk(mu_);    // every helper that picked the job up has finished its last item (helpers that never woke take none)
    wanted_ = 0;
    done_.wait(lk, [&] { return running_ == 0; });
    job_ = nullptr;
  }

 private:
  void work() { for (;;) { const int i = next_.fetch_add(1, std::memory_order_relaxed); if (i >= n_) break; job_(i); } }
  void loop() {
    unsigned long long seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return quit_ || (epoch_ != seen && started_ < wanted_); });
        if (quit_) return;
        seen = epoch_; ++started_; ++running_;
      }
      work();
      { std::lock_guard<std::mutex> lk(mu_); --running_; }
      done_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_;
  std::function<void(int)> job_;
  std::atomic<int> next_{0};
  int n_ = 0, wanted_ = 0, started_ = 0, running_ = 0;
  unsigned long long epoch_ = 0;
  bool quit_ = false;
};

// Grow-only device buffer, optionally mirrored by pinned host memory.  The mirror may run `landing` bytes past the device block: landing
// areas of copies whose source lies elsewhere on the device, which need no device twin.
struct Arena {
  char *dev = nullptr, *host = nullptr;
  size_t cap = 0, hcap = 0;
  ~Arena() { release(); }
  void release() {
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = host = nullptr; cap = hcap = 0;
  }
  // returns hipSuccess; *grew tells the caller that the contents (and every pointer into the arena) are gone.  headroom: a slightly larger
  // next batch does not reallocate (not for device-only scratch of tens of MB).
  hipError_t reserve(size_t bytes, bool mirror, bool *grew, size_t landing = 0, bool headroom = true) {
    const size_t hbytes = mirror ? bytes + landing : 0;
    if (grew) *grew = false;
    if (bytes <= cap && dev && hbytes <= hcap && (!mirror || host)) return hipSuccess;
    auto grown = [&](size_t need, size_t have) { return std::max(std::max<size_t>(need + (headroom ? need / 8 : 0), 4096), have); };
    const size_t want = grown(bytes, cap), hwant = mirror ? grown(hbytes, hcap) : 0;
    release();
    hipError_t e = hipMalloc((void **)&dev, want);
    if (e != hipSuccess) { dev = nullptr; return e; }
    if (mirror) {
      e = hipHostMalloc((void **)&host, hwant, hipHostMallocDefault);
      if (e != hipSuccess) { host = nullptr; release(); return e; }
    }
    cap = want; hcap = hwant;
    if (grew) *grew = true;
    return hipSuccess;
  }
};

static inline int prior_block_size(int kind) { return kind == CTVIO_PK_LD ? 1 : 3; }

// Per-window results of the first pass.
struct PackTmp {
  std::vector<int32_t> iorder, iseg;    // IMU: sample order by (segment, bias state); segment of every sample (input order)
  std::vector<int32_t> vord;            // visual blocks: order by (ti, tj, rowi, rowj)  (frame-pair order: the assembly's items)
  std::vector<int32_t> lord, vpos;      // landmark-major slots: lord[slot] = block or -1 (padding), vpos[block] = slot
  std::vector<int32_t> anc_of, anc_rep; // anchors (distinct i ends), numbered landmark-major: anchor of every block / a block that carries it
  std::vector<int32_t> lm_slot, lm_cnt; // per landmark: its first slot (window-relative) and its block count
  int32_t ngrp = 0, nvitem = 0, Vp = 0; // Vp: slots incl. padding, a multiple of 64
  int32_t A = 0;                        // number of anchors
  // sparsity plan (plan_sparsity): rows of W in sorted landmark order, their knot spans, per-tile row ranges, envelope of the reduced system
  std::vector<int32_t> lm_pos, lm_at, row_klo, row_khi, tl_beg, tl_end, env_first, env_tile;
  int32_t Lobs = 0, max_span = 0, ntr = 0;
  std::string err;
};

// reference asserts / prints when a time falls outside the spline (spline_segment.h:74-81); here every input is checked
inline bool validate_window(const ctvio_window *w, std::string &err) {
  auto bad = [&](const char *m) { err = m; return false; };
  if (!w) return bad("null window");
  if (w->K < 4 || w->F < 1 || w->L < 0 || w->M < 0 || w->NB < 0 || w->V < 0 || w->dt_ns <= 0 || w->pn < 0 || w->pnb < 0)
    return bad("bad sizes (need K >= 4, F >= 1, dt_ns > 0)");
  if (!w->quat || !w->pos || !w->bias || (w->L && !w->rho)) return bad("null state pointer");
  if (!std::isfinite(w->ld)) return bad("non-finite line delay");
  if (!w->fix_ld && !(w->ld_lo <= w->ld_hi && std::isfinite(w->ld_lo) && std::isfinite(w->ld_hi))) return bad("line-delay bounds: need finite ld_lo <= ld_hi");
  if (w->M && (!w->imu_t || !w->imu_gyro || !w->imu_acc || !w->imu_bias)) return bad("null IMU pointer");
  if (w->NB && (!w->bc_i || !w->bc_j || !w->bc_w)) return bad("null bias-chain pointer");
  if (w->V && (!w->v_lm || !w->v_ti || !w->v_tj || !w->v_rowi || !w->v_rowj || !w->v_pi || !w->v_pj)) return bad("null visual pointer");
  const int64_t tmax = w->t0_ns + (int64_t)(w->K - 3) * w->dt_ns;
  for (int m = 0; m < w->M; ++m) {
    if (w->imu_t[m] < w->t0_ns || w->imu_t[m] >= tmax) return bad("IMU time outside the spline");
    if (w->imu_bias[m] < 0 || w->imu_bias[m] >= w->F) return bad("IMU bias index out of range");
  }
  const int64_t ldmax_ns = (int64_t)((w->fix_ld ? w->ld : std::max(w->ld, w->ld_hi)) * 1e9);
  const int64_t ldmin_ns = (int64_t)((w->fix_ld ? w->ld : std::min(w->ld, w->ld_lo)) * 1e9);
  for (int v = 0; v < w->V; ++v) {
    if (w->v_lm[v] < 0 || w->v_lm[v] >= w->L) return bad("visual landmark index out of range");
    if (w->v_rowi[v] < 0 || w->v_rowj[v] < 0) return bad("negative image row");
    const int64_t a = w->v_ti[v], b = w->v_tj[v];
    if (a < w->t0_ns || b < w->t0_ns || a + w->v_rowi[v] * ldmax_ns >= tmax || b + w->v_rowj[v] * ldmax_ns >= tmax ||
        a + w->v_rowi[v] * ldmin_ns < w->t0_ns || b + w->v_rowj[v] * ldmin_ns < w->t0_ns)     // (a negative lower bound of the line delay)
      return bad("visual time (+ row * line delay) outside the spline");
    if (!std::isfinite(w->v_pi[2 * v]) || !std::isfinite(w->v_pi[2 * v + 1]) || !std::isfinite(w->v_pj[2 * v]) || !std::isfinite(w->v_pj[2 * v + 1]))
      return bad("non-finite visual observation");
  }
  for (int b = 0; b < w->NB; ++b)
    if (w->bc_i[b] < 0 || w->bc_i[b] >= w->F || w->bc_j[b] < 0 || w->bc_j[b] >= w->F) return bad("bias chain index out of range");
  if (w->pn > 0) {
    if (!w->pJ0 || !w->pr0 || !w->p_x0 || !w->p_kind || !w->p_index || !w->p_off) return bad("null prior pointer");
    // the kept blocks must tile the prior's columns exactly once (a hole would leave an unmapped column), and name each parameter block
    // at most once (Ceres refuses duplicate parameter blocks in one residual block; the store-semantics tail maps each unknown to ONE
    // prior column) -- so pn <= P
    std::vector<uint8_t> cover((size_t)w->pn, 0), seen((size_t)2 * w->K + 2 * w->F + 1, 0);
    for (int b = 0; b < w->pnb; ++b) {
      const int kind = w->p_kind[b], idx = w->p_index[b];
      const int lim = (kind <= CTVIO_PK_POS) ? w->K : (kind <= CTVIO_PK_BA ? w->F : 1);
      if (kind < 0 || kind > CTVIO_PK_LD || idx < 0 || idx >= lim || w->p_off[b] < 0 || w->p_off[b] + prior_block_size(kind) > w->pn)
        return bad("prior block out of range");
      const size_t slot = kind <= CTVIO_PK_POS ? (size_t)2 * idx + kind : (kind <= CTVIO_PK_BA ? (size_t)2 * w->K + 2 * idx + (kind - CTVIO_PK_BG) : seen.size() - 1);
      if (seen[slot]++) return bad("duplicate prior block (the same kind and index kept twice)");
      for (int k = 0; k < prior_block_size(kind); ++k)
        if (cover[w->p_off[b] + k]++) return bad("prior blocks overlap");
    }
    for (int i = 0; i < w->pn; ++i)
      if (!cover[i]) return bad("prior column not covered by any kept block");
  } else if (w->pnb != 0) {
    return bad("prior blocks without a prior");
  }
  return true;
}

// first pass: IMU samples sorted by (segment, bias state) and cut into groups, visual blocks sorted by frame pair (then rows)
// and cut into items of <= vch blocks -- only the orders and the counts are kept
inline void plan_window(const ctvio_window *w, int vch, PackTmp &t) {
  const int M = w->M, V = w->V;
  t.iseg.resize(M); t.iorder.resize(M);
  bool sorted = true;
  for (int i = 0; i < M; ++i) {
    t.iseg[i] = (int32_t)((w->imu_t[i] - w->t0_ns) / w->dt_ns);
    t.iorder[i] = i;
    if (i && (t.iseg[i] < t.iseg[i - 1] || (t.iseg[i] == t.iseg[i - 1] && w->imu_bias[i] < w->imu_bias[i - 1]))) sorted = false;
  }
  if (!sorted)
    std::stable_sort(t.iorder.begin(), t.iorder.end(), [&](int a, int b) {
      if (t.iseg[a] != t.iseg[b]) return t.iseg[a] < t.iseg[b];
      return w->imu_bias[a] < w->imu_bias[b];
    });
  t.ngrp = 0;
  for (int i = 0; i < M; ++i) {
    const int s = t.iorder[i];
    if (i == 0 || t.iseg[s] != t.iseg[t.iorder[i - 1]] || w->imu_bias[s] != w->imu_bias[t.iorder[i - 1]]) t.ngrp++;
  }
  t.vord.resize(V);
  std::iota(t.vord.begin(), t.vord.end(), 0);
  auto vless = [&](int a, int b) {
    if (w->v_ti[a] != w->v_ti[b]) return w->v_ti[a] < w->v_ti[b];
    if (w->v_tj[a] != w->v_tj[b]) return w->v_tj[a] < w->v_tj[b];
    if (w->v_rowi[a] != w->v_rowi[b]) return w->v_rowi[a] < w->v_rowi[b];
    return w->v_rowj[a] < w->v_rowj[b];
  };
  if (!std::is_sorted(t.vord.begin(), t.vord.end(), vless)) std::stable_sort(t.vord.begin(), t.vord.end(), vless);
  t.nvitem = 0;
  int cnt = 0;
  for (int i = 0; i < V; ++i) {
    const int v = t.vord[i];
    const bool fresh = (i == 0) || w->v_ti[v] != w->v_ti[t.vord[i - 1]] || w->v_tj[v] != w->v_tj[t.vord[i - 1]] || cnt >= vch;
    if (fresh) { t.nvitem++; cnt = 0; }
    cnt++;
  }
  // Anchors: the distinct i ends (landmark, t_i, row_i, p_i).  The reference adds every observation of a feature against the
  // feature's first one (trajectory_manager.cpp:367-383), i.e. one anchor per landmark; the C ABI takes arbitrary blocks, so a
  // landmark may own several (found by a linear search over the landmark's short list).  Numbered landmark-major.
  const int L = w->L;
  std::vector<int32_t> first((size_t)L, -1), next, rep, tmp_anc((size_t)V), acount;
  auto same_anchor = [&](int a, int b) {
    return w->v_ti[a] == w->v_ti[b] && w->v_rowi[a] == w->v_rowi[b] && w->v_pi[2 * a] == w->v_pi[2 * b] && w->v_pi[2 * a + 1] == w->v_pi[2 * b + 1];
  };
  std::vector<int32_t> lcount((size_t)L + 1, 0);
  for (int v = 0; v < V; ++v)   // (before the anchor search below: its per-landmark lists are linear, a malformed window must not make it quadratic)
    if (++lcount[w->v_lm[v]] > 64) { t.err = "more than 64 observations of one landmark"; return; }
  for (int i = 0; i < V; ++i) {
    const int v = t.vord[i], l = w->v_lm[v];
    int a = first[l], prev = -1;
    while (a >= 0 && !same_anchor(rep[a], v)) { prev = a; a = next[a]; }
    if (a < 0) {
      a = (int)rep.size();
      rep.push_back(v); next.push_back(-1); acount.push_back(0);
      if (prev < 0) first[l] = a; else next[prev] = a;
    }
    tmp_anc[v] = a;
    acount[a]++;
  }
  // Evaluation order: landmark-major (inside a landmark anchor by anchor, frame-pair order inside an anchor), so that the wave of
  // k_vis_eval that evaluates a landmark's blocks also forms its row of W.  A landmark never straddles a group of 64 slots (padding
  // slots in front of it); the window's slot count is a multiple of 64 (windows start on a wave boundary).
  t.A = (int)rep.size();
  t.anc_rep.resize((size_t)t.A);
  std::vector<int32_t> newid((size_t)t.A), astart((size_t)t.A);
  t.lm_slot.resize((size_t)L); t.lm_cnt.resize((size_t)L);
  int pos = 0, na = 0;
  for (int l = 0; l < L; ++l) {
    const int c = lcount[l];
    if ((pos & 63) + c > 64) pos = (pos + 63) & ~63;
    t.lm_slot[l] = pos; t.lm_cnt[l] = c;
    for (int a = first[l]; a >= 0; a = next[a]) {
      newid[a] = na; t.anc_rep[na] = rep[a]; astart[na] = pos;
      pos += acount[a];
      ++na;
    }
  }
  t.Vp = (pos + 63) & ~63;
  t.lord.assign((size_t)t.Vp, -1);
  t.vpos.resize(V);
  t.anc_of.resize(V);
  for (int i = 0; i < V; ++i) {     // frame-pair order inside an anchor
    const int v = t.vord[i], a = newid[tmp_anc[v]];
    const int slot = astart[a]++;
    t.lord[slot] = v;
    t.vpos[v] = slot;
    t.anc_of[v] = a;
  }
}

// The segment (first active knot) of an observation at line delay `ld`, exactly as the device computes it (kernels_visual.hpp: vis_times + clamp).
inline int vis_segment(const ctvio_window *w, int64_t t, int row, double ld) {
  const long long ld_ns = (long long)(ld * 1e9);
  const long long tau = (t - w->t0_ns) + (long long)row * ld_ns;
  const int s = (int)(tau / w->dt_ns);
  return std::max(0, std::min(s, w->K - 4));
}

// Sparsity plan of one window: what the reference leaves to SPARSE_NORMAL_CHOLESKY (trajectory_estimator.cpp:371-384) is decided here, once per
// upload, from the factor structure alone.
//   * Every landmark's KNOT SPAN [klo, khi]: the knots its residual blocks can touch (4 per spline end, image_feature_factor.h:79-101), over the
//     whole box of the line delay -- the row time t + row * ld moves with ld (image_feature_factor.h:72), and both extremes of a monotone
//     function bound it.  The rows of W are ordered by (klo, khi), landmarks without observations last.
//   * For every 16-column tile of the pose unknowns: the range of sorted rows that can be non-zero there (the Schur kernels multiply only those).
//   * The ENVELOPE of the reduced system S = Hpp - W^T Hll^-1 W: first[u] = the smallest unknown coupled to u by an IMU group (4 knots + its bias
//     state), a bias-chain link, the prior (all its columns mutually), or a landmark (its span's knots mutually, and each with the line delay);
//     Cholesky fill stays inside the row envelope, so tiles (r, c < env_first[r]) are never formed, stored or multiplied.  dense = true (batches
//     whose factorisation keeps the whole triangle in registers: P <= 223) sets env_first = 0 -- every tile is formed and loaded -- and leaves
//     the raw tile envelope in env_tile, by which k_cholesky_flow skips the PRODUCTS of empty tiles; full_ranges widens every non-empty row
//     range to all observed rows and drops the envelope (the dense cross-check).
inline void plan_sparsity(const ctvio_window *w, bool dense, bool full_ranges, PackTmp &t) {
  const int K = w->K, F = w->F, L = w->L, V = w->V, K6 = 6 * K, P = K6 + 6 * F + 1;
  std::vector<int32_t> klo((size_t)L, K), khi((size_t)L, -1);
  const double ld_a = w->fix_ld ? w->ld : w->ld_lo, ld_b = w->fix_ld ? w->ld : w->ld_hi;
  for (int v = 0; v < V; ++v) {
    const int l = w->v_lm[v];
    const int s[4] = {vis_segment(w, w->v_ti[v], w->v_rowi[v], ld_a), vis_segment(w, w->v_ti[v], w->v_rowi[v], ld_b),
                      vis_segment(w, w->v_tj[v], w->v_rowj[v], ld_a), vis_segment(w, w->v_tj[v], w->v_rowj[v], ld_b)};
    const int lo = std::min(std::min(s[0], s[1]), std::min(s[2], s[3])), hi = std::max(std::max(s[0], s[1]), std::max(s[2], s[3])) + 3;
    klo[l] = std::min(klo[l], lo); khi[l] = std::max(khi[l], hi);
  }
  t.lm_at.resize((size_t)L); t.lm_pos.resize((size_t)L); t.row_klo.resize((size_t)L); t.row_khi.resize((size_t)L);
  std::iota(t.lm_at.begin(), t.lm_at.end(), 0);
  std::stable_sort(t.lm_at.begin(), t.lm_at.end(), [&](int a, int b) { return klo[a] != klo[b] ? klo[a] < klo[b] : khi[a] < khi[b]; });
  t.Lobs = 0; t.max_span = 0;
  for (int r = 0; r < L; ++r) {
    const int l = t.lm_at[r];
    t.lm_pos[l] = r; t.row_klo[r] = klo[l]; t.row_khi[r] = khi[l];
    if (khi[l] >= 0) { t.Lobs = r + 1; t.max_span = std::max(t.max_span, khi[l] - klo[l] + 1); }
  }
  const int ntr = P / 16 + 1;
  t.ntr = ntr;
  t.tl_beg.assign((size_t)ntr, 0); t.tl_end.assign((size_t)ntr, 0); t.env_first.assign((size_t)ntr, 0); t.env_tile.assign((size_t)ntr, 0);
  for (int c = 0; c < ntr; ++c) {
    int beg = L, end = 0;
    if (16 * c < K6) {
      const int kf = 16 * c / 6, kl = std::min(16 * c + 15, K6 - 1) / 6;
      for (int r = 0; r < t.Lobs; ++r)
        if (t.row_klo[r] <= kl && t.row_khi[r] >= kf) { beg = std::min(beg, r); end = r + 1; }
    }
    if (16 * c <= P - 1 && P - 1 < 16 * c + 16 && t.Lobs > 0) { beg = 0; end = t.Lobs; }   // the line-delay column: every observed landmark
    if (end <= beg) beg = end = 0;
    if (full_ranges && end > 0) { beg = 0; end = t.Lobs; }     // (CTVIO_DENSE: the A/B switch -- every tile with products multiplies every row)
    t.tl_beg[c] = beg; t.tl_end[c] = end;
  }
  if (full_ranges) return;   // (CTVIO_DENSE: no envelope at all)
  // envelope, in columns: per knot block, per bias block, line delay
  std::vector<int32_t> fk((size_t)K), fb((size_t)F);
  for (int k = 0; k < K; ++k) fk[k] = 6 * k;
  for (int f = 0; f < F; ++f) fb[f] = K6 + 6 * f;
  int fld = P - 1;
  for (int i = 0; i < w->M; ++i) {
    const int s = t.iseg[i], b = w->imu_bias[i];
    for (int j = 1; j < 4; ++j) fk[s + j] = std::min(fk[s + j], 6 * s);
    fb[b] = std::min(fb[b], 6 * s);
  }
  for (int b = 0; b < w->NB; ++b) {
    const int i = std::min(w->bc_i[b], w->bc_j[b]), j = std::max(w->bc_i[b], w->bc_j[b]);
    fb[j] = std::min(fb[j], K6 + 6 * i);
  }
  for (int l = 0; l < L; ++l) {
    if (khi[l] < 0) continue;
    for (int k = klo[l] + 1; k <= khi[l]; ++k) fk[k] = std::min(fk[k], 6 * klo[l]);
    fld = std::min(fld, 6 * klo[l]);
  }
  if (w->pn > 0) {
    int m = P;
    auto col0 = [&](int b) {
      const int kind = w->p_kind[b], idx = w->p_index[b];
      return kind == CTVIO_PK_ROT ? 6 * idx : kind == CTVIO_PK_POS ? 6 * idx + 3 : kind == CTVIO_PK_BG ? K6 + 6 * idx : kind == CTVIO_PK_BA ? K6 + 6 * idx + 3 : P - 1;
    };
    for (int b = 0; b < w->pnb; ++b) m = std::min(m, col0(b));
    for (int b = 0; b < w->pnb; ++b) {
      const int kind = w->p_kind[b], idx = w->p_index[b];
      if (kind <= CTVIO_PK_POS) fk[idx] = std::min(fk[idx], m);
      else if (kind <= CTVIO_PK_BA) fb[idx] = std::min(fb[idx], m);
      else fld = std::min(fld, m);
    }
  }
  for (int r = 0; r < ntr; ++r) {
    int f = 16 * r;                                            // (a row's own diagonal entry)
    for (int u = 16 * r; u < std::min(16 * r + 16, P); ++u) f = std::min(f, u < K6 ? fk[u / 6] : (u < P - 1 ? fb[(u - K6) / 6] : fld));
    if (16 * r <= P && P < 16 * r + 16) f = 0;                 // the rhs row rides along as row P: dense
    // The panel Cholesky (k_cholesky_solve) works in 32-column panels: the envelope starts on a panel boundary (even tile column), and every
    // tile row reaches at least the panel before its own 32-row block (so that the next diagonal block always takes part in a panel's
    // trailing update: its look-ahead relies on that).  The tiles this adds hold zeros.
    int ft = f / 16;
    t.env_tile[r] = ft;                                        // the envelope as it is (k_cholesky_flow skips the products of empty tiles)
    if (r >= 2) ft = std::min(ft, 2 * (r / 2) - 2);
    t.env_first[r] = (dense || r < 2) ? 0 : (ft & ~1);
  }
}

// The walk of the order-fixed wide-window assembly (kernels_assemble.hpp: k_assemble_wide), after plan_window and plan_sparsity: the window's
// blocks as slots (window-relative), landmark rows in sorted order (t.lm_at), a landmark's blocks in slot order -- vrow[V]; row r's blocks are
// vrow[off[r] .. off[r + 1]), off[L + 1].  A tile walks the rows [tl_beg, tl_end) of both its row and its column tile: a contiguous stretch.
// Python mirror: packer.row_walk.
inline void plan_row_walk(const ctvio_window *w, const PackTmp &t, int32_t *vrow, int32_t *off) {
  const int L = w->L;
  std::vector<int32_t> next((size_t)L + 1, 0);
  for (int s = 0; s < t.Vp; ++s)
    if (t.lord[s] >= 0) next[t.lm_pos[w->v_lm[t.lord[s]]] + 1]++;
  for (int r = 0; r < L; ++r) next[r + 1] += next[r];
  for (int r = 0; r <= L; ++r) off[r] = next[r];
  for (int s = 0; s < t.Vp; ++s)      // (counting sort by row: slot order inside a row)
    if (t.lord[s] >= 0) vrow[next[t.lm_pos[w->v_lm[t.lord[s]]]]++] = s;
}

// The most 16-row tiles that take part in one 32-column panel of k_cholesky_solve, by the kernel's own rule (tile R0 + l below panel jb takes
// part iff env_first[R0 + l] <= jb / 16 + 1): the LDS slots its slot-indexed variant needs to stage every panel of the window without overflow.
// ef: plan_sparsity's env_first (P / 16 + 1 entries).  Python mirror: packer.chol_panel_slots.
inline int chol_panel_slots(const int32_t *ef, int P) {
  int best = 0;
  for (int jb = 0; jb < P; jb += 32) {
    const int r0 = std::min(jb + 32, P), ntile = (P - r0 + 1 + 15) / 16, R0 = r0 / 16;
    int n = 0;
    for (int l = 0; l < ntile; ++l) n += ef[std::min(R0 + l, P / 16)] <= jb / 16 + 1 ? 1 : 0;
    best = std::max(best, n);
  }
  return best;
}

// Unknowns of Ceres' reduced program: referenced by some residual block and not constant
// (trajectory_estimator.cpp:114-141, 236-245, 311-318).
inline void active_mask(const ctvio_window *w, const PackTmp &t, int P, const int32_t *pcol, uint8_t *act) {
  const int N = P + w->L, K = w->K;
  std::memset(act, 0, (size_t)N);
  for (int i = 0; i < w->M; ++i) {
    std::memset(act + 6 * t.iseg[i], 1, 24);
    std::memset(act + 6 * K + 6 * w->imu_bias[i], 1, 6);
  }
  const int64_t pad_ns = (int64_t)(0.039 * 1e9);  // AddImageFeatureDelayAnalytic spans [t, t + 0.039 s] (trajectory_estimator.cpp:299)
  for (int v = 0; v < w->V; ++v) {
    const int64_t tt[2] = {w->v_ti[v], w->v_tj[v]};
    for (int e = 0; e < 2; ++e) {
      const int s0 = (int)((tt[e] - w->t0_ns) / w->dt_ns), s1 = (int)((tt[e] + pad_ns - w->t0_ns) / w->dt_ns);
      for (int k = s0; k < s1 + 4 && k < K; ++k) std::memset(act + 6 * k, 1, 6);
    }
    act[P + w->v_lm[v]] = 1;
    act[P - 1] = 1;
  }
  for (int b = 0; b < w->NB; ++b) { std::memset(act + 6 * K + 6 * w->bc_i[b], 1, 6); std::memset(act + 6 * K + 6 * w->bc_j[b], 1, 6); }
  for (int i = 0; i < w->pn; ++i) act[pcol[i]] = 1;
  for (int k = 0; k <= w->fixed_upto && k < K; ++k) std::memset(act + 6 * k, 0, 6);
  if (w->knot_const)
    for (int k = 0; k < K; ++k) if (w->knot_const[k]) std::memset(act + 6 * k, 0, 6);
  for (int f = 0; f < w->F; ++f) {
    if (w->lock_bg) std::memset(act + 6 * K + 6 * f, 0, 3);
    if (w->lock_ba) std::memset(act + 6 * K + 6 * f + 3, 0, 3);
  }
  if (w->fix_ld) act[P - 1] = 0;
}

// ---------------------------------------------------------------------------------------- the batch: offsets, input arena, fill
// What the serial offset pass gathers about a batch: the totals the arenas are sized by and the maxima the launch list is chosen by.
struct BatchFacts {
  int32_t nw, K0, F0, L0, M0, V0, B0, U0, Pp0, pv0, pb, G0, I0, A0, TR0;   // sums over the windows (V0: block slots incl. padding)
  int64_t H0, W0, pH0;
  int32_t maxN, maxP, maxPn, maxL, maxLdw, maxK, maxK_lds, maxSpan, maxSchurTiles, maxSlots;   // maxK_lds: over the LDS-resident windows
  // (a window whose packed Hessian does not fit in LDS counts as "global" even without visual blocks -- e.g. an IMU-only predict of a
  // long spline: the store-semantics tail only finishes LDS-resident windows, so such a batch must take the accumulate path)
  bool any_vis_lds, any_vis_glb, all_imu;
  bool walk;                               // the row walk of the order-fixed wide-window assembly is uploaded (vrow, vrow_off)
  size_t vis_lds_bytes, vis_glb_bytes;     // dynamic LDS of the visual assembly kernels
  // the factorisation of the batch, set by the upload (the choice steers the planning: dense envelope, slot count)
  int32_t chol_tiles;
  bool chol_compact;
  size_t chol_lds;
};

// One segment of an arena layout: name, byte offset, the bytes a batch fills (CTVIO_POISON checks and poisons these extents); dbl: the
// segment holds doubles that may be poisoned (integer segments never are: they feed addresses).
struct ArenaSeg {
  const char *name;
  size_t off, bytes;
  bool dbl;
};
inline size_t arena_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// The layout of one per-call entry's scratch (ctvio.hip: call_io_ / call_scr_).  The call names every segment ONCE, in order: add(name,
// element size, count, dbl) gives 256-byte aligned offsets and bytes(), the total.  One reservation per call: after reserved() -- the
// caller's arena holds bytes() -- at<T>(base, segment) gives typed pointers and add() is refused (-1), as at() is before it (null): a grow
// frees the old block, and a pointer taken before it would be stale inside an already queued kernel.  A segment without elements costs
// nothing (it shares its offset with the next one).  Segments added after landing() exist in the pinned mirror only: dev_bytes() ends before them.
class CallLayout {
 public:
  int add(const char *name, size_t elem, size_t count, bool dbl) {
    if (reserved_) return -1;
    segs_.push_back(ArenaSeg{name, bytes_, elem * count, dbl});
    bytes_ += arena_align(elem * count);
    if (!landing_) dev_bytes_ = bytes_;
    return (int)segs_.size() - 1;
  }
  void landing() { landing_ = true; }
  void reserved() { reserved_ = true; }
  size_t bytes() const { return bytes_; }
  size_t dev_bytes() const { return dev_bytes_; }
  const std::vector<ArenaSeg> &segs() const { return segs_; }
  size_t off(int seg) const { return segs_[(size_t)seg].off; }
  template <class T> T *at(char *base, int seg) const {
    return reserved_ && base && seg >= 0 && seg < (int)segs_.size() ? reinterpret_cast<T *>(base + segs_[(size_t)seg].off) : nullptr;
  }

 private:
  std::vector<ArenaSeg> segs_;
  size_t bytes_ = 0, dev_bytes_ = 0;
  bool landing_ = false, reserved_ = false;
};

// The device-only scratch of a query entry that wants covariances (ctvio.hip: run_query): the call's activity mask and exclusions over the
// batch's unknowns, then one record of rec_bytes per query.  Without covariances (want false) every segment is empty.
struct CovScratch {
  CallLayout lay;
  int s_mask, s_excl, s_rec;
  CovScratch(bool want, size_t unknowns, size_t rec_bytes, size_t nrec)
      : s_mask(lay.add("mask", 1, want ? unknowns : 0, false)), s_excl(lay.add("excl", 1, want ? unknowns : 0, false)),
        s_rec(lay.add("records", rec_bytes, want ? nrec : 0, false)) {}
};

// The n queries of a per-call entry grouped by window: query i belongs to window `only` (only >= 0; win is not read) or to win[i].
// slot[r] is the caller's index of sorted query r; the sort is stable, so a window's queries keep the caller's order.
class QueryOrder {
 public:
  std::vector<int32_t> slot;
  QueryOrder(int only, int n, const int32_t *win, int nwin) : slot((size_t)std::max(n, 0)), only_(only), win_(win) {
    std::iota(slot.begin(), slot.end(), 0);
    if (only >= 0) return;
    for (int i = 0; i < n && bad_ < 0; ++i)
      if (win[i] < 0 || win[i] >= nwin) bad_ = i;
    if (bad_ < 0) std::stable_sort(slot.begin(), slot.end(), [&](int32_t a, int32_t b) { return win[a] < win[b]; });
  }
  // empty, or the complaint about the first query whose window id lies outside [0, nwin): nothing below may be used then
  std::string error() const { return bad_ < 0 ? std::string() : "query " + std::to_string(bad_) + ": window id out of range"; }
  int win_of(int r) const { return only_ >= 0 ? only_ : win_[slot[(size_t)r]]; }
  // the sorted queries cut into runs of at most per_tile consecutive queries of one window, in order: emit(window, first, count)
  template <class F> void runs(int per_tile, F &&emit) const {
    const int n = (int)slot.size();
    for (int r = 0; r < n;) {
      int cnt = 1;
      while (cnt < per_tile && r + cnt < n && win_of(r + cnt) == win_of(r)) ++cnt;
      emit(win_of(r), r, cnt);
      r += cnt;
    }
  }

 private:
  int only_, bad_ = -1;
  const int32_t *win_;
};

// The statuses a query entry reports share these values (ctvio.h; ctvio.hip asserts it of every enum of kernels_cov.hpp): 1 is the
// host's -- the window's factorisation met a bad pivot (Lm::chol_fail) --, 2 "no information" (an untouched knot or bias state).
enum { QUERY_OK = 0, QUERY_SINGULAR = 1, QUERY_NO_INFO = 2 };
inline int merge_status(int st, bool chol_fail) { return st == QUERY_OK && chol_fail ? (int)QUERY_SINGULAR : st; }
// The dim x dim covariance block (row-major) of a query whose status is not QUERY_OK: no information gives +inf on the diagonal and 0
// elsewhere, every other status NaN.
inline void fill_not_ok(double *o, int dim, int st) {
  const double inf = std::numeric_limits<double>::infinity();
  for (int e = 0; e < dim * dim; ++e) o[e] = st == QUERY_NO_INFO ? (e % (dim + 1) == 0 ? inf : 0.0) : std::nan("");
}
// the caller's block o by status: the block `computed` the kernel left, or the fill
inline void cov_block(double *o, const double *computed, int dim, int st) {
  if (st == QUERY_OK) std::memcpy(o, computed, sizeof(double) * (size_t)dim * dim);
  else fill_not_ok(o, dim, st);
}
// the caller's gate by status, likewise: no information gates nothing
inline double gate_value(double computed, int st) { return st == QUERY_OK ? computed : (st == QUERY_NO_INFO ? 0.0 : std::nan("")); }

// The statuses of a leave-one-out gate (ctvio_visual_gate_batch, ctvio_imu_gate_batch): ok, singular and no_info are QUERY_*'s (ctvio.hip
// asserts it), weak is "redundancy < min_redundancy".
struct GateCodes { int ok, weak, singular, no_info, inactive = -1; };   // inactive (the visual gate alone): an ok block that is switched off -- values as for ok
// One block or sample of a gate by status, into the caller's entries (null: not asked for; the computed values are read only where one
// is).  st: what the kernels left; bad: the window's factorisation failed (Lm::chol_fail), which turns ok and weak into singular and lets
// every other status stand.  The redundancy is the computed one for ok and weak, 0 without information, NaN otherwise; the dim x dim block
// and the gate are cov_block's and gate_value's with weak counted as no information.  Returns the status to report.
inline int gate_scatter(const GateCodes &c, int st, bool bad, int dim, const double *computed_red, const double *computed_cov, const double *computed_chi2,
                        double *red, double *cov, double *chi2) {
  if (bad && (st == c.ok || st == c.weak || st == c.inactive)) st = c.singular;
  const int as = st == c.weak ? c.no_info : (st == c.inactive ? c.ok : st);
  if (red) *red = st == c.ok || st == c.weak || st == c.inactive ? *computed_red : (st == c.no_info ? 0.0 : std::nan(""));
  if (cov) cov_block(cov, computed_cov, dim, as);
  if (chi2) *chi2 = gate_value(*computed_chi2, as);
  return st;
}

// The 2^30 bound every per-call entry puts on a count of queries.
inline bool check_count(int64_t n64) { return n64 >= 0 && n64 <= (int64_t)1 << 30; }
// Whether the bias state of query i (frame null: the newest, always there) lies in [0, F) of its window; otherwise err is the complaint,
// `what` being "query" or "prediction".
inline bool check_frame(const int32_t *frame, int64_t i, int F, const char *what, std::string &err) {
  if (!frame || (frame[i] >= 0 && frame[i] < F)) return true;
  err = std::string(what) + " " + std::to_string(i) + ": bias state out of range";
  return false;
}

// The IMU sample streams of ctvio_imu_predict_batch and ctvio_predict_landmarks_batch: query i (the caller's order) owns n_imu[i]
// consecutive samples of imu_t / imu_gyro / imu_acc.  noise() and streams() validate -- false: `error` says why --, then add() names the
// three io segments (among the call's inputs) and stage() fills them.
struct ImuSamples {
  std::vector<int64_t> first;   // the first sample of every query, and behind them ns, the number of samples
  size_t ns = 0;
  int s_t = -1, s_gyro = -1, s_acc = -1;
  std::string error;
  bool noise(const ctvio_imu_noise &nz) {
    for (double x : {nz.gyr_n, nz.acc_n, nz.gyr_w, nz.acc_w})
      if (!(x >= 0.0) || !std::isfinite(x)) { error = "a noise sigma is negative or not finite"; return false; }
    return true;
  }
  // per query, in this order: the bias state (check_frame against meta[window].F), 1 to 4096 samples, strictly increasing times, finite
  // measurements; then at most 2^30 samples in the call.  what: "query" or "prediction".
  bool streams(const char *what, int only, int n, const int32_t *win, const int32_t *frame, const WinMeta *meta, const int32_t *n_imu, const int64_t *imu_t,
               const double *imu_gyro, const double *imu_acc) {
    first.assign((size_t)n + 1, 0);
    t_ = imu_t; gyro_ = imu_gyro; acc_ = imu_acc;
    for (int i = 0; i < n; ++i) {
      if (!check_frame(frame, i, meta[only >= 0 ? only : win[i]].F, what, error)) return false;
      const std::string q = std::string(what) + " " + std::to_string(i);
      if (n_imu[i] < 1 || n_imu[i] > 4096) { error = q + ": 1 to 4096 samples"; return false; }
      const int64_t b = first[(size_t)i], e = b + n_imu[i];
      first[(size_t)i + 1] = e;
      for (int64_t j = b; j < e; ++j) {
        if (j > b && imu_t[j] <= imu_t[j - 1]) { error = q + ": sample times not strictly increasing"; return false; }
        for (int c = 0; c < 3; ++c)
          if (!std::isfinite(imu_gyro[3 * j + c]) || !std::isfinite(imu_acc[3 * j + c])) { error = q + ": a measurement is not finite"; return false; }
      }
    }
    ns = (size_t)first[(size_t)n];
    if (ns > (size_t)1 << 30) { error = "more than 2^30 samples in one call"; return false; }
    return true;
  }
  void add(CallLayout &io) {
    s_t = io.add("imu_t", sizeof(int64_t), ns, false);
    s_gyro = io.add("imu_gyro", sizeof(double), 3 * ns, false);
    s_acc = io.add("imu_acc", sizeof(double), 3 * ns, false);
  }
  void stage(const CallLayout &io, char *host) const {
    std::memcpy(io.at<int64_t>(host, s_t), t_, sizeof(int64_t) * ns);
    std::memcpy(io.at<double>(host, s_gyro), gyro_, sizeof(double) * 3 * ns);
    std::memcpy(io.at<double>(host, s_acc), acc_, sizeof(double) * 3 * ns);
  }

 private:
  const int64_t *t_ = nullptr;
  const double *gyro_ = nullptr, *acc_ = nullptr;
};

// ctvio_visual_gate_batch writes one record per block slot (kernels_cov.hpp: GateRec, about 0.9 KB) and a large batch holds 10^6 of them, so
// the records of a call live in a scratch of bounded size and the windows are walked in slices.  GATE_SLICE_SLOTS: 65536 slots, 57 MB of
// records -- 8192 tiles of k_cov_solve per slice, four times what the 256 CUs of an MI355X hold at eight workgroups each, so a slice still
// fills the device and its two launches (a few microseconds) are noise against the substitution; and small against HBM, which the
// batch's normal equations already share.
constexpr size_t GATE_SLICE_SLOTS = 65536;
struct GateSlice { int32_t wbeg, wend; int64_t slots; };   // windows [wbeg, wend) and their block slots (padding included)
// The slices of windows [wbeg, wend) with slots[w] block slots each: consecutive whole windows, as many as stay within `budget` slots; a
// window beyond the budget is alone in its slice; a window without slots rides with its predecessor (with its successor at the very
// beginning).  Every window is in exactly one slice, in order; no slice is empty of windows.
inline std::vector<GateSlice> plan_gate_slices(const int32_t *slots, int wbeg, int wend, size_t budget) {
  std::vector<GateSlice> out;
  for (int w = wbeg; w < wend; ++w) {
    const int64_t n = slots[w];
    if (out.empty() || (n > 0 && out.back().slots > 0 && (size_t)(out.back().slots + n) > budget)) out.push_back(GateSlice{w, w + 1, n});
    else { out.back().wend = w + 1; out.back().slots += n; }
  }
  return out;
}

// ctvio_imu_gate_batch walks its windows in the same slices, counted in packed IMU samples (slots[w] = M_w; nothing pads them).  One record
// per sample (kernels_cov.hpp: ImuGateRec): 16 bytes of header, the 6 doubles of the residual and the 24 x 6 Jacobian block, 1216 bytes.
// IMU_GATE_SLICE_SAMPLES: 49152 samples x 1216 B = 59.8 MB of records, within the 64 MB the visual gate's records were held to -- 24576
// tiles of two samples per slice, twelve times what the 256 CUs of an MI355X hold at eight workgroups each.
constexpr size_t IMU_GATE_SLICE_SAMPLES = 49152;
// The absolute packed slot of every sample of a window in the caller's order: the upload sorts the samples by (segment, bias state)
// (PackTmp::iorder[i] = the caller's sample in packed position i), the slots of the window start at imu0.
inline void imu_slot_map(const int32_t *iorder, int M, int32_t imu0, int32_t *slot) {
  for (int i = 0; i < M; ++i) slot[iorder[i]] = imu0 + i;
}
// The tile descriptors of one slice: the first tile of every window [wbeg, wend) when each window's samples[w] packed samples are cut into
// tiles of per_tile consecutive ones that never straddle a window, and behind them the slice's tile count.  A window without samples has no
// tile: its entry equals its successor's.
inline std::vector<int32_t> plan_imugate_tiles(const int32_t *samples, int wbeg, int wend, int per_tile) {
  std::vector<int32_t> first((size_t)(wend - wbeg) + 1, 0);
  for (int w = wbeg; w < wend; ++w) first[(size_t)(w - wbeg) + 1] = first[(size_t)(w - wbeg)] + (samples[w] + per_tile - 1) / per_tile;
  return first;
}

// The input arena (pinned host mirror + device), every segment ONCE: X(element type, segment, Dev member, allocated count, filled count).
// An empty set keeps one entry allocated.  The names stand for BatchFacts members (layout_input).  Irregular: `state` is the contiguous
// block quat | pos | bias | rho | ld (StatePtrs); vrow / vrow_off hold one unused entry unless the row walk is uploaded, and Dev gets null.
#define CTV_INPUT_SEGMENTS(X)                                                                          \
  X(WinMeta, meta, wins, nw, nw)                                                                       \
  X(double, state, quat, 7 * K0 + 6 * F0 + L0 + nw, 7 * K0 + 6 * F0 + L0 + nw)                         \
  X(int32_t, knot_win, knot_win, K0, K0) X(int32_t, bias_win, bias_win, F0, F0) X(int32_t, lm_win, lm_win, L0, L0) \
  X(ImuGroup, groups, groups, G0, G0) X(int32_t, imu_grp, imu_grp, Mt, M0)                             \
  X(double, imu_u, imu_u, Mt, M0) X(double, imu_meas, imu_meas, 6 * Mt, 6 * M0)                        \
  X(int32_t, v_win, v_win, Vt, V0) X(int32_t, v_lm, v_lm, Vt, V0) X(int32_t, v_anc, v_anc, Vt, V0) X(int32_t, v_rowj, v_rowj, Vt, V0) \
  X(int64_t, v_tj, v_tj, Vt, V0) X(double, v_obs, v_obs, 2 * Vt, 2 * V0)                               \
  X(double, v_cauchy, v_cauchy, Vt, V0) X(uint8_t, v_on, v_on, Vt, V0) X(int32_t, vb_win, vb_win, Vt / 64 + 1, V0 / 64) \
  X(int32_t, a_win, a_win, At, A0) X(int32_t, a_lm, a_lm, At, A0) X(int32_t, a_row, a_row, At, A0)     \
  X(int64_t, a_t, a_t, At, A0) X(double, a_obs, a_obs, 2 * At, 2 * A0)                                 \
  X(VisItem, vitems, vitems, std::max<size_t>(I0, 1), I0) X(int32_t, vblk, vblk, Vt, V0) X(int32_t, vblk_anc, vblk_anc, Vt, V0) \
  X(int32_t, bc_win, bc_win, B0, B0) X(int32_t, bc_i, bc_i, B0, B0) X(int32_t, bc_j, bc_j, B0, B0) X(double, bc_w, bc_w, 6 * B0, 6 * B0) \
  X(double, pJ0, pJ0, pH0, pH0) X(double, pr0, pr0, pv0, pv0)                                          \
  X(double, pH, pH, pH0, pH0) X(double, pb0, pb0, pv0, pv0) X(double, pc0, pc0, nw, nw) X(double, p_x0, p_x0, 4 * pb, 4 * pb) \
  X(int32_t, pcol, pcol, pv0, pv0) X(int32_t, p_kind, p_kind, pb, pb) X(int32_t, p_index, p_index, pb, pb) X(int32_t, p_off, p_off, pb, pb) \
  X(int32_t, pinv, pinv, Pp0, Pp0) X(int32_t, bgl_off, bgl_off, F0 + nw, F0 + nw) X(int32_t, bgl, bgl, std::max<size_t>(G0, 1), G0) \
  X(uint8_t, active, active, U0, U0)                                                                   \
  X(int32_t, lm_pos, lm_pos, L0, L0) X(int32_t, lm_at, lm_at, L0, L0) X(int32_t, lm_klo, lm_klo, L0, L0) X(int32_t, lm_khi, lm_khi, L0, L0) \
  X(int32_t, lm_vfirst, lm_vfirst, L0, L0) X(int32_t, lm_vcnt, lm_vcnt, L0, L0)                        \
  X(int32_t, tl_beg, tl_beg, TR0, TR0) X(int32_t, tl_end, tl_end, TR0, TR0) X(int32_t, env_first, env_first, TR0, TR0) X(int32_t, env_tile, env_tile, TR0, TR0) \
  /* the walk of the order-fixed wide-window assembly (deterministic = 2 with a window beyond the LDS-resident Hessian; else not uploaded) */ \
  X(int32_t, vrow, vrow, walk ? Vt : 1, walk ? V0 : 0) X(int32_t, vrow_off, vrow_off, walk ? L0 + nw : 1, walk ? L0 + nw : 0)

#define CTV_X(type, name, member, alloc, used) +1
constexpr int INPUT_NSEG = 0 CTV_INPUT_SEGMENTS(CTV_X);
#undef CTV_X

// One typed pointer per input segment: into the host mirror (the packer fills these) or into the device arena (Dev gets these).
struct InputPtrs {
#define CTV_X(type, name, member, alloc, used) type *name;
  CTV_INPUT_SEGMENTS(CTV_X)
#undef CTV_X
};
// The contiguous state block quat | pos | bias | rho | ld of a batch (the input segment `state`; cstate and snap in the work arena).
struct StatePtrs {
  double *quat, *pos, *bias, *rho, *ld;
  StatePtrs(double *p, const BatchFacts &b) : quat(p), pos(quat + (size_t)4 * b.K0), bias(pos + (size_t)3 * b.K0), rho(bias + (size_t)6 * b.F0), ld(rho + b.L0) {}
};

struct InputLayout {
  ArenaSeg segs[INPUT_NSEG];   // in list order (the extents of the segments, named, without their alignment tails)
  size_t bytes;
  InputPtrs at(char *base) const {
    InputPtrs p;
    int i = 0;
#define CTV_X(type, name, member, alloc, used) p.name = reinterpret_cast<type *>(base + segs[i++].off);
    CTV_INPUT_SEGMENTS(CTV_X)
#undef CTV_X
    return p;
  }
};
inline InputLayout layout_input(const BatchFacts &b) {
  const size_t nw = b.nw, K0 = b.K0, F0 = b.F0, L0 = b.L0, M0 = b.M0, V0 = b.V0, B0 = b.B0, U0 = b.U0, Pp0 = b.Pp0, pv0 = b.pv0, pb = b.pb, G0 = b.G0,
               I0 = b.I0, A0 = b.A0, TR0 = b.TR0, pH0 = (size_t)b.pH0;
  const size_t Mt = std::max<size_t>(M0, 1), Vt = std::max<size_t>(V0, 1), At = std::max<size_t>(A0, 1);
  const bool walk = b.walk;
  InputLayout l;
  size_t off = 0;
  int i = 0;
#define CTV_X(type, name, member, alloc, used)                                    \
  l.segs[i++] = ArenaSeg{#name, off, sizeof(type) * (size_t)(used), false};       \
  off += arena_align(sizeof(type) * (size_t)(alloc));
  CTV_INPUT_SEGMENTS(CTV_X)
#undef CTV_X
  l.bytes = off;
  return l;
}

// The serial offset pass (prefix sums) after the planning: every window's WinMeta and relative time origin, and the batch's facts.
// need_slots: the batch takes the slot-indexed panel Cholesky (its slot count is gathered); vis_stage: the staging bytes of the visual
// assembly beside its LDS Hessian (kernels_assemble.hpp: vis_stage_bytes); wide_walk: deterministic = 2 (a batch with a window beyond
// the LDS-resident Hessian then uploads the row walk).
inline BatchFacts batch_offsets(const std::vector<const ctvio_window *> &wins, const std::vector<PackTmp> &tmp, bool need_slots, size_t vis_stage,
                                bool wide_walk, std::vector<WinMeta> &meta, std::vector<int64_t> &t0) {
  const int nw = (int)wins.size();
  meta.assign(nw, WinMeta());
  t0.resize(nw);
  BatchFacts b;
  std::memset(&b, 0, sizeof b);
  b.nw = nw; b.maxSpan = 1;
  b.vis_lds_bytes = b.vis_glb_bytes = vis_stage;
  b.all_imu = nw > 0;
  for (int wi = 0; wi < nw; ++wi) {
    const ctvio_window &w = *wins[wi];
    WinMeta &m = meta[wi];
    t0[wi] = w.t0_ns;
    m.K = w.K; m.F = w.F; m.L = w.L; m.M = w.M; m.NB = w.NB; m.V = w.V;
    m.P = 6 * w.K + 6 * w.F + 1; m.N = m.P + w.L; m.pn = w.pn; m.pnb = w.pnb;
    m.knot0 = b.K0; m.bias0 = b.F0; m.lm0 = b.L0; m.imu0 = b.M0; m.vis0 = b.V0; m.bc0 = b.B0; m.u0 = b.U0; m.p0 = b.Pp0;
    m.grp0 = b.G0; m.ngrp = tmp[wi].ngrp; m.vitem0 = b.I0; m.nvitem = tmp[wi].nvitem; m.Vp = tmp[wi].Vp;
    m.anc0 = b.A0; m.A = tmp[wi].A;
    m.tr0 = b.TR0; m.ntr = tmp[wi].ntr; m.Lobs = tmp[wi].Lobs; b.TR0 += tmp[wi].ntr; b.maxSpan = std::max(b.maxSpan, tmp[wi].max_span);
    m.ldw = (m.P + 1 + 31) / 32 * 32; m.Lpad = std::max(2, (w.L + 1) / 2 * 2);
    m.pv0 = b.pv0; m.pblk0 = b.pb; m.fix_ld = w.fix_ld; m.lock_bg = w.lock_bg; m.lock_ba = w.lock_ba; m.fixed_upto = w.fixed_upto;
    m.H0 = b.H0; m.W0 = b.W0; m.pH0 = b.pH0; m.ldh = (m.P + 15) / 16 * 16; m.dt_ns = w.dt_ns; m.inv_dt = 1e9 / (double)w.dt_ns;
    for (int i = 0; i < 4; ++i) m.q_CI[i] = w.q_CI[i];
    for (int i = 0; i < 3; ++i) { m.p_CI[i] = w.p_CI[i]; m.gravity[i] = w.gravity[i]; }
    for (int i = 0; i < 6; ++i) m.imu_w[i] = w.imu_w[i];
    m.img_w = w.img_w; m.cauchy_a = w.cauchy_a; m.ld_lo = w.ld_lo; m.ld_hi = w.ld_hi;
    {
      const size_t K6 = 6 * (size_t)w.K, nG = K6 + 1, nH = K6 * (K6 + 1) / 2 + K6 + 1 + nG;
      const size_t need = ((nH + 3) & ~(size_t)3) * sizeof(double) + 32 + vis_stage;   // fp64 accumulators in LDS
      const size_t need_glb = ((nG + 3) & ~(size_t)3) * sizeof(double) + 16 + vis_stage;
      m.vis_lds = need <= 160 * 1024 ? 1 : 0;
      if (m.vis_lds) { b.any_vis_lds = true; b.maxK_lds = std::max(b.maxK_lds, w.K); } else b.any_vis_glb = true;
      b.vis_lds_bytes = std::max(b.vis_lds_bytes, m.vis_lds ? need : need_glb);
      b.vis_glb_bytes = std::max(b.vis_glb_bytes, need_glb);
    }
    if (m.ngrp == 0) b.all_imu = false;
    b.K0 += w.K; b.F0 += w.F; b.L0 += w.L; b.M0 += w.M; b.V0 += m.Vp; b.B0 += w.NB; b.U0 += m.N; b.Pp0 += m.P; b.pv0 += w.pn; b.pb += w.pnb;
    b.G0 += m.ngrp; b.I0 += m.nvitem; b.A0 += m.A;
    b.H0 += (int64_t)m.P * m.ldh; b.W0 += (int64_t)m.Lpad * m.ldw; b.pH0 += (int64_t)w.pn * w.pn;
    b.maxN = std::max(b.maxN, m.N); b.maxP = std::max(b.maxP, m.P); b.maxPn = std::max(b.maxPn, w.pn);
    b.maxL = std::max(b.maxL, m.L); b.maxLdw = std::max(b.maxLdw, m.ldw); b.maxK = std::max(b.maxK, m.K);
    if (need_slots) b.maxSlots = std::max(b.maxSlots, chol_panel_slots(tmp[wi].env_first.data(), m.P));
    {   // 16 x 16 tiles of the reduced system that receive Schur products (k_schur_window_f64): knot columns, line delay, rhs row
      const int ntl = m.ldw / 16, K6 = 6 * m.K;
      int cnt = 0;
      for (int ti = 0; ti < ntl; ++ti)
        for (int tj = 0; tj <= ti; ++tj) {
          const bool nzr = (16 * ti < K6) || (m.P >= 16 * ti && m.P - 1 < 16 * ti + 16);
          const bool nzc = (16 * tj < K6) || (m.P - 1 >= 16 * tj && m.P - 1 < 16 * tj + 16);
          cnt += (nzr && nzc) ? 1 : 0;
        }
      b.maxSchurTiles = std::max(b.maxSchurTiles, cnt);
    }
  }
  b.walk = wide_walk && b.any_vis_glb;
  return b;
}

// Second pass: window wi fills its own slices of every input segment (h: the host mirror's pointers).
inline void fill_window(const ctvio_window &w, int wi, const WinMeta &m, const PackTmp &t, const BatchFacts &b, const InputPtrs &h, int vch) {
  const size_t Mt = (size_t)std::max(b.M0, 1), Vt = (size_t)std::max(b.V0, 1), At = (size_t)std::max(b.A0, 1);
  const StatePtrs st(h.state, b);
  std::memcpy(st.quat + (size_t)4 * m.knot0, w.quat, sizeof(double) * 4 * w.K);
  std::memcpy(st.pos + (size_t)3 * m.knot0, w.pos, sizeof(double) * 3 * w.K);
  std::memcpy(st.bias + (size_t)6 * m.bias0, w.bias, sizeof(double) * 6 * w.F);
  if (w.L) std::memcpy(st.rho + m.lm0, w.rho, sizeof(double) * w.L);
  st.ld[wi] = w.fix_ld ? w.ld : std::min(std::max(w.ld, w.ld_lo), w.ld_hi);   // Ceres IterationZero: project on the feasible set
  std::fill(h.knot_win + m.knot0, h.knot_win + m.knot0 + w.K, wi);
  std::fill(h.bias_win + m.bias0, h.bias_win + m.bias0 + w.F, wi);
  std::fill(h.lm_win + m.lm0, h.lm_win + m.lm0 + w.L, wi);
  if (w.L) {   // sparsity plan: rows of W in sorted landmark order and their knot spans
    std::memcpy(h.lm_pos + m.lm0, t.lm_pos.data(), 4 * (size_t)w.L); std::memcpy(h.lm_at + m.lm0, t.lm_at.data(), 4 * (size_t)w.L);
    std::memcpy(h.lm_klo + m.lm0, t.row_klo.data(), 4 * (size_t)w.L); std::memcpy(h.lm_khi + m.lm0, t.row_khi.data(), 4 * (size_t)w.L);
    for (int l = 0; l < w.L; ++l) { h.lm_vfirst[m.lm0 + l] = m.vis0 + t.lm_slot[l]; h.lm_vcnt[m.lm0 + l] = t.lm_cnt[l]; }
  }
  std::memcpy(h.tl_beg + m.tr0, t.tl_beg.data(), 4 * (size_t)m.ntr); std::memcpy(h.tl_end + m.tr0, t.tl_end.data(), 4 * (size_t)m.ntr);
  std::memcpy(h.env_first + m.tr0, t.env_first.data(), 4 * (size_t)m.ntr); std::memcpy(h.env_tile + m.tr0, t.env_tile.data(), 4 * (size_t)m.ntr);
  if (b.walk) {
    plan_row_walk(&w, t, h.vrow + m.vis0, h.vrow_off + m.lm0 + wi);
    std::fill(h.vrow + m.vis0 + w.V, h.vrow + m.vis0 + m.Vp, 0);   // (unused tail of the window's list)
  }
  // IMU samples in (segment, bias) order; groups = runs of equal (segment, bias)
  int g = m.grp0 - 1;
  for (int i = 0; i < w.M; ++i) {
    const int src = t.iorder[i];
    if (i == 0 || t.iseg[src] != t.iseg[t.iorder[i - 1]] || w.imu_bias[src] != w.imu_bias[t.iorder[i - 1]])
      h.groups[++g] = ImuGroup{wi, t.iseg[src], w.imu_bias[src], i, 0, m.knot0 + t.iseg[src], m.bias0 + w.imu_bias[src], m.imu0 + i};
    h.groups[g].count++;
    const size_t e = (size_t)m.imu0 + i;
    h.imu_grp[e] = g;
    const int64_t st_ns = w.imu_t[src] - w.t0_ns;
    const double uu = (double)(st_ns % w.dt_ns) / (double)w.dt_ns;
    h.imu_u[e] = uu;
    for (int c = 0; c < 3; ++c) {
      h.imu_meas[(size_t)c * Mt + e] = w.imu_gyro[3 * src + c];
      h.imu_meas[(size_t)(3 + c) * Mt + e] = w.imu_acc[3 * src + c];
    }
  }
  // anchors (the i ends, landmark-major) and visual blocks: evaluation slots in landmark-major order (padding slots: window -1,
  // harmless values)
  for (int a = 0; a < m.A; ++a) {
    const int v = t.anc_rep[a];
    const size_t e = (size_t)m.anc0 + a;
    h.a_win[e] = wi; h.a_lm[e] = w.v_lm[v]; h.a_row[e] = w.v_rowi[v]; h.a_t[e] = w.v_ti[v] - w.t0_ns;
    h.a_obs[e] = w.v_pi[2 * v]; h.a_obs[At + e] = w.v_pi[2 * v + 1];
  }
  std::fill(h.vb_win + m.vis0 / 64, h.vb_win + (m.vis0 + m.Vp) / 64, wi);
  for (int i = 0; i < m.Vp; ++i) {
    const int v = t.lord[i];
    const size_t e = (size_t)m.vis0 + i;
    h.v_on[e] = 1;   // (every block is active after an upload; a padding slot's flag is never read)
    if (v < 0) {
      h.v_win[e] = -1; h.v_lm[e] = 0; h.v_anc[e] = m.anc0; h.v_tj[e] = 0; h.v_rowj[e] = 0; h.v_cauchy[e] = 0.0;
      for (int c = 0; c < 2; ++c) h.v_obs[(size_t)c * Vt + e] = 0.0;
      continue;
    }
    h.v_win[e] = wi; h.v_lm[e] = w.v_lm[v]; h.v_anc[e] = m.anc0 + t.anc_of[v];
    h.v_tj[e] = w.v_tj[v] - w.t0_ns;
    h.v_rowj[e] = w.v_rowj[v];
    h.v_obs[e] = w.v_pj[2 * v]; h.v_obs[Vt + e] = w.v_pj[2 * v + 1];
    h.v_cauchy[e] = w.v_cauchy ? w.v_cauchy[v] : w.cauchy_a;
  }
  // the assembly's items: <= vch blocks of one frame pair, frame-pair order, as lists of slots (vblk)
  int it = m.vitem0 - 1;
  for (int i = 0; i < w.V; ++i) {
    const int v = t.vord[i];
    const bool fresh = (i == 0) || w.v_ti[v] != w.v_ti[t.vord[i - 1]] || w.v_tj[v] != w.v_tj[t.vord[i - 1]] || h.vitems[it].count >= vch;
    if (fresh) h.vitems[++it] = VisItem{m.vis0 + i, 0};
    h.vitems[it].count++;
    h.vblk[(size_t)m.vis0 + i] = m.vis0 + t.vpos[v];
    h.vblk_anc[(size_t)m.vis0 + i] = m.anc0 + t.anc_of[v];
  }
  for (int i = w.V; i < m.Vp; ++i) { h.vblk[(size_t)m.vis0 + i] = m.vis0; h.vblk_anc[(size_t)m.vis0 + i] = m.anc0; }   // (unused tail of the window's list)
  for (int k = 0; k < w.NB; ++k) { h.bc_win[m.bc0 + k] = wi; h.bc_i[m.bc0 + k] = w.bc_i[k]; h.bc_j[m.bc0 + k] = w.bc_j[k]; }
  if (w.NB) std::memcpy(h.bc_w + (size_t)6 * m.bc0, w.bc_w, sizeof(double) * 6 * w.NB);
  // prior: J0^T J0 (row-major n*n), J0^T r0, r0^T r0 in fp64; J0 is column-major (Eigen)
  const int n = w.pn;
  h.pc0[wi] = 0.0;
  int32_t *col = h.pcol + m.pv0;
  if (n > 0) {
    for (int k = 0; k < w.pnb; ++k) {
      const int kind = w.p_kind[k], idx = w.p_index[k];
      int u0 = 0;
      switch (kind) {
        case CTVIO_PK_ROT: u0 = 6 * idx; break;
        case CTVIO_PK_POS: u0 = 6 * idx + 3; break;
        case CTVIO_PK_BG: u0 = 6 * w.K + 6 * idx; break;
        case CTVIO_PK_BA: u0 = 6 * w.K + 6 * idx + 3; break;
        default: u0 = m.P - 1;
      }
      for (int c = 0; c < prior_block_size(kind); ++c) col[w.p_off[k] + c] = u0 + c;
    }
    double *pH = h.pH + m.pH0, *pb0 = h.pb0 + m.pv0;
    std::memcpy(h.pJ0 + m.pH0, w.pJ0, sizeof(double) * (size_t)n * n);
    std::memcpy(h.pr0 + m.pv0, w.pr0, sizeof(double) * (size_t)n);
    for (int i = 0; i < n; ++i) {
      const double *Ji = w.pJ0 + (size_t)i * n;
      double bi = 0;
      for (int r = 0; r < n; ++r) bi += Ji[r] * w.pr0[r];
      pb0[i] = bi;
      for (int j = 0; j <= i; ++j) {
        const double *Jj = w.pJ0 + (size_t)j * n;
        double s = 0;
        for (int r = 0; r < n; ++r) s += Ji[r] * Jj[r];
        pH[(size_t)i * n + j] = s; pH[(size_t)j * n + i] = s;
      }
    }
    double c0 = 0;
    for (int r = 0; r < n; ++r) c0 += w.pr0[r] * w.pr0[r];
    h.pc0[wi] = c0;
    std::memcpy(h.p_kind + m.pblk0, w.p_kind, 4 * (size_t)w.pnb); std::memcpy(h.p_index + m.pblk0, w.p_index, 4 * (size_t)w.pnb);
    std::memcpy(h.p_off + m.pblk0, w.p_off, 4 * (size_t)w.pnb); std::memcpy(h.p_x0 + (size_t)4 * m.pblk0, w.p_x0, 8 * 4 * (size_t)w.pnb);
  }
  active_mask(&w, t, m.P, col, h.active + m.u0);
  // inverse column map of the prior, and the IMU groups of every bias state (group order) -- read by the store-semantics assembly
  std::fill(h.pinv + m.p0, h.pinv + m.p0 + m.P, -1);
  for (int i = 0; i < n; ++i) h.pinv[m.p0 + col[i]] = i;
  {
    int32_t *off = h.bgl_off + m.bias0 + wi;
    std::fill(off, off + w.F + 1, 0);
    for (int gi = 0; gi < m.ngrp; ++gi) off[h.groups[m.grp0 + gi].bias + 1]++;
    for (int f = 0; f < w.F; ++f) off[f + 1] += off[f];
    std::vector<int32_t> fill(off, off + w.F);
    for (int gi = 0; gi < m.ngrp; ++gi) h.bgl[m.grp0 + fill[h.groups[m.grp0 + gi].bias]++] = m.grp0 + gi;
    for (int f = 0; f <= w.F; ++f) off[f] += m.grp0;   // absolute positions in bgl
  }
}

// The whole batch into the mirror at `base` (laid out by layout_input): the window records, then every window's slices over the pool.
inline void pack_input(const std::vector<const ctvio_window *> &wins, const std::vector<PackTmp> &tmp, const std::vector<WinMeta> &meta, const BatchFacts &b,
                       const InputLayout &lay, char *base, int vch, WorkerPool &pool, int nthreads) {
  const InputPtrs h = lay.at(base);
  std::memcpy(h.meta, meta.data(), sizeof(WinMeta) * meta.size());
  pool.run((int)wins.size(), nthreads, [&](int wi) { fill_window(*wins[wi], wi, meta[wi], tmp[wi], b, h, vch); });
}

// The staging arena mirrors the device arena byte for byte and is reused: a byte the packer does not write carries the previous batch
// to the device.  Packs the batch over 0x00 and over 0xFF (pack() fills `base`) and compares every segment's filled extent; returns the
// complaint, empty when every byte of every segment comes from the batch.
template <class Pack> inline std::string check_staging(const InputLayout &lay, char *base, Pack &&pack) {
  std::memset(base, 0x00, lay.bytes);
  pack();
  const std::vector<char> first(base, base + lay.bytes);
  std::memset(base, 0xFF, lay.bytes);
  pack();
  for (const ArenaSeg &sg : lay.segs) {
    if (std::memcmp(first.data() + sg.off, base + sg.off, sg.bytes) == 0) continue;
    size_t i = 0;
    while (first[sg.off + i] == base[sg.off + i]) ++i;
    return std::string("staging segment ") + sg.name + ": byte " + std::to_string(i) + " of " + std::to_string(sg.bytes) + " is not written by the packer";
  }
  return std::string();
}

}  // namespace ctv
