// ctvio.hip -- host runtime + C ABI (include/ctvio.h) of the MI355X sliding-window solve.
//
// The host packs windows (the reference's TrajectoryManager::UpdateTrajectory factor set,
// src/estimator/trajectory_manager.cpp:331-451) into flat HBM arrays, then drives a fixed kernel
// sequence per LM iteration on one HIP stream.  All LM decisions (step validity, acceptance,
// radius update, termination: Ceres 1.14 TrustRegionMinimizer) are taken on
// the device; the host only polls a "windows still running" counter every few iterations.
// There is no CPU fallback: without a HIP device ctvio_create fails with CTVIO_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <thread>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/ctvio.h"
#include "kernels.hpp"
#include "marginalize.hpp"
#include "marg_device.hpp"
#include "marg_blocked.hpp"
#include "host_pack.hpp"

namespace ctv {

// A prior built by ctvio_marginalize_batch lives on the next window's trajectory unknowns: every prior it can build must be solvable.
static_assert(CHOL_MAX_P == MARG_MAXD_BLOCKED, "the batch solve's bound on P and the blocked marginalisation's bound must meet");

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                                     \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) return fail(CTVIO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Diagnostic / A-B switches (include/ctvio.h, "Diagnostic switches"): read from the environment ONCE per handle, in ctvio_create -- a later
// change of the environment cannot make upload and solve disagree about a kernel choice.  None of them is needed in production.
struct DebugSwitches {
  int stamps = 0;            // CTVIO_DEBUG_STAMPS=1     clock64 stamps of a few kernels, printed by ctvio_solve (disables the hipGraph)
  int split_linearize = 0;   // CTVIO_SPLIT_LINEARIZE=1  IMU and visual evaluation as separate launches also for small batches (rocprofv3 runs)
  int schur_copy_plain = 0;  // CTVIO_SCHUR_COPY_PLAIN=1 the per-window Schur kernel copies product-free tiles to S
  int chol_tiles = -1;       // CTVIO_CHOL_TILES=0/1/3   P <= 223: panel kernel / k_cholesky_tiles (round 5: barriers) / k_cholesky_flow (default)
  int chol_compact = 0;      // CTVIO_CHOL_COMPACT=1/n   TEST ONLY: the panel kernel's slot-indexed variant for every batch it would run (1: as many
                             //                          slots as the batch needs; n >= 2: at most n slots, the rest overflows to S)
  int dense = 0;             // CTVIO_DENSE=1            the sparsity plan degenerates to the dense one
  int schur_tile2 = -1;      // CTVIO_SCHUR_TILE2=0/1    one wave per tile / per 2 x 2 tiles
  int marg_debug = 0;        // CTVIO_MARG_DEBUG=1       sweep trace of the device eigen-solver on stderr
  int marg_host = 0;         // CTVIO_MARG_HOST=1        ctvio_marginalize on the host factorisation
  int marg_blocked = 0;      // CTVIO_MARG_BLOCKED=1     ctvio_marginalize_batch: every window through the blocked path (csrc/marg_blocked.hpp)
  int shard_oversubscribe = 0;   // CTVIO_SHARD_OVERSUBSCRIBE=1  TEST ONLY: more shards than devices (ctvio_shards_used)
  int gate_slice = 0;        // CTVIO_GATE_SLICE=n       TEST ONLY: ctvio_visual_gate_batch slices its windows at n block slots (host_pack.hpp: GATE_SLICE_SLOTS),
                             //                          ctvio_imu_gate_batch at n samples (IMU_GATE_SLICE_SAMPLES)
  int poison = 0;            // CTVIO_POISON=1/2         TEST ONLY: reused double scratch starts as quiet NaN / 2.6e151 at every use; the
                             //                          upload checks that the packer writes every staged byte (host_pack.hpp: check_staging)
};
static DebugSwitches read_debug_switches() {
  DebugSwitches g;
  struct { const char *name; int *dst; } const tab[] = {
      {"CTVIO_DEBUG_STAMPS", &g.stamps}, {"CTVIO_SPLIT_LINEARIZE", &g.split_linearize},
      {"CTVIO_SCHUR_COPY_PLAIN", &g.schur_copy_plain}, {"CTVIO_CHOL_TILES", &g.chol_tiles}, {"CTVIO_CHOL_COMPACT", &g.chol_compact}, {"CTVIO_DENSE", &g.dense},
      {"CTVIO_SCHUR_TILE2", &g.schur_tile2}, {"CTVIO_MARG_DEBUG", &g.marg_debug}, {"CTVIO_MARG_HOST", &g.marg_host},
      {"CTVIO_MARG_BLOCKED", &g.marg_blocked}, {"CTVIO_SHARD_OVERSUBSCRIBE", &g.shard_oversubscribe}, {"CTVIO_POISON", &g.poison},
      {"CTVIO_GATE_SLICE", &g.gate_slice}};
  for (const auto &t : tab)
    if (const char *e = std::getenv(t.name)) *t.dst = (e[0] == '\0') ? 1 : std::atoi(e);   // (set but empty counts as 1)
  return g;
}

// Owning host copy of one window (ctvio_add_window: the caller's buffers are only read inside that call).
struct HostWindow {
  ctvio_window w;  // scalars + pointers into the vectors below
  std::vector<double> quat, pos, bias, rho, imu_gyro, imu_acc, bc_w, v_pi, v_pj, pJ0, pr0, p_x0, v_cauchy;
  std::vector<uint8_t> knot_const;
  std::vector<int64_t> imu_t, v_ti, v_tj;
  std::vector<int32_t> imu_bias, bc_i, bc_j, v_lm, v_rowi, v_rowj, p_kind, p_index, p_off;
  template <class U> static const U *own(std::vector<U> &dst, const U *src, size_t n) {
    if (src) dst.assign(src, src + n); else dst.assign(n, U(0));
    return dst.data();
  }
  explicit HostWindow(const ctvio_window &c) : w(c) {
    w.quat = own(quat, c.quat, (size_t)4 * c.K); w.pos = own(pos, c.pos, (size_t)3 * c.K);
    w.bias = own(bias, c.bias, (size_t)6 * c.F); w.rho = own(rho, c.rho, (size_t)c.L);
    w.imu_t = own(imu_t, c.imu_t, (size_t)c.M); w.imu_gyro = own(imu_gyro, c.imu_gyro, (size_t)3 * c.M);
    w.imu_acc = own(imu_acc, c.imu_acc, (size_t)3 * c.M); w.imu_bias = own(imu_bias, c.imu_bias, (size_t)c.M);
    w.bc_i = own(bc_i, c.bc_i, (size_t)c.NB); w.bc_j = own(bc_j, c.bc_j, (size_t)c.NB); w.bc_w = own(bc_w, c.bc_w, (size_t)6 * c.NB);
    w.v_lm = own(v_lm, c.v_lm, (size_t)c.V); w.v_ti = own(v_ti, c.v_ti, (size_t)c.V); w.v_tj = own(v_tj, c.v_tj, (size_t)c.V);
    w.v_rowi = own(v_rowi, c.v_rowi, (size_t)c.V); w.v_rowj = own(v_rowj, c.v_rowj, (size_t)c.V);
    w.v_pi = own(v_pi, c.v_pi, (size_t)2 * c.V); w.v_pj = own(v_pj, c.v_pj, (size_t)2 * c.V);
    w.pJ0 = own(pJ0, c.pJ0, (size_t)c.pn * c.pn); w.pr0 = own(pr0, c.pr0, (size_t)c.pn);
    w.p_kind = own(p_kind, c.p_kind, (size_t)c.pnb); w.p_index = own(p_index, c.p_index, (size_t)c.pnb);
    w.p_off = own(p_off, c.p_off, (size_t)c.pnb); w.p_x0 = own(p_x0, c.p_x0, (size_t)4 * c.pnb);
    if (c.v_cauchy) w.v_cauchy = own(v_cauchy, c.v_cauchy, (size_t)c.V);
    if (c.knot_const) w.knot_const = own(knot_const, c.knot_const, (size_t)c.K);
  }
  HostWindow(const HostWindow &) = delete;
  HostWindow &operator=(const HostWindow &) = delete;
};

class SolverImpl {
 public:
  // visual blocks per work item (k_assemble_vis_mfma): eight per-wave staging areas must fit beside the fp64 LDS Hessian -- sized by the
  // constexpr the kernel itself lays its LDS out with (kernels_assemble.hpp: vis_stage_bytes)
  static constexpr int VCH = 8;
  static constexpr size_t vis_stage_bytes() { return ctv::vis_stage_bytes(8, VCH); }
  explicit SolverImpl(const ctvio_options &o) : opt_(o), dbg_(read_debug_switches()) {}
  ~SolverImpl() {
    if (stream_) (void)hipStreamDestroy(stream_);
    for (auto &e : ev_) if (e) (void)hipEventDestroy(e);
    for (auto &e : pev_) (void)hipEventDestroy(e);
    if (graph_exec_) (void)hipGraphExecDestroy(graph_exec_);
  }
  int init() {
    HIPCHK(hipSetDevice(opt_.device));
    HIPCHK(hipStreamCreate(&stream_));
    for (auto &e : ev_) HIPCHK(hipEventCreate(&e));
    // kernels that need more than 64 KiB of dynamic LDS
    HIPCHK(hipFuncSetAttribute((const void *)k_cholesky_solve<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_cholesky_solve<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_cholesky_solve<4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_cholesky_solve<8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_cholesky_tiles, hipFuncAttributeMaxDynamicSharedMemorySize, CHOL_LDS_LIMIT));
    HIPCHK(hipFuncSetAttribute((const void *)k_cholesky_flow, hipFuncAttributeMaxDynamicSharedMemorySize, CHOL_LDS_LIMIT));
    HIPCHK(hipFuncSetAttribute((const void *)k_assemble_vis_mfma<VCH, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_assemble_vis_mfma<VCH, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_assemble_vis_mfma<VCH, true, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_schur_window_f64<7, 14>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_schur_window_f64<5, 14>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_schur_window_f64<5, 7>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_misc, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));   // (+ 2 KB of static LDS)
    HIPCHK(hipFuncSetAttribute((const void *)k_cov_solve<COV_BASE>, hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_cov_solve<COV_REL>, hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_cov_solve<COV_PROJ>, hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_cov_solve<COV_RATES>, hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_cov_solve<COV_GATE>, hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
    HIPCHK(hipFuncSetAttribute((const void *)k_cov_solve<COV_IMUGATE>, hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
    // (no attribute for k_cov_solve<COV_PRED>: its launches are limited to the default dynamic-LDS size)
    return CTVIO_OK;
  }
  int bind() { HIPCHK(hipSetDevice(opt_.device)); return CTVIO_OK; }
  int clear() { own_.clear(); uploaded_ = false; return CTVIO_OK; }
  int num_windows() const { return uploaded_ ? (int)meta_.size() : (int)own_.size(); }
  void *stream() { return (void *)stream_; }
  int graph_captures() const { return graph_captures_; }
  int marg_ran_on_host() const { return marg_ran_on_host_; }

  int add_window(const ctvio_window *w, int32_t *id) {
    std::string err;
    if (!validate_window(w, err)) return fail(CTVIO_ERR_INVALID, err);
    own_.emplace_back(new HostWindow(*w));
    if (id) *id = (int32_t)own_.size() - 1;
    uploaded_ = false;
    return CTVIO_OK;
  }
  int upload() {
    if (own_.empty()) return fail(CTVIO_ERR_STATE, "no windows");
    std::vector<const ctvio_window *> ptr(own_.size());
    for (size_t i = 0; i < own_.size(); ++i) ptr[i] = &own_[i]->w;
    return pack_and_upload(ptr, false);
  }
  // ctvio_set_batch: the windows are read straight from the caller's buffers (no intermediate copy)
  int set_batch(int n, const ctvio_window *wins) {
    if (n <= 0 || !wins) return fail(CTVIO_ERR_INVALID, "empty batch");
    own_.clear();
    uploaded_ = false;
    std::vector<const ctvio_window *> ptr((size_t)n);
    for (int i = 0; i < n; ++i) ptr[i] = wins + i;
    return pack_and_upload(ptr, true);
  }

  // ---------------------------------------------------------------------------------------- pack + upload
  // Two passes over the windows, both spread over host threads: (1) validate, sort, count; (2) fill the pinned staging
  // arena, which mirrors the device input arena byte for byte -- one hipMemcpyAsync carries the batch to HBM.  Work
  // buffers live in a second, device-only arena.  Both arenas only ever grow, so a stream of equally sized batches
  // allocates nothing after the first one.  The host-only steps (plan, offsets, layout, fill) are csrc/host_pack.hpp's.
  int pack_and_upload(const std::vector<const ctvio_window *> &wins, bool validate) {
    const int nw = (int)wins.size();
    const int nth = host_threads(opt_.host_threads);
    std::vector<PackTmp> tmp((size_t)nw);
    std::atomic<int> first_bad{nw};
    // The batch's factorisation: P <= 223 for every window -> the register-resident tile Cholesky, which keeps the whole triangle (dense
    // envelope); otherwise the panel kernel, which works inside every window's envelope.  (Sizes alone decide: known before planning.)
    int maxP_pre = 0;
    for (int wi = 0; wi < nw; ++wi) if (wins[wi]) maxP_pre = std::max(maxP_pre, 6 * wins[wi]->K + 6 * wins[wi]->F + 1);
    if (maxP_pre > CHOL_MAX_P)
      return fail(CTVIO_ERR_INVALID, "window too large for the single-workgroup Cholesky (P = 6K + 6F + 1 > " + std::to_string(CHOL_MAX_P) + ")");
    const int chol_tiles = chol_tiles_for(maxP_pre);
    const bool dense_env = chol_tiles != 0 || sparsity_off();
    // ---- plan (threads)
    pool_.run(nw, nth, [&](int wi) {
      if (validate && !validate_window(wins[wi], tmp[wi].err)) {
        int cur = first_bad.load();
        while (wi < cur && !first_bad.compare_exchange_weak(cur, wi)) {}
        return;
      }
      plan_window(wins[wi], VCH, tmp[wi]);
      if (tmp[wi].err.empty()) plan_sparsity(wins[wi], dense_env, sparsity_off(), tmp[wi]);
      if (!tmp[wi].err.empty()) {
        int cur = first_bad.load();
        while (wi < cur && !first_bad.compare_exchange_weak(cur, wi)) {}
      }
    });
    if (first_bad.load() < nw) return fail(CTVIO_ERR_INVALID, "window " + std::to_string(first_bad.load()) + ": " + tmp[first_bad.load()].err);
    // ---- lay out: offsets (serial prefix sums), then the input arena (host mirror + device)
    // The panel kernel's LDS: a fixed part and the panel, 32 columns x the full trailing height (P <= 591 fits 160 KB).  Batches beyond that
    // (or CTVIO_CHOL_COMPACT) take the slot-indexed variant: 32 x 16 doubles per slot, as many slots as the batch's panels need or fit; the
    // back-substitution reuses the panel as xs[P].
    const bool chol_compact = chol_tiles == 0 && (chol_panel_lds(maxP_pre) > 160 * 1024 || dbg_.chol_compact > 0);
    BatchFacts &b = facts_;
    b = batch_offsets(wins, tmp, chol_compact, vis_stage_bytes(), opt_.deterministic == 2, meta_, t0_);
    b.chol_tiles = chol_tiles; b.chol_compact = chol_compact; b.chol_lds = chol_panel_lds(b.maxP);
    int chol_slots = 0;
    if (chol_compact) {
      const int fit = (int)((160 * 1024 / sizeof(double) - chol_lds_fixed) / (32 * 16));
      chol_slots = std::min(b.maxSlots, fit);
      if (dbg_.chol_compact >= 2) chol_slots = std::min(chol_slots, dbg_.chol_compact);
      chol_slots = std::max(chol_slots, 2);   // (local tiles 0 and 1, the next diagonal block, take part in every panel)
      b.chol_lds = (chol_lds_fixed + std::max((size_t)32 * 16 * chol_slots, (size_t)b.maxP)) * sizeof(double);
    }
    const InputLayout lay = layout_input(b);
    // ---- reserve
    HIPCHK(hipStreamSynchronize(stream_));   // the previous batch may still be reading the staging arena (H2D in flight)
    HIPCHK(in_.reserve(lay.bytes, true, nullptr));
    // ---- fill (threads)
    auto pack = [&]() { pack_input(wins, tmp, meta_, b, lay, in_.host, VCH, pool_, nth); };
    if (dbg_.poison) {   // every byte of every segment must come from the batch: the packs over 0x00 and over 0xFF agree
      const std::string err = check_staging(lay, in_.host, pack);
      if (!err.empty()) return fail(CTVIO_ERR_INTERNAL, err);
    } else {
      pack();
    }
    const InputPtrs hp = lay.at(in_.host), dp = lay.at(in_.dev);
    h_lm_pos_ = hp.lm_pos; h_ld_ = StatePtrs(hp.state, b).ld;
    // the block slot of every caller's block (visual_gate: the upload sorts the blocks landmark-major), window after window
    gate_voff_.assign((size_t)nw + 1, 0);
    for (int wi = 0; wi < nw; ++wi) gate_voff_[(size_t)wi + 1] = gate_voff_[(size_t)wi] + (size_t)meta_[wi].V;
    gate_slot_.resize(gate_voff_[(size_t)nw]);
    for (int wi = 0; wi < nw; ++wi)
      for (int v = 0; v < meta_[wi].V; ++v) gate_slot_[gate_voff_[(size_t)wi] + (size_t)v] = meta_[wi].vis0 + tmp[wi].vpos[(size_t)v];
    // the packed slot of every caller's IMU sample (imu_gate: the upload sorts the samples by segment and bias state), window after window
    imu_moff_.assign((size_t)nw + 1, 0);
    for (int wi = 0; wi < nw; ++wi) imu_moff_[(size_t)wi + 1] = imu_moff_[(size_t)wi] + (size_t)meta_[wi].M;
    imu_slot_.resize(imu_moff_[(size_t)nw]);
    for (int wi = 0; wi < nw; ++wi) imu_slot_map(tmp[wi].iorder.data(), meta_[wi].M, meta_[wi].imu0, imu_slot_.data() + imu_moff_[(size_t)wi]);
    // ---- device pointers of the input arena
    Dev &d = dev_;
    std::memset(&d, 0, sizeof d);
    d.nwin = nw; d.Ktot = b.K0; d.Ftot = b.F0; d.Ltot = b.L0; d.Mtot = b.M0; d.Gtot = b.G0; d.Vtot = b.V0; d.Atot = b.A0;
    d.NBtot = b.B0; d.Utot = b.U0; d.maxN = b.maxN; d.maxP = b.maxP; d.maxPn = b.maxPn; d.maxL = b.maxL; d.maxLdw = b.maxLdw;
#define CTV_X(type, name, member, alloc, used) d.member = dp.name;
    CTV_INPUT_SEGMENTS(CTV_X)
#undef CTV_X
    { const StatePtrs st(dp.state, b); d.pos = st.pos; d.bias = st.bias; d.rho = st.rho; d.ld = st.ld; }   // (d.quat: the head of the block)
    if (!b.walk) d.vrow = d.vrow_off = nullptr;
    d.max_span6 = 6 * b.maxSpan;
    // ---- one copy
    HIPCHK(hipMemcpyAsync(in_.dev, in_.host, lay.bytes, hipMemcpyHostToDevice, stream_));
    // ---- launch plan (before the work arena: the partial Hessians are sized by its parts)
    // deterministic = 1: the order-fixed accumulation of the batches whose every window keeps its packed Hessian in LDS, on the matrix-core
    // kernels.  An explicit request that cannot be honoured is an error; the default (-1) falls back to the accumulate path for such batches.
    // deterministic = 2: every batch -- the other windows take the order-fixed wide-window assembly (k_assemble_wide).
    if (opt_.deterministic > 0 && opt_.deterministic != 2 && (!b.any_vis_lds || b.any_vis_glb))
      return fail(CTVIO_ERR_INVALID, "deterministic = 1 needs every window's packed Hessian in LDS (K <= 25): this batch would "
                                     "fall back to floating-point atomics");
    plan_ = make_plan(false);
    d.schur_plain_in_H = plan_.schur_plain_in_H;
    d.chol_nblk = (b.maxP + 31) / 32;
    d.chol_slots = chol_slots;
    d.line_search = opt_.line_search ? 1 : 0;
    // ---- work arena (device only)
    if (const int rc = layout_work()) return rc;
    // ---- the fixed head of call_io_ (HEAD_*): the pinned landing areas of the results; every call reserves head + its own tail (reserve_call)
    head_ = CallLayout();
    head_.add("lm", sizeof(Lm), (size_t)nw, false); head_.add("poll", sizeof(int32_t), 4, false); head_.add("state", sizeof(double), state_doubles_, false);
    snap_valid_ = false;
    uploaded_ = true;
    return CTVIO_OK;
  }

  // The work arena (device only), every segment ONCE: X(element type, the pointer it becomes, name, count, doubles that CTVIO_POISON
  // may poison -- the integer segments never are: they feed addresses).  Three stretches: the middle one is zeroed at every upload.
  // Irregular: cstate and snap are contiguous state blocks like the input's (StatePtrs); Hpart holds one entry unless the store tail runs
  // with several parts; vexp one entry unless the order-fixed wide assembly runs (Dev gets null); Hpp / W / Hll / g come as two
  // normal-equation sets (current linearisation / speculative linearisation at the candidate, Lm::cur); nact is n_active and span_viol
  // (+ two spare words); dbg reaches Dev only with CTVIO_DEBUG_STAMPS.
#define CTV_WORK_HEAD(X)                                                                                                  \
  X(double, d.cquat, "cstate", state_doubles_, true) X(double, snap_, "snap", state_doubles_, true)                      \
  X(double, d.lkd, "lkd", 3 * K0, true) X(double, d.kjri, "kjri", 9 * K0, true) X(double, d.imu_tiles, "tiles", 1024 * G0, true) \
  X(double, d.imu_cost, "imu_cost", std::max<size_t>(G0, 1), true) X(double, d.vis_cost, "vis_cost", (Vt + 63) / 64, true) \
  X(double, d.misc_cost, "misc_cost", nw, true)                                                                          \
  X(double, d.pgrad, "pgrad", std::max<size_t>(b.pv0, 1), true)                                                          \
  /* packed partial Hessians of the multi-part store-semantics assembly (knot triangle + line-delay row + gradient per part) */ \
  X(double, d.Hpart, "Hpart", nparts_alloc > 1 ? part_stride * nparts_alloc * nw : 1, true)                              \
  X(double, d.Jt, "Jt", (size_t)VT_ROWS * 64 * ((Vt + 63) / 64), true) X(int32_t, d.vsj, "vsj", Vt, false)                \
  X(double, d.arec, "arec", (size_t)AREC * At, true) X(int32_t, d.a_s, "a_s", At, false)                                  \
  /* expanded block records of the wide windows (k_vis_expand) */                                                        \
  X(double, d.vexp, "vexp", wide ? (size_t)VX_LD * Vt : 1, true)                                                          \
  X(double, d.HppS[0], "Hpp", H0, true) X(double, d.HppS[1], "Hpp1", H0, true) X(double, d.S, "S", H0, true)
#define CTV_WORK_ZEROED(X)                                                                                                \
  X(double, d.WS[0], "W", W0, true) X(double, d.WS[1], "W1", W0, true) X(double, d.HllS[0], "Hll", L0, true) X(double, d.HllS[1], "Hll1", L0, true) \
  X(double, d.gS[0], "g", U0, true) X(double, d.gS[1], "g1", U0, true) X(double, d.delta, "delta", U0, true)              \
  X(double, d.cscale, "cscale", U0, true) X(Lm, d.lm, "lm", nw, false) X(int32_t, d.n_active, "nact", 4, false) X(long long, d.dbg, "dbg", 128, false)
#define CTV_WORK_TAIL(X)                                                                                                  \
  X(double, d.rhs, "rhs", b.Pp0, true) X(double, d.dd, "dd", U0, true) X(double, d.dinv, "dinv", L0, true) X(double, d.grs, "grs", L0, true) \
  X(double, d.chol_inv, "chol_inv", nw * d.chol_nblk * 1024, true)
  int layout_work() {
    Dev &d = dev_;
    const BatchFacts &b = facts_;
    const size_t nw = b.nw, K0 = b.K0, L0 = b.L0, G0 = b.G0, U0 = b.U0, H0 = (size_t)b.H0, W0 = (size_t)b.W0;
    const size_t Vt = (size_t)std::max(b.V0, 1), At = (size_t)std::max(b.A0, 1);
    state_doubles_ = (size_t)7 * b.K0 + 6 * b.F0 + b.L0 + nw;
    // (only the LDS-resident windows have parts: with deterministic = 2 a batch may hold wider ones)
    const bool wide = plan_.tail == TAIL_STORE_WIDE;
    const int kpart = wide ? b.maxK_lds : b.maxK;
    const size_t part_stride = ((size_t)6 * kpart * (6 * kpart + 1) / 2 + 2 * (6 * (size_t)kpart + 1) + 7) & ~(size_t)7;
    const size_t nparts_alloc = plan_.tail != TAIL_ACCUMULATE && kpart > 0 ? plan_.parts : 1;
    d.npart_stride = (int32_t)part_stride;
    size_t off = 0;
#define CTV_X(type, ptr, name, count, dbl) off += arena_align(sizeof(type) * (size_t)(count));
    CTV_WORK_HEAD(CTV_X)
    const size_t o_zero0 = off;   // ---- zeroed at every upload from here ...
    CTV_WORK_ZEROED(CTV_X)
    const size_t o_zero1 = off;   // ---- ... to here
    CTV_WORK_TAIL(CTV_X)
#undef CTV_X
    bool grew = false;
    HIPCHK(work_.reserve(off, false, &grew));
    if (grew || dbg_.poison) HIPCHK(hipMemsetAsync(work_.dev, 0, work_.cap, stream_));   // fresh memory may hold NaN patterns (0 * NaN in masked products)
    // (CTVIO_POISON: every double segment outside the per-upload zero region starts as the pattern)
    char *p = work_.dev;
#define CTV_X(type, ptr, name, count, dbl)                                                                                               \
  ptr = reinterpret_cast<type *>(p);                                                                                                     \
  if (dbl && !zeroed && poison(p, sizeof(type) * (size_t)(count)) != hipSuccess) return fail(CTVIO_ERR_HIP, "CTVIO_POISON: work segment " name); \
  p += arena_align(sizeof(type) * (size_t)(count));
    bool zeroed = false;
    CTV_WORK_HEAD(CTV_X)
    zeroed = true;
    CTV_WORK_ZEROED(CTV_X)
    zeroed = false;
    CTV_WORK_TAIL(CTV_X)
#undef CTV_X
    { const StatePtrs st(d.cquat, b); d.cpos = st.pos; d.cbias = st.bias; d.crho = st.rho; d.cld = st.ld; }
    if (!wide) d.vexp = nullptr;
    d.span_viol = d.n_active + 1;
    if (!dbg_.stamps) d.dbg = nullptr;
    HIPCHK(hipMemsetAsync(work_.dev + o_zero0, 0, o_zero1 - o_zero0, stream_));
    return CTVIO_OK;
  }

  // ---------------------------------------------------------------------------------------- launch plan
  // Every resolved decision of the launch list, and nothing else: built by make_plan, the only place that turns a switch or an option into a
  // kernel choice; the launch_* functions read dev_ and this.  Built zero-filled, like Dev: the captured graph is valid while both compare equal.
  enum { TAIL_ACCUMULATE = 0, TAIL_STORE, TAIL_STORE_WIDE };                                        // LaunchPlan::tail
  enum { SCHUR_WINDOW_5_7 = 0, SCHUR_WINDOW_5_14, SCHUR_WINDOW_7_14, SCHUR_TILE, SCHUR_TILE2 };     // LaunchPlan::schur
  enum { CHOL_FLOW = 0, CHOL_TILES, CHOL_PANEL };                                                   // LaunchPlan::chol
  struct LaunchPlan {
    int32_t tail;                    // assembly tail: atomics into zeroed Hpp / g; every entry stored once; stored once + k_assemble_wide for the wide windows
    int32_t parts;                   // workgroups per window of the visual assembly
    int32_t lds_windows, glb_windows;   // the batch has windows with / without the LDS-resident packed Hessian
    int32_t merged, misc_in_pre;     // linearisation in two launches (else split); the prior gradient + cost share rides in k_pre_linearize
    int32_t imu_zero, imu_general;   // kernels_imu.hpp: imu_zero_share mode; every IMU group through the general body
    int32_t misc_imu;                // k_misc's IMU share on the accumulate path: 0 none, 1 straight to Hpp, 2 through the LDS band
    int32_t schur, schur_tiles;      // the Schur kernel; tile kernels: 16 x 16 tiles (or 32 x 32 blocks) per window
    int32_t schur_plain_in_H;        // Dev::schur_plain_in_H
    int32_t chol;                    // the solve's Cholesky kernel
    int32_t panel_slots, panel_waves;   // the panel kernel (launch_chol_panel: the solve's CHOL_PANEL, the covariance's for every batch): slot-indexed variant; waves
    int32_t finish_waves;            // k_step_finish
    int32_t wide_tiles;              // k_assemble_wide: tile rows of the augmented knot block
    size_t vis_lds, vis_glb, misc_lds, schur_lds, chol_lds, panel_lds;   // dynamic LDS bytes (chol_lds: the tile kernels')
  };
  // Runs once per upload, and again around a profiled solve (which keeps every kernel apart); never per pass.
  LaunchPlan make_plan(bool profiling) const {
    const BatchFacts &b = facts_;
    const int nw = b.nw;
    LaunchPlan p;
    std::memset(&p, 0, sizeof p);
    p.lds_windows = b.any_vis_lds; p.glb_windows = b.any_vis_glb;
    // Store-semantics assembly tail (kernels.hpp: bias_rows_store; every entry written once, no atomics): the deterministic mode, when
    // every window's packed Hessian is LDS resident.  (The throughput mode does not take it: measured slower there, the bias-row gather
    // costs more than the zeroing + atomic passes it replaces -- 14.5 vs 13.4 ms per 2048-window solve.)
    // With deterministic = 2 and a window beyond the LDS-resident Hessian the choice is per window: the LDS-resident ones take this tail, the
    // others k_assemble_wide -- both store every entry once, so the batch has no zeroing pass and no atomic assembly at all.
    // (the default falls back to the accumulate path for batches the order-fixed assembly cannot cover; deterministic = 1 on such a batch
    //  was refused by the upload)
    const bool mixed = !b.any_vis_lds || b.any_vis_glb;
    const bool deterministic = mixed ? opt_.deterministic > 0 : (opt_.deterministic > 0 || (opt_.deterministic < 0 && nw <= 64));
    p.tail = !deterministic ? TAIL_ACCUMULATE : (opt_.deterministic == 2 && b.any_vis_glb) ? TAIL_STORE_WIDE : TAIL_STORE;
    const bool store = p.tail != TAIL_ACCUMULATE;
    // Workgroups per window of the visual assembly: batches smaller than the chip split a window's items over several parts.  In the
    // deterministic mode a part is ONE wave (its LDS additions happen in program order) and there are more of them.
    p.parts = store ? std::min(32, std::max(1, 512 / std::max(nw, 1))) : std::min(8, std::max(1, 256 / std::max(nw, 1)));
    // The merged launch runs the visual body with the IMU body's register allocation (one wave per SIMD): only for batches smaller than
    // the chip, where the single-wave latencies of the two evaluations overlap instead of adding up.
    p.merged = b.G0 && b.V0 && !profiling && !dbg_.split_linearize && nw <= 128;
    // (the merged launch carries the prior gradient + cost share only while dx fits its LDS next to the reduction cells)
    p.misc_in_pre = p.merged && b.maxPn <= PRE_LIN_MAX_PN;
    // The IMU linearisation kernels clear the accumulated parts of the normal equations on the side (kernels.hpp: imu_zero_share) when every
    // window has IMU groups: 1 = bias rows only (one visual-assembly part stores the knot x knot block), 2 = everything; 0 = k_zero_normal.
    p.imu_zero = (store || !b.all_imu) ? 0 : (p.parts == 1 ? 1 : 2);
    // use_mfma = 2: every IMU group through the general body (k_imu_linearize_rest) -- the cross-check of the specialised one and the
    // tests' way into the path that large knot-to-knot rotations / anisotropic accelerometer weights take
    p.imu_general = opt_.use_mfma == 2 ? 1 : 0;
    p.vis_lds = b.vis_lds_bytes; p.vis_glb = b.vis_glb_bytes;
    {
      // (windows without the LDS-resident Hessian: the IMU knot blocks are summed in an LDS band before they go to Hpp -- when it fits)
      const size_t dxb = (size_t)((std::max(b.maxPn, 1) + 1) & ~1) * sizeof(double), bandb = (size_t)144 * b.maxK * sizeof(double);
      const bool band = b.any_vis_glb && b.G0 && dxb + bandb <= 150 * 1024;
      p.misc_lds = band ? dxb + bandb : dxb;
      p.misc_imu = b.G0 ? (band ? 2 : 1) : 0;
    }
    {
      // Large batches of small windows take the per-window Schur kernel (one workgroup per window, W staged through LDS once); everything else
      // the tile kernels: one wave per 16 x 16 tile (shorter latency, W re-read per tile).  Every variant also produces the reduced
      // right-hand side (g_rho rides as column P).
      const int nt = (b.maxLdw + 15) / 16, ntile = nt * (nt + 1) / 2;
      const size_t lds = ((size_t)2 * 16 * (b.maxLdw + 16) + 3 * b.maxLdw + 32 + 64) * sizeof(double);   // + column vectors + the list of tiles with products
      const int nc = 6 * b.maxK + 2;   // compact columns of W per landmark: knots, line delay, g_rho
      const int nt2 = b.maxP / 16 + 1, ntile2 = nt2 * (nt2 + 1) / 2;   // tile rows up to index P (the rhs row)
      const int nb2 = (nt2 + 1) / 2, nblk2 = nb2 * (nb2 + 1) / 2;      // 32 x 32 blocks of the lower triangle
      if (nw >= 192 && b.maxLdw <= 224 && ntile <= 112 && lds <= 160 * 1024 && nc <= 224) {
        p.schur = (16 * nc <= 5 * 512 && b.maxSchurTiles <= 56) ? SCHUR_WINDOW_5_7 : (16 * nc <= 5 * 512) ? SCHUR_WINDOW_5_14 : SCHUR_WINDOW_7_14;
        p.schur_lds = lds;
      }
      // enough tiles to fill the chip several times over (config 5: 666 per window): one wave per 2 x 2 tiles, half the operand loads
      // per product; otherwise one wave per tile (more waves in flight).  CTVIO_SCHUR_TILE2 = 0 / 1 forces the choice (A/B).
      else if (dbg_.schur_tile2 >= 0 ? dbg_.schur_tile2 != 0 : (long long)nw * ntile2 >= 16384) { p.schur = SCHUR_TILE2; p.schur_tiles = nblk2; }
      else { p.schur = SCHUR_TILE; p.schur_tiles = ntile2; }
    }
    // P <= 223: the register-resident tile kernel (S read once, nothing written back; 16 waves per window) for batches smaller than
    // the chip, where latency counts; large batches: the panel kernel with 4 waves, two windows per CU (throughput); windows beyond
    // 223 unknowns: the panel kernel, with 8 waves when there are fewer windows than CUs
    if (b.chol_tiles) {
      const int ntr = b.maxP / 16 + 1;
      p.chol = b.chol_tiles == 1 ? CHOL_TILES : CHOL_FLOW;   // (CTVIO_CHOL_TILES=1: round 5's kernel)
      p.chol_lds = b.chol_tiles == 1 ? CholTilesLds(ntr).bytes : CholFlowLds(ntr).bytes;
    } else {
      p.chol = CHOL_PANEL;
    }
    // The panel kernel of the batch, whichever kernel the solve takes (a pure function of the sizes that also key the graph):
    // (8 waves also when the panel's LDS footprint allows one workgroup per CU anyway -- P = 571: 157 KB -- where 4 waves left three quarters
    //  of the CU's wave slots empty)
    // (windows beyond 591 unknowns: the slot-indexed variant, same wave-count rule)
    p.panel_slots = b.chol_compact ? 1 : 0;
    p.panel_lds = b.chol_lds;
    p.panel_waves = (nw <= 192 || b.chol_lds > 80 * 1024) ? 8 : 4;
    // Dev::schur_plain_in_H is part of the Dev struct the captured graph is keyed on: decided once per upload, never inside a launch
    // (launch_schur used to set it, so every upload -- which clears Dev -- invalidated the cached hipGraph of the headline configuration).
    p.schur_plain_in_H = (p.schur <= SCHUR_WINDOW_7_14 && b.chol_tiles != 0 && !dbg_.schur_copy_plain) ? 1 : 0;
    // (fewer windows than CUs: 8 waves per window shorten the landmark back-substitution; 16 waves -- a 128-register cap -- spilled 18
    //  registers to scratch and were measured slower: 3.15 vs 3.09 ms per single-window solve)
    p.finish_waves = nw <= 192 ? 8 : 4;
    p.wide_tiles = (6 * b.maxK + 2 + 15) / 16;
    return p;
  }

  // ---------------------------------------------------------------------------------------- launches
  static int nblk(long long n, int b) { return (int)std::max<long long>((n + b - 1) / b, 1); }
  void set_params(int max_iters) {
    LmParams &p = dev_.prm;
    p.ftol = opt_.function_tolerance; p.gtol = opt_.gradient_tolerance; p.ptol = opt_.parameter_tolerance;
    p.max_radius = opt_.max_radius; p.min_radius = opt_.min_radius; p.min_rel_dec = opt_.min_relative_decrease;
    p.min_diag = opt_.min_lm_diagonal; p.max_diag = opt_.max_lm_diagonal; p.max_invalid = opt_.max_consecutive_invalid_steps;
    p.max_iters = max_iters;
  }
  // ctvio_last_timing's record: ms[0..6] per phase of a profiled solve (or the covariance's three kernels), ms[7] the whole call on the
  // device; n[0..6] the launches behind each figure, n[7] the passes of the solve.  A call clears its own copy, fills it and publishes it.
  struct Timing {
    double ms[8];
    int32_t n[8];
    void clear() { *this = Timing{}; }
  };
  enum Ev { EV_CALL_BEGIN = 0, EV_CALL_END, EV_QUERY_BEGIN, EV_QUERY_END, EV_COV_PREPARE, EV_COV_FACTOR, EV_COV_SOLVE, EV_COV_GRAM, EV_COUNT };
  // Per-phase timing with HIP events on the solver's stream (only when profiling is switched on).
  enum { PH_IMU_LIN = 0, PH_VIS_LIN, PH_ASM_VIS, PH_ASM_REST, PH_SCHUR, PH_CHOL, PH_REST, PH_COUNT };
  void ph_begin(int ph) {
    if (!profiling_) return;
    if (pev_used_ + 2 > pev_.size()) {
      for (int i = 0; i < 64; ++i) { hipEvent_t e; (void)hipEventCreate(&e); pev_.push_back(e); }
    }
    (void)hipEventRecord(pev_[pev_used_], stream_);
    pev_phase_.push_back(ph);
    pev_used_ += 2;
  }
  void ph_end() {
    if (!profiling_) return;
    (void)hipEventRecord(pev_[pev_used_ - 1], stream_);
  }
  void ph_collect(Timing &t) {
    for (size_t i = 0; i < pev_phase_.size(); ++i) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, pev_[2 * i], pev_[2 * i + 1]) == hipSuccess) { t.ms[pev_phase_[i]] += ms; t.n[pev_phase_[i]] += 1; }
    }
    pev_phase_.clear();
    pev_used_ = 0;
  }
  // Linearisation of every window the mode selects (kernels.hpp: LIN_AT_X / LIN_SPEC / COST_AT_X) into its normal-equation set;
  // the cost partials of the evaluated state come out on the way.
  void launch_linearize(int mode) {
    const Dev &d = dev_;
    const LaunchPlan &p = plan_;
    const int nw = d.nwin;
    ph_begin(PH_ASM_REST);
    if (p.tail == TAIL_ACCUMULATE) { if (!p.imu_zero) hipLaunchKernelGGL(k_zero_normal, dim3(64, nw), dim3(256), 0, stream_, d, p.parts == 1 ? 1 : 0, mode); }
    else if (!p.misc_in_pre) hipLaunchKernelGGL(k_misc, dim3(nw), dim3(256), std::max(d.maxPn, 1) * sizeof(double), stream_, d, mode, 1, 0);   // prior gradient + cost share
    ph_end();
    if (p.merged) {
      // Small batches: TWO launches for the whole linearisation.  k_pre_linearize: the anchors' records, the IMU groups the specialised body
      // leaves out and (store-semantics path) the prior gradient + cost share -- three launches of 5 - 7 us each until round 5; then
      // k_linearize_f64: both evaluations (independent work: their latencies overlap on batches smaller than the chip).  A profiled
      // solve (and CTVIO_SPLIT_LINEARIZE=1, for rocprofv3 runs) keeps everything apart so that each kernel gets its own timing.
      const int nab = nblk(d.Atot, 64), with_misc = p.tail != TAIL_ACCUMULATE && p.misc_in_pre ? 1 : 0;
      hipLaunchKernelGGL(k_pre_linearize, dim3(nab + nw + (with_misc ? nw : 0)), dim3(64), 0, stream_, d, mode, p.imu_general, p.imu_zero, nab, with_misc);
      hipLaunchKernelGGL(k_linearize_f64, dim3(d.Gtot + nblk(d.Vtot, 64)), dim3(64), 0, stream_, d, mode, p.imu_general, p.imu_zero);
      return;
    }
    launch_evaluate(mode);
  }
  // The evaluations as separate launches (the split linearisation, and ctvio_cost): IMU groups, anchors, visual blocks.
  static constexpr int IMU_WALK_WAVES = 2048;   // walking waves of k_imu_linearize_f64
  void launch_evaluate(int mode) {
    const Dev &d = dev_;
    ph_begin(PH_IMU_LIN);
    if (d.Gtot) {
      // (at most 2048 waves -- two rounds of one wave per SIMD -- each walking its share of the groups with the next group's data in flight)
      hipLaunchKernelGGL(k_imu_linearize_f64, dim3(std::min(d.Gtot, IMU_WALK_WAVES)), dim3(64), (size_t)(72 * 33 + 64) * sizeof(double), stream_, d, mode, plan_.imu_general, plan_.imu_zero);
      hipLaunchKernelGGL(k_imu_linearize_rest, dim3(d.nwin), dim3(64), (size_t)64 * 33 * sizeof(double), stream_, d, mode, plan_.imu_general, plan_.imu_zero);
    }
    ph_end();
    ph_begin(PH_VIS_LIN);   // (one timed group: the anchors' records, then the blocks)
    if (d.Atot) hipLaunchKernelGGL(k_vis_anchor, dim3(nblk(d.Atot, 64)), dim3(64), 0, stream_, d, mode);   // the i ends, once per anchor
    if (d.Vtot) hipLaunchKernelGGL(k_vis_eval, dim3(nblk(d.Vtot, 64)), dim3(64), 0, stream_, d, mode);
    ph_end();
  }
  void launch_assemble(int mode) {
    const Dev &d = dev_;
    const LaunchPlan &p = plan_;
    const int nw = d.nwin;
    const int parts = p.parts;   // few windows: split each window's items over several workgroups to fill the chip
    if (p.tail != TAIL_ACCUMULATE) {
      // every entry of Hpp / g is written once, completely, with a plain store: no zeroing pass, no k_assemble_imu, no atomics
      ph_begin(PH_ASM_VIS);
      if (p.lds_windows) {   // (the store tail always runs in the deterministic mode: a part is ONE wave)
        hipLaunchKernelGGL((k_assemble_vis_mfma<VCH, true, 1, true>), dim3(nw, parts), dim3(64), p.vis_lds, stream_, d, mode);
        if (parts > 1) hipLaunchKernelGGL(k_reduce_finalize, dim3(48, nw), dim3(256), 0, stream_, d, mode, parts);
        else hipLaunchKernelGGL(k_bias_rows, dim3(8, nw), dim3(256), 0, stream_, d, mode);
      }
      if (p.tail == TAIL_STORE_WIDE) launch_assemble_wide(mode);
      ph_end();
      if (mode != LIN_SPEC) {   // (the candidate's gradient norm: k_pass_end)
        ph_begin(PH_ASM_REST);
        hipLaunchKernelGGL(k_post_linearize, dim3(nblk(d.maxN, 256), nw), dim3(256), 0, stream_, d, mode);
        ph_end();
      }
      return;
    }
    ph_begin(PH_ASM_VIS);
    if (p.lds_windows) hipLaunchKernelGGL((k_assemble_vis_mfma<VCH, true>), dim3(nw, parts), dim3(512), p.vis_lds, stream_, d, mode);
    // windows whose packed Hessian does not fit in LDS (K > 25): run products on the MFMA units, added to Hpp with global atomics
    if (p.glb_windows) hipLaunchKernelGGL((k_assemble_vis_mfma<VCH, false>), dim3(nw, parts), dim3(512), p.vis_glb, stream_, d, mode);
    ph_end();
    ph_begin(PH_ASM_REST);
    // (the IMU tiles' bias rows, the bias chain and the prior in ONE launch: k_misc with assemble_imu_window in front)
    hipLaunchKernelGGL(k_misc, dim3(nw), dim3(256), p.misc_lds, stream_, d, mode, 0, p.misc_imu);
    if (mode != LIN_SPEC) hipLaunchKernelGGL(k_post_linearize, dim3(nblk(d.maxN, 256), nw), dim3(256), 0, stream_, d, mode);
    ph_end();
  }
  // Trust-region step of every window that starts a new iteration (damping, Schur complement, Cholesky, back-substitution), then the
  // candidate x (+) alpha delta of every window with a valid step (also those inside the line search: new alpha, same delta).
  void launch_step() {
    const Dev &d = dev_;
    const LaunchPlan &p = plan_;
    const int nw = d.nwin;
    ph_begin(PH_SCHUR);
    launch_schur(d);
    ph_end();
    ph_begin(PH_CHOL);
    switch (p.chol) {
      case CHOL_TILES: hipLaunchKernelGGL(k_cholesky_tiles, dim3(nw), dim3(1024), p.chol_lds, stream_, d); break;
      case CHOL_FLOW: hipLaunchKernelGGL(k_cholesky_flow, dim3(nw), dim3(1024), p.chol_lds, stream_, d); break;
      default: launch_chol_panel(d);
    }
    ph_end();
    ph_begin(PH_REST);
    if (p.finish_waves == 8) hipLaunchKernelGGL((k_step_finish<8>), dim3(nw), dim3(512), (size_t)d.maxP * sizeof(double), stream_, d);
    else hipLaunchKernelGGL((k_step_finish<4>), dim3(nw), dim3(256), (size_t)d.maxP * sizeof(double), stream_, d);
    ph_end();
  }
  void launch_chol_panel(const Dev &d) {   // (d: dev_, or the covariance's copy of it)
    const LaunchPlan &p = plan_;
    if (p.panel_slots) {
      if (p.panel_waves == 8) hipLaunchKernelGGL((k_cholesky_solve<8, true>), dim3(d.nwin), dim3(512), p.panel_lds, stream_, d);
      else hipLaunchKernelGGL((k_cholesky_solve<4, true>), dim3(d.nwin), dim3(256), p.panel_lds, stream_, d);
    } else {
      if (p.panel_waves == 8) hipLaunchKernelGGL((k_cholesky_solve<8>), dim3(d.nwin), dim3(512), p.panel_lds, stream_, d);
      else hipLaunchKernelGGL((k_cholesky_solve<4>), dim3(d.nwin), dim3(256), p.panel_lds, stream_, d);
    }
  }
  void launch_schur(const Dev &d) {   // (d: dev_, or the covariance's copy of it)
    const LaunchPlan &p = plan_;
    const int ngrid = p.schur_tiles * 8 * ((d.nwin + 7) / 8);   // (the tile kernels)
    switch (p.schur) {
      case SCHUR_WINDOW_5_7: hipLaunchKernelGGL((k_schur_window_f64<5, 7>), dim3(d.nwin), dim3(512), p.schur_lds, stream_, d); break;
      case SCHUR_WINDOW_5_14: hipLaunchKernelGGL((k_schur_window_f64<5, 14>), dim3(d.nwin), dim3(512), p.schur_lds, stream_, d); break;
      case SCHUR_WINDOW_7_14: hipLaunchKernelGGL((k_schur_window_f64<7, 14>), dim3(d.nwin), dim3(512), p.schur_lds, stream_, d); break;
      case SCHUR_TILE2: hipLaunchKernelGGL(k_schur_tile2_f64, dim3(ngrid), dim3(64), 0, stream_, d, p.schur_tiles); break;
      default: hipLaunchKernelGGL(k_schur_tile_f64, dim3(ngrid), dim3(64), 0, stream_, d, p.schur_tiles);
    }
  }
  // The windows beyond the LDS-resident Hessian under deterministic = 2: the expanded block records, one workgroup per 16 x 16 tile of the knot
  // block + line-delay row + gradient (augmented: 6K + 2 unknowns), the bias rows by gather.
  void launch_assemble_wide(int mode) {
    const Dev &d = dev_;
    const int nt = plan_.wide_tiles;
    if (d.Vtot) hipLaunchKernelGGL(k_vis_expand, dim3(nblk((long long)d.Vtot * (VX_COLS + 1), 256)), dim3(256), 0, stream_, d, mode);
    hipLaunchKernelGGL(k_assemble_wide, dim3(nt * (nt + 1) / 2, d.nwin), dim3(64 * WIDE_NW), 0, stream_, d, mode);
    hipLaunchKernelGGL(k_bias_rows_wide, dim3(32, d.nwin), dim3(256), 0, stream_, d, mode);
  }
  // CTVIO_CHOL_TILES = 0 / 1 / 3 forces the choice (A/B measurements: panel kernel / k_cholesky_tiles / k_cholesky_flow)
  int chol_tiles_for(int maxP) const {
    if (maxP > 223) return 0;
    if (dbg_.chol_tiles >= 0) return dbg_.chol_tiles;
    return 3;   // (register-resident tiles as a data-flow of waves: k_cholesky_flow; 1 = round 5's k_cholesky_tiles, the barrier-per-panel form)
  }
  // k_cholesky_solve's LDS in doubles: Lb, LiT, dinvs, yb, flags, plist (fixed) + the panel, 32 columns x the trailing height of the first panel
  static constexpr size_t chol_lds_fixed = 2 * 32 * 34 + 32 + 34 + 32;
  static size_t chol_panel_lds(int maxP) { return (chol_lds_fixed + (size_t)((std::max(maxP - 32, 0) + 1 + 15) / 16 * 16) * 32) * sizeof(double); }
  // CTVIO_DENSE=1: the sparsity plan degenerates to the dense one (every row range = all landmarks, envelope = the whole triangle) -- the
  // A/B switch of the sparsity-aware kernels and the cross-check of tests/test_gpu_sparsity.py
  bool sparsity_off() const { return dbg_.dense == 1; }

  // One PASS of the device-resident LM: every running window advances by one phase -- a new trust-region iteration (damp, Schur,
  // Cholesky, back-substitute, candidate) or, inside Ceres' projected line search, one trial step (candidate at the new alpha) --
  // and the candidate is evaluated ONCE: speculative linearisation into the window's other normal-equation set, cost as a
  // by-product; k_pass_end accepts / rejects / continues the search, swaps the sets on acceptance and starts the next iteration
  // (continuation tests, LM diagonal).  The launch list is fixed: kernels skip windows that are not in the matching phase.
  void launch_pass() {
    Dev &d = dev_;
    const int nw = d.nwin;
    launch_step();
    launch_linearize(LIN_SPEC);
    launch_assemble(LIN_SPEC);
    ph_begin(PH_REST);
    // (windows that start another pass count themselves in k_pass_end; the counter was cleared by k_step_finish)
    hipLaunchKernelGGL(k_pass_end, dim3(nw), dim3(256), 0, stream_, d);
    ph_end();
  }
  // The first linearisation of a solve (and of the diagnostic entries): knot-pair constants, normal equations and cost of the
  // current state in set 0, Jacobi scaling.
  void launch_initial(double mu) {
    launch_prepare(mu, 0);
    launch_linearize(LIN_AT_X);
    launch_assemble(LIN_AT_X);
    hipLaunchKernelGGL(k_initial_cost, dim3(dev_.nwin), dim3(64), 0, stream_, dev_, 0);
  }
  // what every evaluation of the current state starts with (launch_initial, ctvio_cost): the LM records, the knot-pair constants
  void launch_prepare(double mu, int keep_scale) {
    const Dev &d = dev_;
    hipLaunchKernelGGL(k_lm_init, dim3(nblk(d.nwin, 64)), dim3(64), 0, stream_, d, mu, keep_scale);
    hipLaunchKernelGGL(k_knot_prep, dim3(nblk(d.Ktot, 256)), dim3(256), 0, stream_, d);
  }
  // The pass as a hipGraph (captured once per batch shape: the kernel arguments are the Dev struct, so equal shapes in the
  // grow-only arenas give identical graphs), replayed instead of ~25 launches.  Everything else the launch list depends on -- dynamic
  // LDS sizes, kernel choices (template arguments, which assembly variants run) -- is the launch plan: two batches with identical totals
  // can differ in these (e.g. the same sum K split differently).
  int ensure_graph() {
    if (graph_exec_ && std::memcmp(&graph_dev_, &dev_, sizeof dev_) == 0 && std::memcmp(&graph_plan_, &plan_, sizeof plan_) == 0) return CTVIO_OK;
    if (graph_exec_) { (void)hipGraphExecDestroy(graph_exec_); graph_exec_ = nullptr; }
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
    launch_pass();
    HIPCHK(hipStreamEndCapture(stream_, &g));
    hipError_t e = hipGraphInstantiate(&graph_exec_, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { graph_exec_ = nullptr; return fail(CTVIO_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); }
    graph_dev_ = dev_;
    graph_plan_ = plan_;
    ++graph_captures_;
    return CTVIO_OK;
  }

  // ---------------------------------------------------------------------------------------- per-call entries
  // Every entry below starts with guard() and lays its scratch out ONCE (host_pack.hpp: CallLayout) in two arenas: call_io_, mirrored by
  // pinned host memory, holds what is copied in or out -- every asynchronous copy to the host lands in its mirror and reaches the caller's
  // buffer after the synchronise --, call_scr_ (device only) everything else.  io starts as a copy of head_, the result areas
  // pack_and_upload laid out (HEAD_*: the LM records, the poll words -- a segment of their own, so they alias no record at any nwin --, the
  // batch state); segments after io.landing() have no device twin (their sources lie in the input / work arena).  Irregular: the head is
  // such a landing area too, but stays in front, so its device twin is unused.  reserve_call comes before the first launch or copy that
  // takes a pointer into either arena.  CTVIO_POISON: every segment declared dbl -- doubles the call reads after a kernel wrote them --
  // starts as the pattern at every call; integer segments and staged inputs never do.
  enum { HEAD_LM = 0, HEAD_POLL, HEAD_STATE };
  int guard() const { return uploaded_ ? CTVIO_OK : fail(CTVIO_ERR_STATE, "ctvio_upload not called"); }
  int guard(int id, const char *msg = "window id out of range") const {
    if (const int rc = guard()) return rc;
    return id >= 0 && id < dev_.nwin ? CTVIO_OK : fail(CTVIO_ERR_INVALID, msg);
  }
  int reserve_call(CallLayout &io, CallLayout *scr = nullptr) {
    HIPCHK(call_io_.reserve(io.dev_bytes(), true, nullptr, io.bytes() - io.dev_bytes()));
    io.reserved();
    if (scr) { HIPCHK(call_scr_.reserve(scr->bytes(), false, nullptr, 0, false)); scr->reserved(); }
    if (!dbg_.poison) return CTVIO_OK;
    for (const ArenaSeg &sg : io.segs()) if (sg.dbl) HIPCHK(poison(call_io_.dev + sg.off, sg.bytes));
    if (scr) for (const ArenaSeg &sg : scr->segs()) if (sg.dbl) HIPCHK(poison(call_scr_.dev + sg.off, sg.bytes));
    return CTVIO_OK;
  }
  template <class U> U *io_host(const CallLayout &io, int seg) { return io.at<U>(call_io_.host, seg); }
  template <class U> U *io_dev(const CallLayout &io, int seg) { return io.at<U>(call_io_.dev, seg); }
  int sync_call() {
    HIPCHK(hipStreamSynchronize(stream_));
    HIPCHK(hipGetLastError());
    return CTVIO_OK;
  }
  // The end of every entry that launches k_vis_eval, in ONE blocking round trip with the entry's own copies.  The kernel counts evaluations
  // that fall outside the knot span the packer planned for their landmark (host_pack.hpp: plan_sparsity): such a row of W was written into
  // a neighbour's columns.  The counter is cleared again so that a later call on the same batch (after ctvio_set_state /
  // ctvio_restore_state) starts clean.
  int finish_call(const CallLayout &io) {
    int32_t *viol = io_host<int32_t>(io, HEAD_POLL) + 1;   // (beside the "still running" word)
    HIPCHK(hipMemcpyAsync(viol, dev_.span_viol, sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    if (const int rc = sync_call()) return rc;
    if (*viol == 0) return CTVIO_OK;
    const int n = *viol;
    HIPCHK(hipMemsetAsync(dev_.span_viol, 0, sizeof(int32_t), stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    return fail(CTVIO_ERR_INTERNAL, std::to_string(n) + " evaluation(s) fell outside the planned knot span of their landmark (host_pack.hpp: plan_sparsity): "
                                    "the normal equations of this call are not to be trusted");
  }
  int publish_timing(Timing &t, int passes) {   // (the stream is idle)
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev_[EV_CALL_BEGIN], ev_[EV_CALL_END]));
    t.ms[7] = ms; t.n[7] = passes;
    timing_ = t;
    return CTVIO_OK;
  }

  int solve(int max_iters, ctvio_summary *out) {
    if (const int rc = guard()) return rc;
    if (max_iters < 0) return fail(CTVIO_ERR_INVALID, "max_iterations < 0");
    Dev &d = dev_;
    const int nw = d.nwin;
    CallLayout io = head_;
    if (const int rc = reserve_call(io)) return rc;
    Lm *lm = io_host<Lm>(io, HEAD_LM);   // pinned: the copy does not stage through a runtime bounce buffer
    int32_t *na = io_host<int32_t>(io, HEAD_POLL);
    set_params(max_iters);
    profiling_ = profiling_requested_;
    if (profiling_) plan_ = make_plan(true);   // (every kernel apart; the upload's plan comes back below)
    pev_phase_.clear(); pev_used_ = 0;
    const bool graph = opt_.use_graph && !profiling_ && !d.dbg;
    if (graph) { const int rc = ensure_graph(); if (rc != CTVIO_OK) return rc; }
    HIPCHK(hipEventRecord(ev_[EV_CALL_BEGIN], stream_));
    launch_initial(opt_.initial_radius);
    HIPCHK(hipMemsetAsync(d.n_active, 0, sizeof(int32_t), stream_));
    hipLaunchKernelGGL(k_begin_iter, dim3(nw), dim3(256), 0, stream_, d);   // the first iteration; later ones start in k_pass_end
    // max_iters passes finish every window that never enters the line search; the host looks at the "windows that start another
    // pass" counter every check_every passes and keeps launching while any is left
    const int check = std::max(1, opt_.check_every);
    const int pass_cap = (max_iters + 1) * 22 + 4;   // every LM iteration may take up to 20 trial steps + 1 re-evaluation
    int it = 0;
    for (;;) {
      if (graph) HIPCHK(hipGraphLaunch(graph_exec_, stream_)); else launch_pass();
      ++it;
      if (it >= pass_cap) break;
      if (it >= max_iters || it % check == 0) {
        HIPCHK(hipMemcpyAsync(na, d.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
        HIPCHK(hipStreamSynchronize(stream_));
        if (*na == 0) break;
      }
    }
    HIPCHK(hipEventRecord(ev_[EV_CALL_END], stream_));
    HIPCHK(hipMemcpyAsync(lm, d.lm, sizeof(Lm) * nw, hipMemcpyDeviceToHost, stream_));
    if (const int rc = finish_call(io)) return rc;
    Timing t;
    t.clear();
    if (profiling_) { ph_collect(t); plan_ = make_plan(false); }
    profiling_ = false;
    if (const int rc = publish_timing(t, it)) return rc;
    if (d.dbg) {
      long long st[128];
      HIPCHK(hipMemcpy(st, d.dbg, sizeof st, hipMemcpyDeviceToHost));
      std::fprintf(stderr, "[ctvio] imu fast body, group 5000, clock64 deltas (prologue | per pass: loads+values, gyro jac, gyro rows+MFMA, accel jac, accel rows+MFMA | .. | epilogue):");
      for (int i = 65; i < 64 + 16 && st[i] != 0; ++i) std::fprintf(stderr, " %lld", st[i] - st[i - 1]);
      std::fprintf(stderr, "\n");
      std::fprintf(stderr, "[ctvio] cholesky clock64 deltas:");
      for (int i = 1; i < 30 && st[i] != 0; ++i) std::fprintf(stderr, " %lld", st[i] - st[i - 1]);
      std::fprintf(stderr, "\n[ctvio] vis_eval<LIN> wave 1000, clock64 deltas (evaluation | contributions + segmented sums | record copy-out | per sweep: scatter, rows out):");
      for (int i = 32; i < 40; ++i) std::fprintf(stderr, " %lld", st[i] - st[i - 1]);
      std::fprintf(stderr, " | landmarks %lld, rows per sweep %lld", st[42] / 1000000, st[43] / 1000);
      std::fprintf(stderr, "\n[ctvio] schur_window clock64 deltas (prologue + first chunk staged | the chunk loop | product tiles out | other tiles out):");
      for (int i = 97; i < 128 && st[i] != 0; ++i) std::fprintf(stderr, " %lld", st[i] - st[i - 1]);
      std::fprintf(stderr, "\n[ctvio] assemble_vis clock64 deltas (zero | per item of rounds 0, 1: staged, run products.., scatter | rounds | imu tiles | H flush | g flush):");
      for (int i = 49; i < 63; ++i) std::fprintf(stderr, " %lld", st[i] - st[i - 1]);
      std::fprintf(stderr, "\n");
    }
    if (out)
      for (int w = 0; w < nw; ++w) {
        out[w].iterations = lm[w].iter; out[w].num_successful = lm[w].nsucc; out[w].num_unsuccessful = lm[w].nunsucc;
        out[w].termination = lm[w].status > 0 ? lm[w].status - 1 : 0;
        out[w].initial_cost = lm[w].initial_cost; out[w].final_cost = lm[w].cost; out[w].final_radius = lm[w].mu;
        out[w].num_line_search_steps = lm[w].nls_steps; out[w].num_line_search_reduced = lm[w].nls_reduced;
      }
    return CTVIO_OK;
  }

  int get_state(int id, double *quat, double *pos, double *bias, double *rho, double *ld) {
    if (const int rc = guard(id)) return rc;
    const WinMeta &m = meta_[id];
    if (quat) HIPCHK(hipMemcpyAsync(quat, dev_.quat + 4 * (size_t)m.knot0, sizeof(double) * 4 * m.K, hipMemcpyDeviceToHost, stream_));
    if (pos) HIPCHK(hipMemcpyAsync(pos, dev_.pos + 3 * (size_t)m.knot0, sizeof(double) * 3 * m.K, hipMemcpyDeviceToHost, stream_));
    if (bias) HIPCHK(hipMemcpyAsync(bias, dev_.bias + 6 * (size_t)m.bias0, sizeof(double) * 6 * m.F, hipMemcpyDeviceToHost, stream_));
    if (rho && m.L) HIPCHK(hipMemcpyAsync(rho, dev_.rho + m.lm0, sizeof(double) * m.L, hipMemcpyDeviceToHost, stream_));
    if (ld) HIPCHK(hipMemcpyAsync(ld, dev_.ld + id, sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    return CTVIO_OK;
  }
  int set_state(int id, const double *quat, const double *pos, const double *bias, const double *rho, double ld) {
    if (const int rc = guard(id)) return rc;
    const WinMeta &m = meta_[id];
    if (!m.fix_ld) ld = std::min(std::max(ld, m.ld_lo), m.ld_hi);
    else if (ld != h_ld_[id]) return fail(CTVIO_ERR_INVALID, "the line delay of a fix_ld window cannot change after the upload: the knot spans of its landmarks were planned for it");
    if (quat) HIPCHK(hipMemcpyAsync(dev_.quat + 4 * (size_t)m.knot0, quat, sizeof(double) * 4 * m.K, hipMemcpyHostToDevice, stream_));
    if (pos) HIPCHK(hipMemcpyAsync(dev_.pos + 3 * (size_t)m.knot0, pos, sizeof(double) * 3 * m.K, hipMemcpyHostToDevice, stream_));
    if (bias) HIPCHK(hipMemcpyAsync(dev_.bias + 6 * (size_t)m.bias0, bias, sizeof(double) * 6 * m.F, hipMemcpyHostToDevice, stream_));
    if (rho && m.L) HIPCHK(hipMemcpyAsync(dev_.rho + m.lm0, rho, sizeof(double) * m.L, hipMemcpyHostToDevice, stream_));
    HIPCHK(hipMemcpyAsync(dev_.ld + id, &ld, sizeof(double), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    return CTVIO_OK;
  }

  // device-side copy of the whole batch state (restore != 0: copy back); the state is one contiguous block
  int snapshot(int restore) {
    if (const int rc = guard()) return rc;
    if (restore && !snap_valid_) return fail(CTVIO_ERR_STATE, "no snapshot taken");
    HIPCHK(hipMemcpyAsync(restore ? dev_.quat : snap_, restore ? snap_ : dev_.quat, state_doubles_ * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    if (!restore) { HIPCHK(hipStreamSynchronize(stream_)); snap_valid_ = true; }
    return CTVIO_OK;
  }
  // every window's state in one device-to-host copy (concatenated in window order, like the device arrays)
  int get_batch_state(double *quat, double *pos, double *bias, double *rho, double *ld) {
    if (const int rc = guard()) return rc;
    const Dev &d = dev_;
    CallLayout io = head_;
    if (const int rc = reserve_call(io)) return rc;
    double *p = io_host<double>(io, HEAD_STATE);
    HIPCHK(hipMemcpyAsync(p, d.quat, state_doubles_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    const std::pair<double *, size_t> dst[] = {{quat, (size_t)4 * d.Ktot}, {pos, (size_t)3 * d.Ktot}, {bias, (size_t)6 * d.Ftot}, {rho, (size_t)d.Ltot}, {ld, (size_t)d.nwin}};
    for (const auto &x : dst) { if (x.first && x.second) std::memcpy(x.first, p, sizeof(double) * x.second); p += x.second; }
    return CTVIO_OK;
  }

  int linearize(int id, double *Hpp, double *W, double *Hll, double *g, double *cost) {
    if (const int rc = guard(id)) return rc;
    Dev &d = dev_;
    const WinMeta &m = meta_[id];
    const size_t P = (size_t)m.P, L = (size_t)m.L, nW = W ? (size_t)m.Lpad * m.ldw : 0;
    CallLayout io = head_;
    io.landing();   // (W comes as the device keeps it: Lpad sorted rows of ldw)
    const int s_h = io.add("Hpp", sizeof(double), Hpp ? P * P : 0, false), s_w = io.add("W", sizeof(double), L ? nW : 0, false),
              s_l = io.add("Hll", sizeof(double), Hll ? L : 0, false), s_g = io.add("g", sizeof(double), g ? (size_t)m.N : 0, false);
    if (const int rc = reserve_call(io)) return rc;
    double *hH = io_host<double>(io, s_h), *hW = io_host<double>(io, s_w), *hL = io_host<double>(io, s_l), *hg = io_host<double>(io, s_g);
    Lm *lm = io_host<Lm>(io, HEAD_LM) + id;
    set_params(1);
    launch_initial(opt_.initial_radius);
    if (Hpp) {
      HIPCHK(hipMemcpy2DAsync(hH, sizeof(double) * P, d.HppS[0] + m.H0, sizeof(double) * (size_t)m.ldh, sizeof(double) * P, P, hipMemcpyDeviceToHost, stream_));
    }
    if (W && L) HIPCHK(hipMemcpyAsync(hW, d.WS[0] + m.W0, sizeof(double) * nW, hipMemcpyDeviceToHost, stream_));
    if (Hll && L) HIPCHK(hipMemcpyAsync(hL, d.HllS[0] + m.lm0, sizeof(double) * L, hipMemcpyDeviceToHost, stream_));
    if (g) HIPCHK(hipMemcpyAsync(hg, d.gS[0] + m.u0, sizeof(double) * m.N, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(lm, d.lm + id, sizeof(Lm), hipMemcpyDeviceToHost, stream_));
    if (const int rc = finish_call(io)) return rc;
    if (Hpp)   // (the device keeps the lower triangle)
      for (size_t i = 0; i < P; ++i)
        for (size_t j = 0; j < P; ++j) Hpp[i * P + j] = j <= i ? hH[i * P + j] : hH[j * P + i];
    if (W && L)
      for (size_t i = 0; i < P; ++i)
        for (size_t l = 0; l < L; ++l) W[i * L + l] = hW[(size_t)h_lm_pos_[m.lm0 + l] * m.ldw + i];   // (rows of W: sorted landmark order)
    if (Hll && L) std::memcpy(Hll, hL, sizeof(double) * L);
    if (g) std::memcpy(g, hg, sizeof(double) * m.N);
    if (cost) *cost = lm->cost;
    return CTVIO_OK;
  }
  int cost(int id, double *cost) {
    if (const int rc = guard(id)) return rc;
    Dev &d = dev_;
    CallLayout io = head_;
    if (const int rc = reserve_call(io)) return rc;
    Lm *lm = io_host<Lm>(io, HEAD_LM) + id;
    set_params(1);
    launch_prepare(opt_.initial_radius, 1);
    launch_evaluate(COST_AT_X);
    hipLaunchKernelGGL(k_misc, dim3(d.nwin), dim3(256), std::max(d.maxPn, 1) * sizeof(double), stream_, d, (int)COST_AT_X, 0, 0);
    hipLaunchKernelGGL(k_initial_cost, dim3(d.nwin), dim3(64), 0, stream_, d, 1);
    HIPCHK(hipMemcpyAsync(lm, d.lm + id, sizeof(Lm), hipMemcpyDeviceToHost, stream_));
    if (const int rc = finish_call(io)) return rc;
    if (cost) *cost = lm->cand_cost;
    return CTVIO_OK;
  }
  int lm_step(int id, double mu, double *delta, double *mc) {
    if (const int rc = guard(id)) return rc;
    Dev &d = dev_;
    const WinMeta &m = meta_[id];
    CallLayout io = head_;
    io.landing();
    const int s_d = io.add("delta", sizeof(double), delta ? (size_t)m.N : 0, false);
    if (const int rc = reserve_call(io)) return rc;
    Lm *lm = io_host<Lm>(io, HEAD_LM) + id;
    set_params(1);
    launch_initial(mu);
    HIPCHK(hipMemsetAsync(d.n_active, 0, sizeof(int32_t), stream_));
    hipLaunchKernelGGL(k_begin_iter, dim3(d.nwin), dim3(256), 0, stream_, d);
    launch_step();
    if (delta) HIPCHK(hipMemcpyAsync(io_host<double>(io, s_d), d.delta + m.u0, sizeof(double) * m.N, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(lm, d.lm + id, sizeof(Lm), hipMemcpyDeviceToHost, stream_));
    if (const int rc = finish_call(io)) return rc;
    if (delta) std::memcpy(delta, io_host<double>(io, s_d), sizeof(double) * m.N);
    if (mc) *mc = lm->step_valid ? lm->model_change : -1.0;
    return CTVIO_OK;
  }
  // Prior construction, all on the device: A, b of every window's factors by the linearise kernels, then one
  // workgroup per window eliminates the marginalised unknowns and factors the rest (csrc/marg_device.hpp: parallel Jacobi
  // in LDS).  role: concatenated per window (sum N entries, window i at its unknown offset); `only` >= 0 restricts the work
  // to that window.  Outputs: n_keep[nwin]; kept at the window's unknown offset; J0 / r0 packed tightly in window order.
  // allow_blocked: windows with m or n in (MARG_MAXD, MARG_MAXD_BLOCKED] take the blocked path (csrc/marg_blocked.hpp, one window
  // after the other, after the in-LDS launch of the small ones); without it they are reported too large.
  struct MargResult {   // too_large: a window is beyond what the call may take (rc is CTVIO_OK, nothing computed); stalled: the window
    int rc; bool too_large = false; int stalled = -1;   // whose eigen-solver did not converge (rc is an error then), or -1
    MargResult(int rc_ = CTVIO_OK) : rc(rc_) {}
  };
  struct BlockedMeta { int w; MargMeta mm; };
  struct MbBase {   // where the blocked path works: one window's scratch at a time (mb_scratch), the per-block sweep mass and its mirror, the call's lists
    char *scr; double *mass, *mass_host; int32_t *rank; const int32_t *idx; double *out;
  };
  MargResult marg_device(const int8_t *role_all, int only, double eps, int32_t *n_keep, int32_t *kept, double *J0, double *r0, bool allow_blocked) {
    MargResult res;
    Dev &d = dev_;
    const int nw = d.nwin;
    std::vector<MargMeta> metas((size_t)nw);
    std::vector<BlockedMeta> bmeta;   // the blocked windows (k_marginalize sees them with m = n = 0)
    std::vector<int32_t> iscr;
    // scr: A / V / X / Y / rot / b of every in-LDS window (MargMeta keeps their offsets in doubles), then the blocked path's scratch, sized for
    // its largest window, and rank vector.  io: descriptors and index lists (in), J0 | r0 of every window packed as the caller gets them,
    // and the blocked path's per-block mass (out: the host reads it after every sweep).
    CallLayout io = head_, scr;
    size_t outd = 0, mb_bytes = 0;
    int mb_D = 0, mb_n = 0;
    for (int w = 0; w < nw; ++w) {
      const WinMeta &m = meta_[w];
      MargMeta &mm = metas[w];
      std::memset(&mm, 0, sizeof mm);
      mm.N = m.N;
      if (only >= 0 && w != only) { n_keep[w] = 0; continue; }
      const int8_t *role = role_all + m.u0;
      mm.idx0 = (int32_t)iscr.size();
      for (int i = 0; i < m.N; ++i) if (role[i] == 1) { iscr.push_back(i); mm.m++; }
      for (int i = 0; i < m.N; ++i) if (role[i] == 0) { iscr.push_back(i); kept[m.u0 + mm.n] = i; mm.n++; }
      n_keep[w] = mm.n;
      const bool big = mm.m > MARG_MAXD || mm.n > MARG_MAXD;
      if (mm.m > MARG_MAXD_BLOCKED || mm.n > MARG_MAXD_BLOCKED || (big && !allow_blocked)) { res.too_large = true; return res; }
      mm.J0 = (int64_t)outd; outd += (size_t)mm.n * mm.n;
      mm.r0 = (int64_t)outd; outd += (size_t)mm.n;
      if (allow_blocked && mm.n > 0 && (big || dbg_.marg_blocked)) {
        bmeta.push_back({w, mm});
        MbWin b = mb_window(w, mm);
        mb_bytes = std::max(mb_bytes, mb_scratch(b, nullptr, nullptr));
        mb_D = std::max(mb_D, std::max(b.dm, b.dn)); mb_n = std::max(mb_n, b.n);
        mm.m = mm.n = 0;
        continue;
      }
      const int np = std::max(mm.m, mm.n) + (std::max(mm.m, mm.n) & 1);
      const size_t mn1 = (size_t)mm.m * (mm.n + 1);
      const std::pair<int64_t *, size_t> segs[] = {{&mm.A0, (size_t)m.N * m.N}, {&mm.V0, (size_t)mm.m * mm.m}, {&mm.X0, mn1}, {&mm.Y0, mn1},
                                                   {&mm.rot0, (size_t)MARG_MAX_SWEEPS * std::max(np - 1, 1) * (np / 2) * 2}, {&mm.b0, (size_t)mm.n}};
      for (const auto &sg : segs) *sg.first = (int64_t)(scr.off(scr.add("marg", sizeof(double), sg.second, true)) / sizeof(double));
    }
    if (iscr.empty()) iscr.push_back(0);
    const int s_mb = scr.add("mb", 1, mb_bytes, true), s_rank = scr.add("rank", sizeof(int32_t), (size_t)mb_n, false);
    const int s_meta = io.add("meta", sizeof(MargMeta), (size_t)nw, false), s_idx = io.add("idx", sizeof(int32_t), iscr.size(), false),
              s_out = io.add("out", sizeof(double), outd, true), s_mass = io.add("mass", sizeof(double), (size_t)2 * mb_D / MB_BLK, true);
    if (const int rc = reserve_call(io, &scr)) return rc;
    MargMeta *hmeta = io_host<MargMeta>(io, s_meta), *dmeta = io_dev<MargMeta>(io, s_meta);
    const MbBase mb{scr.at<char>(call_scr_.dev, s_mb), io_dev<double>(io, s_mass), io_host<double>(io, s_mass), scr.at<int32_t>(call_scr_.dev, s_rank),
                    io_dev<int32_t>(io, s_idx), io_dev<double>(io, s_out)};
    // normal equations of every window at its current state
    set_params(1);
    launch_initial(opt_.initial_radius);
    std::memcpy(hmeta, metas.data(), sizeof(MargMeta) * nw);
    std::memcpy(io_host<int32_t>(io, s_idx), iscr.data(), sizeof(int32_t) * iscr.size());
    HIPCHK(hipMemcpyAsync(dmeta, hmeta, io.off(s_out) - io.off(s_meta), hipMemcpyHostToDevice, stream_));   // (meta | idx)
    if (!marg_attr_set_) { HIPCHK(hipFuncSetAttribute((const void *)k_marginalize, hipFuncAttributeMaxDynamicSharedMemorySize, MARG_LDS_LIMIT)); marg_attr_set_ = true; }
    if (bmeta.size() < (size_t)nw)
      hipLaunchKernelGGL(k_marginalize, dim3(nw), dim3(256), MargLds::BYTES, stream_, d, dmeta, mb.idx, reinterpret_cast<double *>(call_scr_.dev), mb.out, eps);
    for (BlockedMeta &b : bmeta) {
      const int rc = marg_blocked(b.w, b.mm, eps, mb);
      if (rc != CTVIO_OK) return rc;
      metas[b.w] = b.mm;
    }
    const double *outh = io_host<double>(io, s_out);
    if (outd) HIPCHK(hipMemcpyAsync((void *)outh, mb.out, sizeof(double) * outd, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(hmeta, dmeta, sizeof(MargMeta) * nw, hipMemcpyDeviceToHost, stream_));
    if (const int rc = finish_call(io)) return rc;
    for (int w = 0; w < nw; ++w) if (hmeta[w].n > 0) metas[w] = hmeta[w];
    size_t oj = 0, orr = 0;
    for (int w = 0; w < nw; ++w) {
      const MargMeta &mm = metas[w];
      if (mm.n <= 0) continue;
      if (dbg_.marg_debug && w == (only >= 0 ? only : 0)) {
        std::fprintf(stderr, "[ctvio] marg window %d: m %d n %d sweeps %d / %d; off/dia per sweep (A'):", w, mm.m, mm.n, mm.sweeps_m, mm.sweeps_n);
        for (int i = 0; i < JACOBI_TRACE && i <= std::max(mm.sweeps_n, 0) + 1; ++i) std::fprintf(stderr, " %.2e", mm.trace[JACOBI_TRACE + i]);
        std::fprintf(stderr, "\n");
      }
      if (mm.status) { res.stalled = w; res.rc = fail(CTVIO_ERR_HIP, "device eigen-solver did not converge (window " + std::to_string(w) + ")"); return res; }
      std::memcpy(J0 + oj, outh + mm.J0, sizeof(double) * (size_t)mm.n * mm.n);
      std::memcpy(r0 + orr, outh + mm.r0, sizeof(double) * (size_t)mm.n);
      oj += (size_t)mm.n * mm.n; orr += (size_t)mm.n;
    }
    return res;
  }
  // Block two-sided Jacobi (csrc/marg_blocked.hpp) on B (D x D, nd real rows / columns) and V, one launch per phase; the host reads the
  // per-block mass after every sweep and applies jacobi_converged (csrc/jacobi_core.hpp).  *sweeps: the sweeps done, or -1; off / diagonal mass per sweep in trace.
  int mb_jacobi(double *B, double *V, int D, int nd, double *Q, const MbBase &mb, double *trace, int32_t *sweeps) {
    const int nb = D / MB_BLK, npair = nb / 2;
    const double *part = mb.mass_host;
    double prev_off = 1e300;
    *sweeps = -1;
    for (int sweep = 0; sweep < MB_MAX_SWEEPS; ++sweep) {
      hipLaunchKernelGGL(k_mb_mass, dim3(nb), dim3(256), 0, stream_, B, D, mb.mass);
      HIPCHK(hipMemcpyAsync(mb.mass_host, mb.mass, sizeof(double) * 2 * nb, hipMemcpyDeviceToHost, stream_));
      HIPCHK(hipStreamSynchronize(stream_));
      double off = 0.0, d2 = 0.0;
      for (int b = 0; b < nb; ++b) { off += part[2 * b]; d2 += part[2 * b + 1]; }
      if (sweep < JACOBI_TRACE) trace[sweep] = off / d2;
      if (jacobi_converged(off, d2, nd, sweep, prev_off)) { *sweeps = sweep; return CTVIO_OK; }
      prev_off = off;
      for (int s = 0; s < nb - 1; ++s) {
        hipLaunchKernelGGL(k_mb_pair, dim3(npair), dim3(256), 0, stream_, B, D, s, Q);
        hipLaunchKernelGGL(k_mb_update, dim3(npair * (npair - 1) / 2 + (D / 64) * npair), dim3(256), 0, stream_, B, V, D, s, Q);
      }
      HIPCHK(hipGetLastError());
    }
    return CTVIO_OK;
  }
  static MbWin mb_window(int w, const MargMeta &bm) {
    MbWin b{};
    b.w = w; b.m = bm.m; b.n = bm.n; b.dm = bm.m > 0 ? mb_padded(bm.m) : 0; b.dn = mb_padded(bm.n);
    return b;
  }
  // The scratch of one blocked window, every segment once -- a layout of its own inside the call's "mb" segment: points b and *Q (the Q of a
  // step's block pairs) into base and returns the bytes used; base = nullptr gives the size alone.
  static size_t mb_scratch(MbWin &b, char *base, double **Q) {
    const size_t dm2 = (size_t)b.dm * b.dm, dn2 = (size_t)b.dn * b.dn, mn1 = (size_t)b.m * (b.n + 1);
    const std::pair<double **, size_t> segs[] = {{&b.Bm, dm2}, {&b.Vm, dm2}, {&b.Bn, dn2}, {&b.Vn, dn2}, {&b.G, mn1}, {&b.Y, mn1}, {&b.X, mn1},
                                                 {&b.bp, (size_t)b.n}, {Q, (size_t)(std::max(b.dm, b.dn) / 64) * 64 * 64}};
    CallLayout l;
    for (const auto &sg : segs) l.add("mb", sizeof(double), sg.second, true);
    if (base) {
      l.reserved();
      for (size_t k = 0; k < sizeof segs / sizeof segs[0]; ++k) *segs[k].first = l.at<double>(base, (int)k);
    }
    return l.bytes();
  }
  // one window through the blocked path, in the call's reservation; J0 / r0 to mb.out at bm's offsets, status and sweeps into bm
  int marg_blocked(int w, MargMeta &bm, double eps, const MbBase &mb) {
    MbWin b = mb_window(w, bm);
    const int m = b.m, n = b.n, dm = b.dm, dn = b.dn;
    const size_t mn1 = (size_t)m * (n + 1);
    double *Q;
    const size_t need = mb_scratch(b, mb.scr, &Q);
    // (CTVIO_POISON: every window starts on the pattern, not on the previous window's numbers)
    HIPCHK(poison(mb.scr, need));
    HIPCHK(poison(mb.mass, sizeof(double) * 2 * std::max(dm, dn) / MB_BLK));
    b.im = mb.idx + bm.idx0; b.ik = b.im + m;
    b.J0 = mb.out + bm.J0; b.r0 = mb.out + bm.r0; b.rank = mb.rank;
    auto grid = [](long long cnt) { return dim3((unsigned)std::max<long long>(1, (cnt + 255) / 256)); };
    const long long gat = std::max<long long>((long long)dm * dm, std::max<long long>((long long)mn1, (long long)dn * dn));
    hipLaunchKernelGGL(k_mb_gather, dim3((unsigned)std::min<long long>(2048, (gat + 255) / 256)), dim3(256), 0, stream_, dev_, b);
    int status = 0;
    bm.sweeps_m = 0;
    if (m > 0) {
      if (const int rc = mb_jacobi(b.Bm, b.Vm, dm, m, Q, mb, bm.trace, &bm.sweeps_m)) return rc;
      if (bm.sweeps_m < 0) status = 1;
      hipLaunchKernelGGL(k_mb_y, grid((long long)mn1), dim3(256), 0, stream_, b, eps);
      hipLaunchKernelGGL(k_mb_x, grid((long long)mn1), dim3(256), 0, stream_, b);
    }
    hipLaunchKernelGGL(k_mb_reduce, grid((long long)dn * dn + n), dim3(256), 0, stream_, dev_, b);
    if (const int rc = mb_jacobi(b.Bn, b.Vn, dn, n, Q, mb, bm.trace + JACOBI_TRACE, &bm.sweeps_n)) return rc;
    if (bm.sweeps_n < 0) status = 1;
    hipLaunchKernelGGL(k_mb_rank, grid(n), dim3(256), 0, stream_, b, eps);
    hipLaunchKernelGGL(k_mb_j0, grid((long long)n * n), dim3(256), 0, stream_, b, eps);
    HIPCHK(hipGetLastError());
    bm.status = status;
    return CTVIO_OK;
  }
  int marginalize_batch(const int8_t *role, double eps, int32_t *n_keep, int32_t *kept, double *J0, double *r0) {
    if (const int rc = guard()) return rc;
    if (!role || !n_keep || !kept || !J0 || !r0 || !(eps >= 0)) return fail(CTVIO_ERR_INVALID, "bad arguments");
    for (int i = 0; i < dev_.Utot; ++i) if (role[i] < -1 || role[i] > 1) return fail(CTVIO_ERR_INVALID, "role must be -1, 0 or 1");
    marg_ran_on_host_ = 0;
    const MargResult r = marg_device(role, -1, eps, n_keep, kept, J0, r0, true);
    if (r.stalled >= 0)
      return fail(CTVIO_ERR_HIP, "device eigen-solver did not converge for window " + std::to_string(r.stalled) + ": call ctvio_marginalize for it (host factorisation)");
    if (r.rc != CTVIO_OK) return r.rc;
    if (r.too_large) return fail(CTVIO_ERR_INVALID, "a window has more than " + std::to_string(MARG_MAXD_BLOCKED) + " marginalised or kept unknowns");
    return CTVIO_OK;
  }
  // one window; windows beyond the device eigen-solver's size (m or n > MARG_MAXD) take the host path (csrc/marginalize.hpp)
  int marginalize(int id, const int8_t *role, double eps, int32_t *n_keep, int32_t *kept, double *J0, double *r0) {
    if (const int rc = guard(id)) return rc;
    if (!role || !n_keep || !kept || !J0 || !r0 || !(eps >= 0)) return fail(CTVIO_ERR_INVALID, "bad arguments");
    const WinMeta &m = meta_[id];
    const int N = m.N, P = m.P, L = m.L;
    for (int i = 0; i < N; ++i) if (role[i] < -1 || role[i] > 1) return fail(CTVIO_ERR_INVALID, "role must be -1, 0 or 1");
    marg_ran_on_host_ = 0;
    if (!dbg_.marg_host) {
      std::vector<int8_t> role_all((size_t)dev_.Utot, (int8_t)-1);
      std::copy(role, role + N, role_all.begin() + m.u0);
      std::vector<int32_t> nk((size_t)dev_.nwin), kv((size_t)dev_.Utot);
      const MargResult r = marg_device(role_all.data(), id, eps, nk.data(), kv.data(), J0, r0, false);
      if (r.rc != CTVIO_OK && r.stalled < 0) return r.rc;
      // the in-LDS Jacobi sweep stalled above its (tight) off-diagonal bound: the host Householder / QL path below takes over
      if (r.rc == CTVIO_OK && !r.too_large) {
        *n_keep = nk[id];
        std::copy(kv.begin() + m.u0, kv.begin() + m.u0 + nk[id], kept);
        return CTVIO_OK;
      }
    }
    // Host leg (csrc/marginalize.hpp: Householder tridiagonalisation + QL on the host cores; the normal equations still come from the device
    // kernels): taken when the window is beyond the device eigen-solver's size, when its Jacobi sweeps stalled, or when forced.  The caller
    // can tell: ctvio_marginalize_ran_on_host.
    marg_ran_on_host_ = 1;
    std::vector<double> Hpp((size_t)P * P), W((size_t)P * std::max(L, 1)), Hll(std::max(L, 1)), g(N);
    const int rc = linearize(id, Hpp.data(), L ? W.data() : nullptr, L ? Hll.data() : nullptr, g.data(), nullptr);
    if (rc != CTVIO_OK) return rc;
    std::vector<double> A((size_t)N * N, 0.0);
    for (int i = 0; i < P; ++i) {
      for (int j = 0; j < P; ++j) A[(size_t)i * N + j] = Hpp[(size_t)i * P + j];
      for (int l = 0; l < L; ++l) { A[(size_t)i * N + P + l] = W[(size_t)i * L + l]; A[(size_t)(P + l) * N + i] = W[(size_t)i * L + l]; }
    }
    for (int l = 0; l < L; ++l) A[(size_t)(P + l) * N + P + l] = Hll[l];
    std::vector<int32_t> kv;
    std::vector<double> Jv, rv;
    const int n = marginalize_dense(N, A.data(), g.data(), role, eps, kv, Jv, rv);
    *n_keep = n;
    std::copy(kv.begin(), kv.end(), kept);
    std::copy(Jv.begin(), Jv.end(), J0);
    std::copy(rv.begin(), rv.end(), r0);
    return CTVIO_OK;
  }
  // ResidualSummary (reference trajectory_estimator.h:37-59): per-type sums of |r_i| at the current state
  int residual_summary(int id, double *sums, int32_t *counts4) {
    if (const int rc = guard(id, "bad arguments")) return rc;
    if (!sums) return fail(CTVIO_ERR_INVALID, "bad arguments");
    const WinMeta &m = meta_[id];
    const size_t n = (size_t)14 + m.pn;
    CallLayout io = head_;
    const int s_out = io.add("sums", sizeof(double), n + 1, true);   // (+ the number of active visual blocks)
    if (const int rc = reserve_call(io)) return rc;
    hipLaunchKernelGGL(k_residual_summary, dim3(1), dim3(256), (size_t)(14 + 2 * m.pn) * sizeof(double), stream_, dev_, id, io_dev<double>(io, s_out));
    HIPCHK(hipMemcpyAsync(io_host<double>(io, s_out), io_dev<double>(io, s_out), sizeof(double) * (n + 1), hipMemcpyDeviceToHost, stream_));
    if (const int rc = sync_call()) return rc;
    std::memcpy(sums, io_host<double>(io, s_out), sizeof(double) * n);
    if (counts4) { counts4[0] = m.M; counts4[1] = m.NB; counts4[2] = (int32_t)io_host<double>(io, s_out)[n]; counts4[3] = m.pn > 0 ? 1 : 0; }
    return CTVIO_OK;
  }
  int gauge_restore(int n, const int32_t *ids, const int32_t *knot, const double *q0, const double *t0) {
    if (const int rc = guard()) return rc;
    if (n < 0 || (n && (!ids || !knot || !q0 || !t0))) return fail(CTVIO_ERR_INVALID, "bad arguments");
    for (int i = 0; i < n; ++i) {
      if (ids[i] < 0 || ids[i] >= dev_.nwin) return fail(CTVIO_ERR_INVALID, "window id out of range");
      if (knot[i] < 0 || knot[i] >= meta_[ids[i]].K) return fail(CTVIO_ERR_INVALID, "knot index out of range");
      for (int j = 0; j < i; ++j) if (ids[j] == ids[i]) return fail(CTVIO_ERR_INVALID, "window listed twice");
    }
    if (n == 0) return CTVIO_OK;
    // one staged copy: [ids | knot], then [q0 | t0]
    const size_t nn = (size_t)n;
    CallLayout io = head_;
    const int s_i = io.add("ids_knot", sizeof(int32_t), 2 * nn, false), s_p = io.add("q0_t0", sizeof(double), 7 * nn, false);
    if (const int rc = reserve_call(io)) return rc;
    int32_t *hi = io_host<int32_t>(io, s_i), *di = io_dev<int32_t>(io, s_i);
    double *hp = io_host<double>(io, s_p), *dp = io_dev<double>(io, s_p);
    std::memcpy(hi, ids, sizeof(int32_t) * nn); std::memcpy(hi + nn, knot, sizeof(int32_t) * nn);
    std::memcpy(hp, q0, sizeof(double) * 4 * nn); std::memcpy(hp + 4 * nn, t0, sizeof(double) * 3 * nn);
    HIPCHK(hipMemcpyAsync(di, hi, io.bytes() - io.off(s_i), hipMemcpyHostToDevice, stream_));
    hipLaunchKernelGGL(k_gauge_restore, dim3(n), dim3(64), 0, stream_, dev_, n, di, di + nn, dp, dp + 4 * nn);
    return sync_call();
  }
  // the sensor-to-IMU extrinsic as the kernels take it: the quaternion normalised
  static int sensor_ext(const double *q_SI, const double *p_SI, SensorExt &ext) {
    const double nq = std::sqrt(q_SI[0] * q_SI[0] + q_SI[1] * q_SI[1] + q_SI[2] * q_SI[2] + q_SI[3] * q_SI[3]);
    if (!(nq > 0.0) || !std::isfinite(nq)) return fail(CTVIO_ERR_INVALID, "sensor extrinsic: quaternion must be non-zero and finite");
    for (int i = 0; i < 4; ++i) ext.q[i] = q_SI[i] / nq;
    for (int i = 0; i < 3; ++i) ext.p[i] = p_SI[i];
    ext.on = 1;
    return CTVIO_OK;
  }
  int spline_eval(int id, int n, const int64_t *t_ns, double *pose7, double *vel3, double *omega3, double *acc3, const double *q_SI = nullptr,
                  const double *p_SI = nullptr) {
    SensorExt ext{};
    if (q_SI && p_SI)
      if (const int rc = sensor_ext(q_SI, p_SI, ext)) return rc;
    if (const int rc = guard(id, "bad arguments")) return rc;
    if (n < 0 || (n && !t_ns)) return fail(CTVIO_ERR_INVALID, "bad arguments");
    return spline_query(id, nullptr, n, t_ns, pose7, vel3, omega3, acc3, ext, nullptr);
  }
  // Queries of any windows of the batch in ONE launch (query i: window win[i], absolute time t_ns[i]).
  int spline_eval_batch(int64_t n64, const int32_t *win, const int64_t *t_ns, double *pose7, double *vel3, double *omega3, double *acc3,
                        double *kernel_ms) {
    if (const int rc = guard()) return rc;
    if (!check_count(n64) || (n64 && (!t_ns || !win))) return fail(CTVIO_ERR_INVALID, "bad arguments");
    if (kernel_ms) *kernel_ms = 0.0;
    return spline_query(0, win, (int)n64, t_ns, pose7, vel3, omega3, acc3, SensorExt{}, kernel_ms);
  }
  // n queries of window `id` (win == null, as the kernel takes it) or of the windows win[i]
  int spline_query(int id, const int32_t *win, int n, const int64_t *t_ns, double *pose7, double *vel3, double *omega3, double *acc3,
                   const SensorExt &ext, double *kernel_ms) {
    if (n == 0) return CTVIO_OK;
    // in: relative times, windows (with a window list), the error word; out: the error word again and the outputs the caller asked for
    const size_t nn = (size_t)n;
    double *const out[4] = {pose7, vel3, omega3, acc3};
    const size_t width[4] = {7, 3, 3, 3};
    CallLayout io = head_;
    const int s_rel = io.add("t_rel", sizeof(long long), nn, false), s_win = io.add("win", sizeof(int32_t), win ? nn : 0, false),
              s_err = io.add("err", sizeof(int32_t), 4, false);
    int s_out[4];
    for (int k = 0; k < 4; ++k) s_out[k] = io.add("query_out", sizeof(double), out[k] ? width[k] * nn : 0, true);
    if (const int rc = reserve_call(io)) return rc;
    long long *rel = io_host<long long>(io, s_rel);
    int32_t *hw = io_host<int32_t>(io, s_win);
    int *herr = io_host<int>(io, s_err), *derr = io_dev<int>(io, s_err);
    for (int i = 0; i < n; ++i) {
      if (win && (win[i] < 0 || win[i] >= dev_.nwin)) return fail(CTVIO_ERR_INVALID, "query " + std::to_string(i) + ": window id out of range");
      if (win) hw[i] = win[i];
      rel[i] = (long long)(t_ns[i] - t0_[win ? win[i] : id]);
    }
    *herr = 0;
    HIPCHK(hipMemcpyAsync(io_dev<char>(io, s_rel), rel, io.off(s_out[0]) - io.off(s_rel), hipMemcpyHostToDevice, stream_));
    double *dv[4];
    for (int k = 0; k < 4; ++k) dv[k] = out[k] ? io_dev<double>(io, s_out[k]) : nullptr;
    if (kernel_ms) HIPCHK(hipEventRecord(ev_[EV_QUERY_BEGIN], stream_));
    hipLaunchKernelGGL(k_spline_eval, dim3(nblk(n, 256)), dim3(256), 0, stream_, dev_, id, win ? io_dev<int32_t>(io, s_win) : nullptr, n,
                       io_dev<long long>(io, s_rel), dv[0], dv[1], dv[2], dv[3], derr, ext);
    if (kernel_ms) HIPCHK(hipEventRecord(ev_[EV_QUERY_END], stream_));
    HIPCHK(hipMemcpyAsync(herr, derr, io.bytes() - io.off(s_err), hipMemcpyDeviceToHost, stream_));   // (err | outputs)
    if (const int rc = sync_call()) return rc;
    if (kernel_ms) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ev_[EV_QUERY_BEGIN], ev_[EV_QUERY_END])); *kernel_ms = ms; }
    for (int k = 0; k < 4; ++k) if (out[k]) std::memcpy(out[k], io_host<double>(io, s_out[k]), sizeof(double) * width[k] * nn);
    if (*herr) return fail(CTVIO_ERR_INVALID, "query time outside the spline");
    return CTVIO_OK;
  }
  // ---------------------------------------------------------------------------------------- marginal covariances
  // ctvio_covariance_batch / ctvio_covariance (only >= 0: that window alone, n_sel / sel / outputs are its own).  The normal equations of the
  // current state (as ctvio_linearize forms them), then Schur complement and panel Cholesky on a COPY of Dev -- per-call activity mask, zero
  // damping, every tile of S written -- and the kernels of csrc/kernels_cov.hpp, in run_query's sequence (below; always full).  The panel
  // kernel launches from the plan like the solve's (launch_chol_panel).  The scratch follows the call's selections, not the upload.
  static constexpr int COV_MAX_SEL = 64;
  // What every full call of run_query starts with: the normal equations at the current state, then the factor of the undamped
  // reduced system on c, the call's copy of Dev.  Records EV_CALL_BEGIN .. EV_COV_SOLVE; the stream is left ready for k_cov_solve.
  int cov_factor(Dev &c, uint8_t *mask, uint8_t *excl) {
    set_params(1);
    HIPCHK(hipEventRecord(ev_[EV_CALL_BEGIN], stream_));
    launch_initial(opt_.initial_radius);
    c = dev_;
    c.schur_plain_in_H = 0;
    c.active = mask;
    HIPCHK(hipEventRecord(ev_[EV_COV_PREPARE], stream_));
    hipLaunchKernelGGL(k_cov_prepare, dim3(dev_.nwin), dim3(256), 0, stream_, dev_, mask, excl);
    HIPCHK(hipEventRecord(ev_[EV_COV_FACTOR], stream_));
    launch_schur(c);
    launch_chol_panel(c);
    HIPCHK(hipEventRecord(ev_[EV_COV_SOLVE], stream_));
    return CTVIO_OK;
  }
  size_t cov_solve_lds() const { return ((size_t)16 * 32 * ((dev_.maxP + 31) / 32) + 512) * sizeof(double); }   // Ys | part (k_cov_solve)
  template <CovInst I> void launch_cov_solve(const Dev &c, size_t ntiles, const CovSolveIO<I> &a) {
    hipLaunchKernelGGL((k_cov_solve<I>), dim3((unsigned)ntiles), dim3(COV_NT), cov_solve_lds(), stream_, c, a);
  }
  // the device times of a call between pairs of its events (the stream is idle): ms[slot] of ctvio_last_timing, one launch each where it ran
  struct Span { int slot; Ev begin, end; bool ran = true; };
  typedef std::initializer_list<Span> Spans;
  int span_timing(Spans spans) {
    Timing t;
    t.clear();
    for (const Span &s : spans) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, ev_[s.begin], ev_[s.end]));
      t.ms[s.slot] = ms; t.n[s.slot] = s.ran ? 1 : 0;
    }
    return publish_timing(t, 0);
  }
  // ---- the entries that factor (covariance .. imu_gate, landmark_points) share what follows.  Each validates its arguments, groups its
  // queries by window (host_pack.hpp: QueryOrder), names its segments ONCE -- what a call without covariances does not need has no elements:
  // io is its inputs (one staged copy), then the outputs (one copy back); the device-only scratch is CovScratch --, fills the host inputs,
  // runs run_query and scatters the mirror into the caller's arrays by status.
  static_assert(POSE_OK == QUERY_OK && POSE_SINGULAR == QUERY_SINGULAR && POSE_UNTOUCHED == QUERY_NO_INFO, "merge_status / fill_not_ok");
  static_assert(LMP_OK == QUERY_OK && LMP_SINGULAR == QUERY_SINGULAR && LMP_NO_INFO == QUERY_NO_INFO, "merge_status / fill_not_ok");
  static_assert(PRJ_OK == QUERY_OK && PRJ_SINGULAR == QUERY_SINGULAR && PRJ_NO_INFO == QUERY_NO_INFO, "merge_status / fill_not_ok");
  static_assert(IMUG_OK == QUERY_OK && IMUG_SINGULAR == QUERY_SINGULAR && IMUG_NO_INFO == QUERY_NO_INFO, "merge_status / fill_not_ok");
  static_assert(GATE_WEAK == IMUG_WEAK, "gate_scatter: one set of codes for the two gates");
  static constexpr GateCodes GATE_CODES{QUERY_OK, GATE_WEAK, QUERY_SINGULAR, QUERY_NO_INFO};
  // the tiles of a covariance query: at most per_tile consecutive sorted queries of one window each
  static std::vector<CovTile> query_tiles(const QueryOrder &ord, int per_tile, CovKind kind) {
    std::vector<CovTile> tiles;
    ord.runs(per_tile, [&](int w, int first, int cnt) { tiles.push_back(CovTile{w, kind, first, cnt, 0}); });
    return tiles;
  }
  // the tiles and (s_slot >= 0: kernels that write into the caller's slots) the sorted order into the mirror; no tiles: values only, neither
  void stage_tiles(const CallLayout &io, int s_slot, int s_tiles, const QueryOrder &ord, const std::vector<CovTile> &tiles) {
    if (tiles.empty()) return;
    if (s_slot >= 0) std::memcpy(io_host<int32_t>(io, s_slot), ord.slot.data(), sizeof(int32_t) * ord.slot.size());
    std::memcpy(io_host<CovTile>(io, s_tiles), tiles.data(), sizeof(CovTile) * tiles.size());
  }
  // What an entry's launches see of the run (run_query).  excl: the exclusions k_cov_prepare left -- null in a values-only call: nothing
  // was factored and there are no records --; rec<Rec>(): the record scratch; c: the factored copy of Dev that k_cov_solve runs on.
  // mark(e) records event e behind what has been launched so far; the first failure is kept and becomes the run's.
  struct QueryRun {
    SolverImpl &self;
    const uint8_t *excl;
    void *records;
    Dev c;
    hipError_t err;
    template <class Rec> Rec *rec() const { return static_cast<Rec *>(records); }
    void mark(Ev e) {
      const hipError_t r = hipEventRecord(self.ev_[e], self.stream_);
      if (err == hipSuccess) err = r;
    }
  };
  // THE run sequence, from "layout reserved, host inputs filled" to "results in the pinned mirror, timing published".  io: the segments
  // [s_in, s_out) go to the device in one copy, [s_out, end) come back in one.  launches(x) queues the entry's kernels in stream order and
  // marks the events its span tables name.
  //   scr null (values only; nothing is linearised or factored): EV_CALL_BEGIN, the copy in, EV_COV_SOLVE where the values table starts
  //     a span there, launches, the copy back, EV_CALL_END, sync_call, span_timing(values).
  //   otherwise: the copy in, cov_factor on the call's copy of Dev (EV_CALL_BEGIN .. EV_COV_SOLVE), launches, EV_CALL_END, the copy back
  //     and the window records (Lm::chol_fail), finish_call, span_timing(full).
  // So a span from EV_COV_SOLVE starts in front of the entry's first launch either way; ms[0] of a full table is k_cov_prepare (span_prepare()).
  // dev_, plan_ and the captured graph are not touched.
  static Span span_prepare() { return {0, EV_COV_PREPARE, EV_COV_FACTOR}; }
  template <class Launches> int run_query(const CallLayout &io, int s_in, int s_out, const CovScratch *scr, Spans values, Spans full, Launches &&launches) {
    const size_t in_bytes = io.off(s_out) - io.off(s_in), out_bytes = io.bytes() - io.off(s_out);
    QueryRun x{*this, nullptr, nullptr, Dev{}, hipSuccess};
    if (!scr) HIPCHK(hipEventRecord(ev_[EV_CALL_BEGIN], stream_));
    if (in_bytes) HIPCHK(hipMemcpyAsync(io_dev<char>(io, s_in), io_host<char>(io, s_in), in_bytes, hipMemcpyHostToDevice, stream_));
    if (scr) {
      x.excl = scr->lay.at<uint8_t>(call_scr_.dev, scr->s_excl);
      x.records = scr->lay.at<char>(call_scr_.dev, scr->s_rec);
      if (const int rc = cov_factor(x.c, scr->lay.at<uint8_t>(call_scr_.dev, scr->s_mask), scr->lay.at<uint8_t>(call_scr_.dev, scr->s_excl))) return rc;
    } else if (std::any_of(values.begin(), values.end(), [](const Span &s) { return s.begin == EV_COV_SOLVE; })) {
      HIPCHK(hipEventRecord(ev_[EV_COV_SOLVE], stream_));   // (an event costs a few microseconds of the call: none that no span reads)
    }
    launches(x);
    HIPCHK(x.err);
    if (scr) HIPCHK(hipEventRecord(ev_[EV_CALL_END], stream_));
    if (out_bytes) HIPCHK(hipMemcpyAsync(io_host<char>(io, s_out), io_dev<char>(io, s_out), out_bytes, hipMemcpyDeviceToHost, stream_));
    if (scr) HIPCHK(hipMemcpyAsync(io_host<Lm>(io, HEAD_LM), dev_.lm, sizeof(Lm) * dev_.nwin, hipMemcpyDeviceToHost, stream_));
    else HIPCHK(hipEventRecord(ev_[EV_CALL_END], stream_));
    if (const int rc = scr ? finish_call(io) : sync_call()) return rc;
    return span_timing(scr ? full : values);
  }
  // The usual launches: jac(x), the entry's record kernel -- after k_cov_prepare in a full call: it reads the exclusions --, then
  // solve(x), its k_cov_solve.  ms[1] k_cov_solve, ms[2] the record kernel (values only: ms[values_slot]).
  template <class Jac, class Solve>
  int run_query(const CallLayout &io, int s_in, int s_out, const CovScratch *scr, Jac &&jac, Solve &&solve, int values_slot = 2) {
    return run_query(io, s_in, s_out, scr, {{values_slot, EV_COV_SOLVE, EV_COV_GRAM}}, {span_prepare(), {1, EV_COV_GRAM, EV_CALL_END}, {2, EV_COV_SOLVE, EV_COV_GRAM}},
                     [&](QueryRun &x) {
                       jac(x);
                       x.mark(EV_COV_GRAM);
                       if (x.excl) solve(x);
                     });
  }
  // The windows [wbeg, wend) of a leave-one-out gate cut into slices of at most `budget` slots (plan_gate_slices; CTVIO_GATE_SLICE
  // overrides the budget), window w holding meta_[w].*count of them: the record scratch is bounded by nrec, the largest slice.
  struct GateSlices {
    std::vector<int32_t> counts;   // by window, the whole batch
    std::vector<GateSlice> slices;
    size_t nrec = 0;
  };
  GateSlices gate_slices(int32_t WinMeta::*count, int wbeg, int wend, size_t budget) const {
    GateSlices g;
    for (const WinMeta &m : meta_) g.counts.push_back(m.*count);
    g.slices = plan_gate_slices(g.counts.data(), wbeg, wend, dbg_.gate_slice > 0 ? (size_t)dbg_.gate_slice : budget);
    for (const GateSlice &sl : g.slices) g.nrec = std::max(g.nrec, (size_t)sl.slots);
    return g;
  }
  // run_query for a gate; slot0: the WinMeta member that holds a window's first slot.  Values only: record(x, s0, nall) over every slot at
  // once and reduce(x), both in ms[2].  Otherwise one factorisation, then per slice record(x, first slot, slots) and solve(x, slice,
  // first slot, slots) -- the first slice's record kernel is the timed one (ms[2]), the later slices' fall inside ms[1] --, then
  // reduce(x) (ms[3]) and, in a full call that acts on the results (act: ctvio_cull_visual), act(x) behind it (ms[4]).
  struct NoAct { void operator()(QueryRun &) const {} };
  template <class Record, class Solve, class Reduce, class Act = NoAct>
  int run_gate(const CallLayout &io, int s_in, int s_out, const CovScratch *scr, const GateSlices &gs, int32_t WinMeta::*slot0, int s0, int nall, Record &&record,
               Solve &&solve, Reduce &&reduce, Act &&act = Act()) {
    constexpr bool acts = !std::is_same<typename std::decay<Act>::type, NoAct>::value;
    const Spans full = {span_prepare(), {1, EV_COV_GRAM, EV_QUERY_BEGIN}, {2, EV_COV_SOLVE, EV_COV_GRAM}, {3, EV_QUERY_BEGIN, EV_QUERY_END}};
    const Spans full_act = {span_prepare(), {1, EV_COV_GRAM, EV_QUERY_BEGIN}, {2, EV_COV_SOLVE, EV_COV_GRAM}, {3, EV_QUERY_BEGIN, EV_QUERY_END},
                            {4, EV_QUERY_END, EV_CALL_END}};   // (run_query marks EV_CALL_END right behind the launches of a full call)
    return run_query(io, s_in, s_out, scr, {{2, EV_COV_SOLVE, EV_COV_GRAM}}, acts ? full_act : full, [&](QueryRun &x) {
                       if (!x.excl) {
                         if (nall) record(x, s0, nall);
                         reduce(x);
                         x.mark(EV_COV_GRAM);
                         return;
                       }
                       for (size_t si = 0; si < gs.slices.size(); ++si) {
                         const int first = meta_[gs.slices[si].wbeg].*slot0, n = (int)gs.slices[si].slots;
                         if (n) record(x, first, n);
                         if (si == 0) x.mark(EV_COV_GRAM);
                         if (n) solve(x, si, first, n);
                       }
                       x.mark(EV_QUERY_BEGIN);
                       reduce(x);
                       x.mark(EV_QUERY_END);
                       act(x);
                     });
  }
  int covariance(int only, const int32_t *n_sel, const int32_t *sel, double *cov, double *var_rho, int32_t *singular) {
    if (const int rc = guard()) return rc;
    const int nw = dev_.nwin;
    if (only >= nw) return fail(CTVIO_ERR_INVALID, "window id out of range");
    if (!n_sel) return fail(CTVIO_ERR_INVALID, "null n_sel");
    const int wbeg = only >= 0 ? only : 0, wend = only >= 0 ? only + 1 : nw;
    // ---- the call's tiles: selections first, then (with var_rho) every 16 consecutive sorted rows of W
    std::vector<CovTile> tiles;
    std::vector<CovWin> cwins;
    size_t nsel_tot = 0, ycount = 0, ncov = 0;
    {
      std::vector<uint8_t> seen;
      for (int w = wbeg; w < wend; ++w) {
        const WinMeta &m = meta_[w];
        const int ns = n_sel[w - wbeg];
        if (ns < 0 || ns > COV_MAX_SEL) return fail(CTVIO_ERR_INVALID, "window " + std::to_string(w) + ": n_sel outside [0, " + std::to_string(COV_MAX_SEL) + "]");
        if (ns && (!sel || !cov)) return fail(CTVIO_ERR_INVALID, "null sel / cov with a non-empty selection");
        seen.assign((size_t)m.P, 0);
        for (int i = 0; i < ns; ++i) {
          const int j = sel[nsel_tot + i];
          if (j < 0 || j >= m.P) return fail(CTVIO_ERR_INVALID, "window " + std::to_string(w) + ": selected unknown outside [0, P)");
          if (seen[j]) return fail(CTVIO_ERR_INVALID, "window " + std::to_string(w) + ": unknown " + std::to_string(j) + " selected twice");
          seen[j] = 1;
        }
        if (ns) {
          CovWin cw{w, ns, (int32_t)nsel_tot, 0, (long long)ycount, (long long)ncov};
          cwins.push_back(cw);
          for (int t = 0; 16 * t < ns; ++t) {
            tiles.push_back(CovTile{w, TILE_SEL, (int32_t)nsel_tot + 16 * t, std::min(16, ns - 16 * t), (long long)ycount});
            ycount += (size_t)16 * m.P;
          }
        }
        if (var_rho)
          for (int r = 0; r < m.L; r += 16) tiles.push_back(CovTile{w, TILE_RHO, r, std::min(16, m.L - r), 0});
        nsel_tot += (size_t)ns; ncov += (size_t)ns * ns;
      }
    }
    // ---- scratch.  io: selections, tiles, windows (in, one staged copy); cov | var_rho (Ltot, batch order) (out, one copy).  scr: mask,
    // exclusions, no records, Y
    const size_t nvar = var_rho ? (size_t)dev_.Ltot : 0;
    CovScratch cs(true, (size_t)dev_.Utot, 0, 0);
    CallLayout io = head_, &scr = cs.lay;
    const int s_sel = io.add("sel", sizeof(int32_t), nsel_tot, false), s_tiles = io.add("tiles", sizeof(CovTile), tiles.size(), false),
              s_wins = io.add("wins", sizeof(CovWin), cwins.size(), false), s_cov = io.add("cov", sizeof(double), ncov, true),
              s_var = io.add("var_rho", sizeof(double), nvar, true);
    const int s_y = scr.add("Y", sizeof(double), ycount, true);
    if (const int rc = reserve_call(io, &scr)) return rc;
    double *dy = scr.at<double>(call_scr_.dev, s_y), *dcov = io_dev<double>(io, s_cov), *dvar = io_dev<double>(io, s_var);
    const int32_t *dsel = io_dev<int32_t>(io, s_sel);
    const CovTile *dtiles = io_dev<CovTile>(io, s_tiles);
    const CovWin *dwins = io_dev<CovWin>(io, s_wins);
    const double *hcov = io_host<double>(io, s_cov), *vh = io_host<double>(io, s_var);
    Lm *lm = io_host<Lm>(io, HEAD_LM);
    if (nsel_tot) std::memcpy(io_host<int32_t>(io, s_sel), sel, sizeof(int32_t) * nsel_tot);
    if (!tiles.empty()) std::memcpy(io_host<CovTile>(io, s_tiles), tiles.data(), sizeof(CovTile) * tiles.size());
    if (!cwins.empty()) std::memcpy(io_host<CovWin>(io, s_wins), cwins.data(), sizeof(CovWin) * cwins.size());
    // the run sequence with k_cov_solve (ms[1]) and k_cov_gram (ms[2]) for launches, each where the call has work for it
    const int rc = run_query(io, s_sel, s_cov, &cs, {}, {span_prepare(), {1, EV_COV_SOLVE, EV_COV_GRAM, !tiles.empty()}, {2, EV_COV_GRAM, EV_CALL_END, !cwins.empty()}},
                             [&](QueryRun &x) {
                               if (!tiles.empty()) {
                                 CovSolveIO<COV_BASE> a;
                                 a.tiles = dtiles; a.sel = dsel; a.Y = dy; a.var_rho = dvar;
                                 launch_cov_solve(x.c, tiles.size(), a);
                               }
                               x.mark(EV_COV_GRAM);
                               if (!cwins.empty())
                                 hipLaunchKernelGGL(k_cov_gram, dim3(10, (unsigned)cwins.size()), dim3(256), 0, stream_, x.c, dwins, dsel, x.excl, dy, dcov);
                             });
    if (rc) return rc;
    // ---- results
    // (a window whose factorisation met a non-positive or non-finite pivot: its outputs are NaN)
    const double nan = std::nan("");
    size_t oc = 0, ov = 0;
    for (int w = wbeg; w < wend; ++w) {
      const WinMeta &m = meta_[w];
      const size_t ns = (size_t)n_sel[w - wbeg];
      const bool bad = lm[w].chol_fail != 0;
      if (singular) singular[w - wbeg] = bad ? 1 : 0;
      if (ns) { if (bad) std::fill(cov + oc, cov + oc + ns * ns, nan); else std::memcpy(cov + oc, hcov + oc, sizeof(double) * ns * ns); }
      if (var_rho) {
        for (int l = 0; l < m.L; ++l) var_rho[ov + l] = bad ? nan : vh[(size_t)m.lm0 + l];
        ov += (size_t)m.L;
      }
      oc += ns * ns;
    }
    return CTVIO_OK;
  }
  // ctvio_pose_covariance_batch / ctvio_pose_covariance (only >= 0: every query belongs to that window, win is not read): J Sigma J^T of the
  // pose at n query times.  The queries are grouped by window (stable: a window's queries keep the caller's order) and paired into tiles of
  // kind TILE_POSE; k_cov_pose_jac writes one record per query after k_cov_prepare (it reads the exclusions), k_cov_solve the 6 x 6 blocks into the
  // caller's slots (run_query, always full).
  int pose_covariance(int only, int64_t n64, const int32_t *win, const int64_t *t_ns, const double *q_SI, const double *p_SI, double *cov36,
                      int32_t *status) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    if (!check_count(n64) || (n64 && (!t_ns || !cov36 || (only < 0 && !win)))) return fail(CTVIO_ERR_INVALID, "bad arguments");
    if ((q_SI == nullptr) != (p_SI == nullptr)) return fail(CTVIO_ERR_INVALID, "sensor extrinsic: q_SI and p_SI come together (both null: the body pose)");
    SensorExt ext{};
    if (q_SI)
      if (const int rc = sensor_ext(q_SI, p_SI, ext)) return rc;
    const int n = (int)n64;
    const size_t nn = (size_t)n;
    const QueryOrder ord(only, n, win, dev_.nwin);
    if (!ord.error().empty()) return fail(CTVIO_ERR_INVALID, ord.error());
    if (n == 0) return CTVIO_OK;
    const std::vector<CovTile> tiles = query_tiles(ord, 2, TILE_POSE);
    // ---- out: cov36 | status
    CovScratch scr(true, (size_t)dev_.Utot, sizeof(PoseRec), nn);
    CallLayout io = head_;
    const int s_q = io.add("queries", sizeof(PoseQuery), nn, false), s_slot = io.add("slot", sizeof(int32_t), nn, false),
              s_tiles = io.add("tiles", sizeof(CovTile), tiles.size(), false), s_cov = io.add("cov36", sizeof(double), 36 * nn, true),
              s_stat = io.add("status", sizeof(int32_t), nn, false);
    if (const int rc = reserve_call(io, &scr.lay)) return rc;
    PoseQuery *hq = io_host<PoseQuery>(io, s_q);
    for (int r = 0; r < n; ++r) hq[r] = PoseQuery{ord.win_of(r), 0, (long long)(t_ns[ord.slot[(size_t)r]] - t0_[ord.win_of(r)])};
    stage_tiles(io, s_slot, s_tiles, ord, tiles);
    const int rc = run_query(
        io, s_q, s_cov, &scr,
        [&](QueryRun &x) {
          hipLaunchKernelGGL(k_cov_pose_jac, dim3(nblk(n, 64)), dim3(64), 0, stream_, dev_, n, io_dev<PoseQuery>(io, s_q), x.excl, ext, x.rec<PoseRec>(),
                             io_dev<int32_t>(io, s_stat));
        },
        [&](QueryRun &x) {
          CovSolveIO<COV_BASE> a;
          a.tiles = io_dev<CovTile>(io, s_tiles); a.slot = io_dev<int32_t>(io, s_slot); a.rec = x.rec<PoseRec>(); a.blocks = io_dev<double>(io, s_cov);
          launch_cov_solve(x.c, tiles.size(), a);
        });
    if (rc) return rc;
    // ---- results: the blocks as the kernel left them (the caller's order), the statuses in sorted order (time outside the spline: NaN)
    const Lm *lm = io_host<Lm>(io, HEAD_LM);
    const double *hcov = io_host<double>(io, s_cov);
    const int32_t *hstat = io_host<int32_t>(io, s_stat);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r];
      const int st = merge_status(hstat[r], lm[ord.win_of(r)].chol_fail != 0);
      cov_block(cov36 + 36 * i, hcov + 36 * i, 6, st);
      if (status) status[i] = st;
    }
    return CTVIO_OK;
  }
  // ctvio_nav_state_batch / ctvio_nav_state (only >= 0: every query belongs to that window, win is not read): the navigation state (pose,
  // world velocity, the biases of state frame[i]; frame null: the newest) at n query times and J Sigma J^T of its 15 tangent dimensions.
  // Values only (cov225 null): k_cov_nav_jac alone, nothing is linearised or factored.  Otherwise the queries are grouped by window (stable)
  // into tiles of kind TILE_NAV, one each; k_cov_nav_jac writes one record per query after k_cov_prepare (it reads the exclusions), k_cov_solve the
  // 15 x 15 blocks into the caller's slots (run_query).
  int nav_state(int only, int64_t n64, const int32_t *win, const int64_t *t_ns, const int32_t *frame, double *state16, double *cov225, int32_t *status) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    if (!check_count(n64) || (n64 && (!t_ns || (only < 0 && !win) || (!state16 && !cov225 && !status))))
      return fail(CTVIO_ERR_INVALID, "bad arguments");
    const int n = (int)n64;
    const size_t nn = (size_t)n;
    const QueryOrder ord(only, n, win, dev_.nwin);
    if (!ord.error().empty()) return fail(CTVIO_ERR_INVALID, ord.error());
    std::string err;
    for (int i = 0; i < n; ++i) {
      const int w = only >= 0 ? only : win[i];
      if (!check_frame(frame, i, meta_[w].F, "query", err)) return fail(CTVIO_ERR_INVALID, err);
    }
    if (n == 0) return CTVIO_OK;
    const bool want_cov = cov225 != nullptr;
    const size_t nc = want_cov ? nn : 0;
    const std::vector<CovTile> tiles = want_cov ? query_tiles(ord, 1, TILE_NAV) : std::vector<CovTile>();
    // ---- out: cov225 | state16 | status
    CovScratch scr(want_cov, (size_t)dev_.Utot, sizeof(NavRec), nn);
    CallLayout io = head_;
    const int s_q = io.add("queries", sizeof(NavQuery), nn, false), s_slot = io.add("slot", sizeof(int32_t), nc, false),
              s_tiles = io.add("tiles", sizeof(CovTile), tiles.size(), false), s_cov = io.add("cov225", sizeof(double), 225 * nc, true),
              s_state = io.add("state16", sizeof(double), 16 * nn, true), s_stat = io.add("status", sizeof(int32_t), nn, false);
    if (const int rc = reserve_call(io, want_cov ? &scr.lay : nullptr)) return rc;
    NavQuery *hq = io_host<NavQuery>(io, s_q);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r];
      const int w = ord.win_of(r);
      hq[r] = NavQuery{w, frame ? frame[i] : meta_[w].F - 1, (long long)(t_ns[i] - t0_[w])};
    }
    stage_tiles(io, s_slot, s_tiles, ord, tiles);
    const int rc = run_query(
        io, s_q, s_cov, want_cov ? &scr : nullptr,
        [&](QueryRun &x) {
          hipLaunchKernelGGL(k_cov_nav_jac, dim3(nblk(n, 64)), dim3(64), 0, stream_, dev_, n, io_dev<NavQuery>(io, s_q), x.excl, x.rec<NavRec>(),
                             io_dev<double>(io, s_state), io_dev<int32_t>(io, s_stat));
        },
        [&](QueryRun &x) {
          CovSolveIO<COV_BASE> a;
          a.tiles = io_dev<CovTile>(io, s_tiles); a.slot = io_dev<int32_t>(io, s_slot); a.nrec = x.rec<NavRec>(); a.nav_cov = io_dev<double>(io, s_cov);
          launch_cov_solve(x.c, tiles.size(), a);
        });
    if (rc) return rc;
    // ---- results: the blocks as the kernel left them (the caller's order), the states and statuses in sorted order (time outside the
    // spline: NaN)
    const Lm *lm = io_host<Lm>(io, HEAD_LM);
    const double *hcov = io_host<double>(io, s_cov), *hstate = io_host<double>(io, s_state);
    const int32_t *hstat = io_host<int32_t>(io, s_stat);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r];
      const int st = want_cov ? merge_status(hstat[r], lm[ord.win_of(r)].chol_fail != 0) : hstat[r];
      if (want_cov) cov_block(cov225 + 225 * i, hcov + 225 * i, 15, st);
      if (state16) std::memcpy(state16 + 16 * i, hstate + 16 * (size_t)r, sizeof(double) * 16);
      if (status) status[i] = st;
    }
    return CTVIO_OK;
  }
  // ctvio_body_rates_batch / ctvio_body_rates (only >= 0: every query belongs to that window, win is not read): body angular velocity,
  // specific force and body-frame velocity at n query times, J Sigma J^T of (domega, df, dv_B, dbg, dba) with the biases of state frame[i]
  // (frame null: the newest), and the gate of a candidate IMU sample.  Values only (cov225 and chi2 null): k_cov_rates_jac alone, nothing
  // is linearised or factored.  Otherwise the queries are grouped by window (stable) into tiles of kind TILE_RATES, one each;
  // k_cov_rates_jac writes one record per query after k_cov_prepare (it reads the exclusions), k_cov_solve the 15 x 15 blocks and the gates
  // into the caller's slots (run_query).
  int body_rates(int only, int64_t n64, const int32_t *win, const int64_t *t_ns, const int32_t *frame, const double *meas6, const double *noise6,
                 double *rates9, double *cov225, double *chi2, int32_t *status) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    if (!check_count(n64) || (n64 && (!t_ns || (only < 0 && !win) || (!rates9 && !cov225 && !chi2 && !status) || (chi2 && !meas6))))
      return fail(CTVIO_ERR_INVALID, "bad arguments");
    const int n = (int)n64;
    const size_t nn = (size_t)n;
    if (n && noise6)
      for (int c = 0; c < 6; ++c)
        if (!(noise6[c] > 0.0) || !std::isfinite(noise6[c])) return fail(CTVIO_ERR_INVALID, "noise6: six positive, finite standard deviations");
    const QueryOrder ord(only, n, win, dev_.nwin);
    if (!ord.error().empty()) return fail(CTVIO_ERR_INVALID, ord.error());
    std::string err;
    for (int i = 0; i < n; ++i) {
      const int w = only >= 0 ? only : win[i];
      if (!check_frame(frame, i, meta_[w].F, "query", err)) return fail(CTVIO_ERR_INVALID, err);
      for (int c = 0; c < 6; ++c) {
        if (meas6 && !std::isfinite(meas6[6 * (size_t)i + c])) return fail(CTVIO_ERR_INVALID, "query " + std::to_string(i) + ": non-finite IMU sample");
        if (chi2 && !noise6 && !(meta_[w].imu_w[c] > 0.0))
          return fail(CTVIO_ERR_INVALID, "query " + std::to_string(i) + ": noise6 is null and the window's imu_w has a non-positive entry");
      }
    }
    if (n == 0) return CTVIO_OK;
    const bool want_cov = cov225 || chi2;
    const size_t nc = want_cov ? nn : 0;
    const std::vector<CovTile> tiles = want_cov ? query_tiles(ord, 1, TILE_RATES) : std::vector<CovTile>();
    // ---- out: cov225 | chi2 | rates9 | status
    CovScratch scr(want_cov, (size_t)dev_.Utot, sizeof(RatesRec), nn);
    CallLayout io = head_;
    const int s_q = io.add("queries", sizeof(RatesQuery), nn, false), s_slot = io.add("slot", sizeof(int32_t), nc, false),
              s_tiles = io.add("tiles", sizeof(CovTile), tiles.size(), false), s_cov = io.add("cov225", sizeof(double), 225 * nc, true),
              s_chi = io.add("chi2", sizeof(double), nc, true), s_val = io.add("rates9", sizeof(double), 9 * nn, true),
              s_stat = io.add("status", sizeof(int32_t), nn, false);
    if (const int rc = reserve_call(io, want_cov ? &scr.lay : nullptr)) return rc;
    RatesQuery *hq = io_host<RatesQuery>(io, s_q);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r];
      const int w = ord.win_of(r);
      RatesQuery q{w, frame ? frame[i] : meta_[w].F - 1, (long long)(t_ns[i] - t0_[w]), {0, 0, 0, 0, 0, 0}, {1, 1, 1, 1, 1, 1}};
      for (int c = 0; c < 6 && chi2; ++c) { q.meas[c] = meas6[6 * i + c]; q.sig[c] = noise6 ? noise6[c] : 1.0 / meta_[w].imu_w[c]; }
      hq[r] = q;
    }
    stage_tiles(io, s_slot, s_tiles, ord, tiles);
    const int rc = run_query(
        io, s_q, s_cov, want_cov ? &scr : nullptr,
        [&](QueryRun &x) {
          hipLaunchKernelGGL(k_cov_rates_jac, dim3(nblk(n, 64)), dim3(64), 0, stream_, dev_, n, io_dev<RatesQuery>(io, s_q), x.excl, x.rec<RatesRec>(),
                             io_dev<double>(io, s_val), io_dev<int32_t>(io, s_stat));
        },
        [&](QueryRun &x) {
          CovSolveIO<COV_RATES> a;
          a.tiles = io_dev<CovTile>(io, s_tiles); a.slot = io_dev<int32_t>(io, s_slot); a.rec = x.rec<RatesRec>(); a.blocks = io_dev<double>(io, s_cov);
          if (chi2) a.chi2 = io_dev<double>(io, s_chi);
          launch_cov_solve(x.c, tiles.size(), a);
        });
    if (rc) return rc;
    // ---- results: the blocks and gates as the kernel left them (the caller's order), the values and statuses in sorted order (time
    // outside the spline: NaN)
    const Lm *lm = io_host<Lm>(io, HEAD_LM);
    const double *hcov = io_host<double>(io, s_cov), *hchi = io_host<double>(io, s_chi), *hval = io_host<double>(io, s_val);
    const int32_t *hstat = io_host<int32_t>(io, s_stat);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r];
      const int st = want_cov ? merge_status(hstat[r], lm[ord.win_of(r)].chol_fail != 0) : hstat[r];
      if (cov225) cov_block(cov225 + 225 * i, hcov + 225 * i, 15, st);
      if (chi2) chi2[i] = gate_value(hchi[i], st);
      if (rates9) std::memcpy(rates9 + 9 * i, hval + 9 * (size_t)r, sizeof(double) * 9);
      if (status) status[i] = st;
    }
    return CTVIO_OK;
  }
  // ctvio_imu_predict_batch / ctvio_imu_predict (only >= 0: every query belongs to that window, win is not read): the navigation state of
  // query i at imu_t[first sample of i] (bias state frame[i]; frame null: the newest) carried through the query's n_imu[i] samples by
  // k_imu_propagate, with its 15 x 15 covariance.  nav_state()'s launches -- queries grouped by window (stable), k_cov_nav_jac, and with
  // cov225 k_cov_solve on TILE_NAV tiles, whose slot is the query's first output entry, so that P_0 lands where sample 0 is reported --,
  // then k_imu_propagate (run_query with a fourth timing slot).  The samples of all queries (ImuSamples) are staged with the queries in one copy.
  int imu_predict(int only, int64_t n64, const int32_t *win, const int32_t *frame, const int32_t *n_imu, const int64_t *imu_t, const double *imu_gyro,
                  const double *imu_acc, const ctvio_imu_noise *noise, int last_only, double *state16, double *cov225, int32_t *status) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    if (!check_count(n64) ||
        (n64 && (!n_imu || !imu_t || !imu_gyro || !imu_acc || !noise || (only < 0 && !win) || (!state16 && !cov225 && !status))))
      return fail(CTVIO_ERR_INVALID, "bad arguments");
    const int n = (int)n64;
    const size_t nn = (size_t)n;
    if (n == 0) return CTVIO_OK;
    ImuSamples sam;
    if (!sam.noise(*noise)) return fail(CTVIO_ERR_INVALID, sam.error);
    const QueryOrder ord(only, n, win, dev_.nwin);
    if (!ord.error().empty()) return fail(CTVIO_ERR_INVALID, ord.error());
    if (!sam.streams("query", only, n, win, frame, meta_.data(), n_imu, imu_t, imu_gyro, imu_acc)) return fail(CTVIO_ERR_INVALID, sam.error);
    const std::vector<int64_t> &first = sam.first;   // first sample of every query (the caller's order)
    const size_t ns = sam.ns, no = last_only ? nn : ns;   // samples; output entries
    auto entry0 = [&](size_t i) { return last_only ? (int64_t)i : first[i]; };
    auto entries = [&](size_t i) { return last_only ? (size_t)1 : (size_t)n_imu[i]; };
    const bool want_cov = cov225 != nullptr;
    const std::vector<CovTile> tiles = want_cov ? query_tiles(ord, 1, TILE_NAV) : std::vector<CovTile>();
    // ---- scratch.  io: queries, propagation queries, sample times and measurements, entries, tiles (in, one staged copy); cov225 | state16 |
    // status (out, one copy).  scr: mask, exclusions, records, the states at sample 0
    CovScratch cs(want_cov, (size_t)dev_.Utot, sizeof(NavRec), nn);
    CallLayout io = head_, &scr = cs.lay;
    const int s_q = io.add("queries", sizeof(NavQuery), nn, false), s_pq = io.add("prop", sizeof(PropQuery), nn, false);
    sam.add(io);
    const int s_slot = io.add("entry", sizeof(int32_t), want_cov ? nn : 0, false), s_tiles = io.add("tiles", sizeof(CovTile), tiles.size(), false),
              s_cov = io.add("cov225", sizeof(double), want_cov ? 225 * no : 0, true), s_state = io.add("state16", sizeof(double), 16 * no, true),
              s_stat = io.add("status", sizeof(int32_t), nn, false);
    const int s_x0 = scr.add("state0", sizeof(double), 16 * nn, true);
    if (const int rc = reserve_call(io, &scr)) return rc;
    NavQuery *hq = io_host<NavQuery>(io, s_q);
    PropQuery *hp = io_host<PropQuery>(io, s_pq);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r];
      const int w = ord.win_of(r);
      hq[r] = NavQuery{w, frame ? frame[i] : meta_[w].F - 1, (long long)(imu_t[first[i]] - t0_[w])};
      hp[r] = PropQuery{w, n_imu[i], (long long)first[i], (long long)entry0(i)};
      if (want_cov) io_host<int32_t>(io, s_slot)[r] = (int32_t)entry0(i);
    }
    stage_tiles(io, -1, s_tiles, ord, tiles);
    sam.stage(io, call_io_.host);
    const ImuNoise nz{noise->gyr_n, noise->acc_n, noise->gyr_w, noise->acc_w};
    double *x0 = scr.at<double>(call_scr_.dev, s_x0);
    // the launches: k_cov_nav_jac (ms[2]), with cov225 k_cov_solve (ms[1]), then k_imu_propagate (ms[3]) behind whichever came last
    const int rc = run_query(
        io, s_q, s_cov, want_cov ? &cs : nullptr, {{2, EV_COV_SOLVE, EV_COV_GRAM}, {3, EV_COV_GRAM, EV_QUERY_END}},
        {span_prepare(), {1, EV_COV_GRAM, EV_QUERY_BEGIN}, {2, EV_COV_SOLVE, EV_COV_GRAM}, {3, EV_QUERY_BEGIN, EV_QUERY_END}}, [&](QueryRun &x) {
          hipLaunchKernelGGL(k_cov_nav_jac, dim3(nblk(n, 64)), dim3(64), 0, stream_, dev_, n, io_dev<NavQuery>(io, s_q), x.excl, x.rec<NavRec>(), x0,
                             io_dev<int32_t>(io, s_stat));
          x.mark(EV_COV_GRAM);
          if (x.excl) {
            CovSolveIO<COV_BASE> a;
            a.tiles = io_dev<CovTile>(io, s_tiles); a.slot = io_dev<int32_t>(io, s_slot); a.nrec = x.rec<NavRec>(); a.nav_cov = io_dev<double>(io, s_cov);
            launch_cov_solve(x.c, tiles.size(), a);
            x.mark(EV_QUERY_BEGIN);
          }
          hipLaunchKernelGGL(k_imu_propagate, dim3(nblk(n, 4)), dim3(64), 0, stream_, dev_, n, io_dev<PropQuery>(io, s_pq), io_dev<int32_t>(io, s_stat),
                             io_dev<long long>(io, sam.s_t), io_dev<double>(io, sam.s_gyro), io_dev<double>(io, sam.s_acc), nz, last_only ? 1 : 0, (const double *)x0,
                             io_dev<double>(io, s_state), want_cov ? io_dev<double>(io, s_cov) : (double *)nullptr);
          x.mark(EV_QUERY_END);
        });
    if (rc) return rc;
    // ---- results, every entry of a query by the query's status (time outside the spline: NaN)
    const Lm *lm = io_host<Lm>(io, HEAD_LM);
    const double *hcov = io_host<double>(io, s_cov), *hstate = io_host<double>(io, s_state);
    const int32_t *hstat = io_host<int32_t>(io, s_stat);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r], e0 = (size_t)entry0(i), ne = entries(i);
      const int st = want_cov ? merge_status(hstat[r], lm[ord.win_of(r)].chol_fail != 0) : hstat[r];
      for (size_t e = e0; e < e0 + ne && want_cov; ++e) cov_block(cov225 + 225 * e, hcov + 225 * e, 15, st);
      if (state16) {
        if (st != POSE_OUTSIDE) std::memcpy(state16 + 16 * e0, hstate + 16 * e0, sizeof(double) * 16 * ne);
        else std::fill(state16 + 16 * e0, state16 + 16 * (e0 + ne), std::nan(""));
      }
      if (status) status[i] = st;
    }
    return CTVIO_OK;
  }
  // ctvio_relative_pose_batch / ctvio_relative_pose (only >= 0: every query belongs to that window, win is not read): the pose increment
  // T(t_a)^-1 T(t_b) of n pairs of times and J_rel Sigma J_rel^T of its six tangent dimensions.  Values only (cov36 null): k_cov_rel_jac
  // alone, nothing is linearised or factored.  Otherwise the queries are grouped by window (stable: a window's queries keep the caller's
  // order) and paired into tiles of kind TILE_REL; k_cov_rel_jac writes one record per query after k_cov_prepare (it reads the exclusions),
  // k_cov_solve the 6 x 6 blocks into the caller's slots (run_query).
  int relative_pose(int only, int64_t n64, const int32_t *win, const int64_t *t_a_ns, const int64_t *t_b_ns, const double *q_SI, const double *p_SI,
                    double *rel7, double *cov36, int32_t *status) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    if (!check_count(n64) || (n64 && (!t_a_ns || !t_b_ns || (only < 0 && !win) || (!rel7 && !cov36 && !status))))
      return fail(CTVIO_ERR_INVALID, "bad arguments");
    if ((q_SI == nullptr) != (p_SI == nullptr)) return fail(CTVIO_ERR_INVALID, "sensor extrinsic: q_SI and p_SI come together (both null: the body pose)");
    SensorExt ext{};
    if (q_SI)
      if (const int rc = sensor_ext(q_SI, p_SI, ext)) return rc;
    const int n = (int)n64;
    const size_t nn = (size_t)n;
    const QueryOrder ord(only, n, win, dev_.nwin);
    if (!ord.error().empty()) return fail(CTVIO_ERR_INVALID, ord.error());
    if (n == 0) return CTVIO_OK;
    const bool want_cov = cov36 != nullptr;
    const size_t nc = want_cov ? nn : 0;
    const std::vector<CovTile> tiles = want_cov ? query_tiles(ord, 2, TILE_REL) : std::vector<CovTile>();
    // ---- out: rel7 | cov36 | status
    CovScratch scr(want_cov, (size_t)dev_.Utot, sizeof(RelRec), nn);
    CallLayout io = head_;
    const int s_q = io.add("queries", sizeof(RelQuery), nn, false), s_slot = io.add("slot", sizeof(int32_t), nc, false),
              s_tiles = io.add("tiles", sizeof(CovTile), tiles.size(), false), s_rel = io.add("rel7", sizeof(double), 7 * nn, true),
              s_cov = io.add("cov36", sizeof(double), 36 * nc, true), s_stat = io.add("status", sizeof(int32_t), nn, false);
    if (const int rc = reserve_call(io, want_cov ? &scr.lay : nullptr)) return rc;
    RelQuery *hq = io_host<RelQuery>(io, s_q);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r];
      const int w = ord.win_of(r);
      hq[r] = RelQuery{w, 0, (long long)(t_a_ns[i] - t0_[w]), (long long)(t_b_ns[i] - t0_[w])};
    }
    stage_tiles(io, s_slot, s_tiles, ord, tiles);
    const int rc = run_query(
        io, s_q, s_rel, want_cov ? &scr : nullptr,
        [&](QueryRun &x) {
          hipLaunchKernelGGL(k_cov_rel_jac, dim3(nblk(n, 64)), dim3(64), 0, stream_, dev_, n, io_dev<RelQuery>(io, s_q), x.excl, ext, x.rec<RelRec>(),
                             io_dev<double>(io, s_rel), io_dev<int32_t>(io, s_stat));
        },
        [&](QueryRun &x) {
          CovSolveIO<COV_REL> a;
          a.tiles = io_dev<CovTile>(io, s_tiles); a.slot = io_dev<int32_t>(io, s_slot); a.rec = x.rec<RelRec>(); a.blocks = io_dev<double>(io, s_cov);
          launch_cov_solve(x.c, tiles.size(), a);
        });
    if (rc) return rc;
    // ---- results: the blocks as the kernel left them (the caller's order), the values and statuses in sorted order (either time outside
    // the spline: NaN)
    const Lm *lm = io_host<Lm>(io, HEAD_LM);
    const double *hcov = io_host<double>(io, s_cov), *hrel = io_host<double>(io, s_rel);
    const int32_t *hstat = io_host<int32_t>(io, s_stat);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r];
      const int st = want_cov ? merge_status(hstat[r], lm[ord.win_of(r)].chol_fail != 0) : hstat[r];
      if (want_cov) cov_block(cov36 + 36 * i, hcov + 36 * i, 6, st);
      if (rel7) std::memcpy(rel7 + 7 * i, hrel + 7 * (size_t)r, sizeof(double) * 7);
      if (status) status[i] = st;
    }
    return CTVIO_OK;
  }
  // ctvio_project_landmarks_batch / ctvio_project_landmarks (only >= 0: every query belongs to that window, win is not read): the predicted
  // image point of landmark lm[i] in the camera at (t_ns[i], row[i]), its 2 x 2 covariance and the gate of a candidate point.  Values only
  // (cov4 and chi2 null): k_cov_proj_jac alone, nothing is linearised or factored.  Otherwise the queries are grouped by window (stable: a
  // window's queries keep the caller's order), eight to a tile of kind TILE_PROJ; k_cov_proj_jac writes one record per query after k_cov_prepare (it
  // reads the exclusions and 1 / Hll), k_cov_solve the 2 x 2 blocks and gates by record (run_query).
  int project_landmarks(int only, int64_t n64, const int32_t *win, const int32_t *lmi, const int64_t *t_ns, const int32_t *row, const ctvio_row_model *rm,
                        const double *obs2, double *proj3, double *cov4, double *chi2, int32_t *row_out, int32_t *status) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    if (!check_count(n64) ||
        (n64 && (!lmi || !t_ns || !row || (only < 0 && !win) || (!proj3 && !cov4 && !chi2 && !row_out && !status) || (chi2 && !obs2))))
      return fail(CTVIO_ERR_INVALID, "bad arguments");
    ProjRowModel prm{0.0, 0.0, 1, 0};
    if (rm) {
      if (rm->iterations < 1 || rm->iterations > 8 || rm->rows < 1 || !std::isfinite(rm->fy) || !std::isfinite(rm->cy))
        return fail(CTVIO_ERR_INVALID, "row model: iterations in 1 .. 8, rows >= 1, finite fy and cy");
      prm = ProjRowModel{rm->fy, rm->cy, rm->rows, rm->iterations};
    }
    const int n = (int)n64;
    const size_t nn = (size_t)n;
    const QueryOrder ord(only, n, win, dev_.nwin);
    if (!ord.error().empty()) return fail(CTVIO_ERR_INVALID, ord.error());
    for (int i = 0; i < n; ++i) {
      const int w = only >= 0 ? only : win[i];
      if (lmi[i] < 0 || lmi[i] >= meta_[w].L) return fail(CTVIO_ERR_INVALID, "query " + std::to_string(i) + ": landmark index out of range");
      if (obs2 && !(std::isfinite(obs2[2 * (size_t)i]) && std::isfinite(obs2[2 * (size_t)i + 1])))
        return fail(CTVIO_ERR_INVALID, "query " + std::to_string(i) + ": non-finite candidate point");
    }
    if (n == 0) return CTVIO_OK;
    const bool want_cov = cov4 || chi2;
    const size_t nc = want_cov ? nn : 0;
    const std::vector<CovTile> tiles = want_cov ? query_tiles(ord, PRJ_PER_TILE, TILE_PROJ) : std::vector<CovTile>();
    // ---- out: proj3 | cov4 | chi2 | row | status, all in sorted order (the kernels write by record: no slots)
    CovScratch scr(want_cov, (size_t)dev_.Utot, sizeof(ProjRec), nn);
    CallLayout io = head_;
    const int s_q = io.add("queries", sizeof(ProjQuery), nn, false), s_tiles = io.add("tiles", sizeof(CovTile), tiles.size(), false),
              s_proj = io.add("proj3", sizeof(double), 3 * nn, true), s_cov = io.add("cov4", sizeof(double), 4 * nc, true),
              s_chi = io.add("chi2", sizeof(double), nc, true), s_row = io.add("row", sizeof(int32_t), nn, false),
              s_stat = io.add("status", sizeof(int32_t), nn, false);
    if (const int rc = reserve_call(io, want_cov ? &scr.lay : nullptr)) return rc;
    ProjQuery *hq = io_host<ProjQuery>(io, s_q);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r];
      const int w = ord.win_of(r);
      hq[r] = ProjQuery{w, lmi[i], row[i], 0, (long long)(t_ns[i] - t0_[w]), {obs2 ? obs2[2 * i] : 0.0, obs2 ? obs2[2 * i + 1] : 0.0}};
    }
    stage_tiles(io, -1, s_tiles, ord, tiles);
    const int rc = run_query(
        io, s_q, s_proj, want_cov ? &scr : nullptr,
        [&](QueryRun &x) {
          hipLaunchKernelGGL(k_cov_proj_jac, dim3(nblk(n, 64)), dim3(64), 0, stream_, dev_, n, io_dev<ProjQuery>(io, s_q), x.excl, prm, x.rec<ProjRec>(),
                             io_dev<double>(io, s_proj), io_dev<int32_t>(io, s_row), io_dev<int32_t>(io, s_stat));
        },
        [&](QueryRun &x) {
          CovSolveIO<COV_PROJ> a;
          a.tiles = io_dev<CovTile>(io, s_tiles); a.rec = x.rec<ProjRec>(); a.blocks = io_dev<double>(io, s_cov);
          if (chi2) a.chi2 = io_dev<double>(io, s_chi);
          launch_cov_solve(x.c, tiles.size(), a);
        });
    if (rc) return rc;
    // ---- results (not computable: NaN)
    const Lm *lm = io_host<Lm>(io, HEAD_LM);
    const double *hproj = io_host<double>(io, s_proj), *hcov = io_host<double>(io, s_cov), *hchi = io_host<double>(io, s_chi);
    const int32_t *hrow = io_host<int32_t>(io, s_row), *hstat = io_host<int32_t>(io, s_stat);
    for (int r = 0; r < n; ++r) {
      const size_t i = (size_t)ord.slot[(size_t)r];
      const int st = want_cov ? merge_status(hstat[r], lm[ord.win_of(r)].chol_fail != 0) : hstat[r];
      if (cov4) cov_block(cov4 + 4 * i, hcov + 4 * (size_t)r, 2, st);
      if (chi2) chi2[i] = gate_value(hchi[r], st);
      if (proj3) std::memcpy(proj3 + 3 * i, hproj + 3 * (size_t)r, sizeof(double) * 3);
      if (row_out) row_out[i] = hrow[r];
      if (status) status[i] = st;
    }
    return CTVIO_OK;
  }
  // ctvio_visual_gate_batch / ctvio_visual_gate (only >= 0: that window alone): the leave-one-out test of every visual block of the windows
  // themselves.  No inputs: k_cov_gate_jac reads the block slots the upload holds and writes by slot; the host scatters into the caller's
  // block order (gate_slot_).  Values only (redundancy, cov4, chi2 and lm_stats3 null): k_cov_gate_jac alone (and k_cov_gate_reduce for
  // lm_count), nothing is linearised or factored.  Otherwise run_gate: per slice of windows k_cov_gate_jac and k_cov_solve<COV_GATE> (kind
  // TILE_GATE), then k_cov_gate_reduce.
  // ctvio_cull_visual_batch / ctvio_cull_visual are the same call with `cull`: always full, every gate output stays on the device, and
  // k_vis_cull behind the reduction decides on them and updates Dev::v_on; what comes back is culled | flags by slot.
  static constexpr GateCodes VIS_GATE_CODES{QUERY_OK, GATE_WEAK, QUERY_SINGULAR, QUERY_NO_INFO, GATE_INACTIVE};
  struct CullCall { CullRules rules; int32_t *n_culled; uint8_t *active; };
  int visual_gate(int only, const ctvio_gate_options *o, double *res2, double *weight, double *depth, double *red, double *cov4, double *chi2, int32_t *status,
                  double *lm_stats3, int32_t *lm_count, const CullCall *cull = nullptr) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    if (!o) return fail(CTVIO_ERR_INVALID, "null options");
    if (!(o->min_redundancy > 0.0 && o->min_redundancy < 1.0)) return fail(CTVIO_ERR_INVALID, "min_redundancy outside (0, 1)");
    const int wbeg = only >= 0 ? only : 0, wend = only >= 0 ? only + 1 : dev_.nwin;
    const int s0 = meta_[wbeg].vis0, nslot = meta_[wend - 1].vis0 + meta_[wend - 1].Vp - s0, l0 = meta_[wbeg].lm0;
    const size_t v0 = gate_voff_[(size_t)wbeg], V = gate_voff_[(size_t)wend] - v0;
    size_t L = 0;
    for (int w = wbeg; w < wend; ++w) L += (size_t)meta_[w].L;
    if (V && !cull && !res2 && !weight && !depth && !red && !cov4 && !chi2 && !status && !lm_stats3 && !lm_count) return fail(CTVIO_ERR_INVALID, "every output is null");
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    if (V == 0) {   // (nothing is launched; a landmark without blocks: count 0 and (NaN, 0, +inf))
      for (size_t l = 0; l < L; ++l) {
        if (lm_count) lm_count[l] = 0;
        if (lm_stats3) { lm_stats3[3 * l] = nan; lm_stats3[3 * l + 1] = 0.0; lm_stats3[3 * l + 2] = inf; }
      }
      if (cull && cull->n_culled) std::fill(cull->n_culled, cull->n_culled + (wend - wbeg), 0);
      return CTVIO_OK;
    }
    const bool full = cull || red || cov4 || chi2 || lm_stats3, want_lm = cull || lm_stats3 || lm_count, want_stats = cull || lm_stats3;
    const GateSlices gs = gate_slices(&WinMeta::Vp, wbeg, wend, GATE_SLICE_SLOTS);
    // ---- out, by block slot: res2 | weight | depth | redundancy | cov4 | chi2 | status, then by landmark: lm_stats3 | lm_count; no inputs
    const size_t ns = (size_t)nslot, nf = full ? ns : 0, nl = want_lm ? L : 0;
    CovScratch scr(full, (size_t)dev_.Utot, sizeof(GateRec), gs.nrec);
    const int s_en = scr.lay.add("enorm", sizeof(double), want_stats ? ns : 0, true);
    CallLayout io = head_;
    const int s_res = io.add("res2", sizeof(double), 2 * ns, true), s_wgt = io.add("weight", sizeof(double), ns, true),
              s_dep = io.add("depth", sizeof(double), ns, true), s_red = io.add("redundancy", sizeof(double), nf, true),
              s_cov = io.add("cov4", sizeof(double), 4 * nf, true), s_chi = io.add("chi2", sizeof(double), nf, true),
              s_stat = io.add("status", sizeof(int32_t), ns, false), s_lms = io.add("lm_stats3", sizeof(double), want_stats ? 3 * L : 0, true),
              s_lmc = io.add("lm_count", sizeof(int32_t), nl, false), s_cul = io.add("culled", 1, cull ? ns : 0, false),
              s_flg = io.add("flags", 1, cull ? ns : 0, false);
    if (const int rc = reserve_call(io, full ? &scr.lay : nullptr)) return rc;
    GateOut out{io_dev<double>(io, s_res), io_dev<double>(io, s_wgt), io_dev<double>(io, s_dep), want_stats ? scr.lay.at<double>(call_scr_.dev, s_en) : nullptr,
                full ? io_dev<double>(io, s_red) : nullptr, full ? io_dev<double>(io, s_cov) : nullptr, full ? io_dev<double>(io, s_chi) : nullptr,
                io_dev<int32_t>(io, s_stat), s0, 0, o->min_redundancy};
    const auto record = [&](QueryRun &x, int first, int n) {
      hipLaunchKernelGGL(k_cov_gate_jac, dim3(nblk(n, 64)), dim3(64), 0, stream_, dev_, first, n, x.excl, x.rec<GateRec>(), out);
    };
    const auto solve = [&](QueryRun &x, size_t, int first, int n) {
      CovSolveIO<COV_GATE> a;
      a.rec = x.rec<GateRec>(); a.slot_base = first; a.gate = out; a.gate.nslot = n;
      launch_cov_solve(x.c, (size_t)nblk(n, PRJ_PER_TILE), a);
    };
    const auto reduce = [&](QueryRun &) {
      if (want_lm && L)
        hipLaunchKernelGGL(k_cov_gate_reduce, dim3(nblk((int)L, 64)), dim3(64), 0, stream_, dev_, l0, (int)L, out, full ? 1 : 0,
                           want_stats ? io_dev<double>(io, s_lms) : nullptr, io_dev<int32_t>(io, s_lmc));
    };
    if (cull) {
      // (no inputs; culled | flags come back)
      const int rc = run_gate(io, s_cul, s_cul, &scr, gs, &WinMeta::vis0, s0, nslot, record, solve, reduce, [&](QueryRun &) {
        if (L)
          hipLaunchKernelGGL(k_vis_cull, dim3(nblk((int)L, 64)), dim3(64), 0, stream_, dev_, l0, (int)L, out, cull->rules, io_dev<double>(io, s_lms),
                             io_dev<int32_t>(io, s_lmc), io_dev<uint8_t>(io, s_cul), io_dev<uint8_t>(io, s_flg));
      });
      if (rc) return rc;
      const uint8_t *hcul = io_host<uint8_t>(io, s_cul), *hflg = io_host<uint8_t>(io, s_flg);
      for (int w = wbeg; w < wend; ++w) {
        int32_t nc = 0;
        for (size_t b = gate_voff_[(size_t)w]; b < gate_voff_[(size_t)w + 1]; ++b) {
          const size_t k = (size_t)(gate_slot_[b] - s0);
          nc += hcul[k];
          if (cull->active) cull->active[b - v0] = hflg[k];
        }
        if (cull->n_culled) cull->n_culled[w - wbeg] = nc;
      }
      return CTVIO_OK;
    }
    const int rc = run_gate(io, s_res, s_res, full ? &scr : nullptr, gs, &WinMeta::vis0, s0, nslot, record, solve, reduce);
    if (rc) return rc;
    // ---- results, in the caller's block order.  Precedence 3, 2, 1 (the window's factorisation failed), 5 (inactive), 4, 0.
    const Lm *lm = io_host<Lm>(io, HEAD_LM);
    const double *hres = io_host<double>(io, s_res), *hwgt = io_host<double>(io, s_wgt), *hdep = io_host<double>(io, s_dep), *hred = io_host<double>(io, s_red),
                 *hcov = io_host<double>(io, s_cov), *hchi = io_host<double>(io, s_chi);
    const int32_t *hstat = io_host<int32_t>(io, s_stat);
    for (int w = wbeg; w < wend; ++w) {
      const bool bad = full && lm[w].chol_fail != 0;
      for (size_t b = gate_voff_[(size_t)w]; b < gate_voff_[(size_t)w + 1]; ++b) {
        const size_t i = b - v0, k = (size_t)(gate_slot_[b] - s0);
        const int st = gate_scatter(VIS_GATE_CODES, hstat[k], bad, 2, hred + k, hcov + 4 * k, hchi + k, red ? red + i : nullptr, cov4 ? cov4 + 4 * i : nullptr,
                                    chi2 ? chi2 + i : nullptr);
        if (res2) { res2[2 * i] = hres[2 * k]; res2[2 * i + 1] = hres[2 * k + 1]; }
        if (weight) weight[i] = hwgt[k];
        if (depth) depth[i] = hdep[k];
        if (status) status[i] = st;
      }
    }
    if (lm_stats3) std::memcpy(lm_stats3, io_host<double>(io, s_lms), sizeof(double) * 3 * L);
    if (lm_count) std::memcpy(lm_count, io_host<int32_t>(io, s_lmc), sizeof(int32_t) * L);
    return CTVIO_OK;
  }
  int cull_visual(int only, const ctvio_cull_options *o, int32_t *n_culled, uint8_t *active) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    if (!o) return fail(CTVIO_ERR_INVALID, "null options");
    const ctvio_gate_options g{o->min_redundancy};
    const CullCall c{CullRules{o->chi2_max, o->mean_error_max, o->worst_only, o->drop_uncomputable}, n_culled, active};
    return visual_gate(only, &g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &c);
  }
  // ctvio_set_visual_active* / ctvio_get_visual_active* (only >= 0: that window alone): Dev::v_on of the windows' slots (padding included:
  // nobody reads a padding slot's flag) in ONE copy, the caller's block order by gate_slot_.  Nothing else of the handle moves.
  int set_visual_active(int only, const uint8_t *active) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    const int wbeg = only >= 0 ? only : 0, wend = only >= 0 ? only + 1 : dev_.nwin;
    const int s0 = meta_[wbeg].vis0, nslot = meta_[wend - 1].vis0 + meta_[wend - 1].Vp - s0;
    const size_t v0 = gate_voff_[(size_t)wbeg];
    if (nslot == 0) return CTVIO_OK;
    CallLayout io = head_;
    const int s_f = io.add("flags", 1, (size_t)nslot, false);
    if (const int rc = reserve_call(io)) return rc;
    uint8_t *h = io_host<uint8_t>(io, s_f);
    std::memset(h, 1, (size_t)nslot);
    if (active)
      for (size_t b = v0; b < gate_voff_[(size_t)wend]; ++b) h[gate_slot_[b] - s0] = active[b - v0] ? 1 : 0;
    HIPCHK(hipMemcpyAsync(dev_.v_on + s0, h, (size_t)nslot, hipMemcpyHostToDevice, stream_));
    return sync_call();
  }
  int get_visual_active(int only, uint8_t *active) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    const int wbeg = only >= 0 ? only : 0, wend = only >= 0 ? only + 1 : dev_.nwin;
    const int s0 = meta_[wbeg].vis0, nslot = meta_[wend - 1].vis0 + meta_[wend - 1].Vp - s0;
    const size_t v0 = gate_voff_[(size_t)wbeg], V = gate_voff_[(size_t)wend] - v0;
    if (V == 0) return CTVIO_OK;
    if (!active) return fail(CTVIO_ERR_INVALID, "null output");
    CallLayout io = head_;
    const int s_f = io.add("flags", 1, (size_t)nslot, false);
    if (const int rc = reserve_call(io)) return rc;
    uint8_t *h = io_host<uint8_t>(io, s_f);
    HIPCHK(hipMemcpyAsync(h, dev_.v_on + s0, (size_t)nslot, hipMemcpyDeviceToHost, stream_));
    if (const int rc = sync_call()) return rc;
    for (size_t b = v0; b < v0 + V; ++b) active[b - v0] = h[gate_slot_[b] - s0] ? 1 : 0;
    return CTVIO_OK;
  }
  // ctvio_imu_gate_batch / ctvio_imu_gate (only >= 0: that window alone): the leave-one-out test of every IMU sample of the windows
  // themselves.  No inputs but the tile descriptors (one per window and slice): k_cov_imugate_jac reads the packed samples the upload holds
  // and writes by slot; the host scatters into the caller's sample order (imu_slot_).  Values only (redundancy, cov36, chi2 and
  // frame_stats4 null): k_cov_imugate_jac alone, nothing is linearised or factored.  Otherwise run_gate on the sample counts: per slice of
  // windows k_cov_imugate_jac and k_cov_solve<COV_IMUGATE>, then k_cov_imugate_reduce.
  int imu_gate(int only, const ctvio_gate_options *o, double *res6, double *red, double *cov36, double *chi2, int32_t *status, double *frame_stats4) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    if (!o) return fail(CTVIO_ERR_INVALID, "null options");
    if (!(o->min_redundancy > 0.0 && o->min_redundancy < 1.0)) return fail(CTVIO_ERR_INVALID, "min_redundancy outside (0, 1)");
    const int wbeg = only >= 0 ? only : 0, wend = only >= 0 ? only + 1 : dev_.nwin;
    const int s0 = meta_[wbeg].imu0, f0 = meta_[wbeg].bias0;
    const size_t m0 = imu_moff_[(size_t)wbeg], M = imu_moff_[(size_t)wend] - m0;
    size_t F = 0;
    for (int w = wbeg; w < wend; ++w) F += (size_t)meta_[w].F;
    if (M && !res6 && !red && !cov36 && !chi2 && !status && !frame_stats4) return fail(CTVIO_ERR_INVALID, "every output is null");
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    if (M == 0) {   // (nothing is launched; a bias state without samples: (0, NaN, 0, +inf))
      for (size_t f = 0; f < F && frame_stats4; ++f) { frame_stats4[4 * f] = 0.0; frame_stats4[4 * f + 1] = nan; frame_stats4[4 * f + 2] = 0.0; frame_stats4[4 * f + 3] = inf; }
      return CTVIO_OK;
    }
    const bool full = red || cov36 || chi2 || frame_stats4;
    const GateSlices gs = gate_slices(&WinMeta::M, wbeg, wend, IMU_GATE_SLICE_SAMPLES);
    size_t ndesc = 0;
    for (const GateSlice &sl : gs.slices) ndesc += (size_t)(sl.wend - sl.wbeg) + 1;
    // ---- in: the tile descriptors of every slice; out, by packed sample slot: res6 | redundancy | cov36 | chi2 | status, then by bias state:
    // frame_stats4 (the reduction reads redundancy and chi2, so they exist whenever the call factors)
    const size_t nf = full ? M : 0;
    CovScratch scr(full, (size_t)dev_.Utot, sizeof(ImuGateRec), gs.nrec);
    CallLayout io = head_;
    const int s_desc = io.add("wtile", sizeof(int32_t), full ? ndesc : 0, false), s_res = io.add("res6", sizeof(double), 6 * M, true),
              s_red = io.add("redundancy", sizeof(double), nf, true), s_cov = io.add("cov36", sizeof(double), cov36 ? 36 * M : 0, true),
              s_chi = io.add("chi2", sizeof(double), nf, true), s_stat = io.add("status", sizeof(int32_t), M, false),
              s_fs = io.add("frame_stats4", sizeof(double), frame_stats4 ? 4 * F : 0, true);
    if (const int rc = reserve_call(io, full ? &scr.lay : nullptr)) return rc;
    std::vector<size_t> desc0;   // every slice's first descriptor
    if (full) {
      int32_t *hd = io_host<int32_t>(io, s_desc);
      size_t at = 0;
      for (const GateSlice &sl : gs.slices) {
        const std::vector<int32_t> first = plan_imugate_tiles(gs.counts.data(), sl.wbeg, sl.wend, IMUG_PER_TILE);
        std::memcpy(hd + at, first.data(), sizeof(int32_t) * first.size());
        desc0.push_back(at);
        at += first.size();
      }
    }
    const ImuGateOut out{io_dev<double>(io, s_res), full ? io_dev<double>(io, s_red) : nullptr, cov36 ? io_dev<double>(io, s_cov) : nullptr,
                         full ? io_dev<double>(io, s_chi) : nullptr, io_dev<int32_t>(io, s_stat), s0, 0, o->min_redundancy};
    const int rc = run_gate(
        io, s_desc, s_res, full ? &scr : nullptr, gs, &WinMeta::imu0, s0, (int)M,
        [&](QueryRun &x, int first, int n) {
          hipLaunchKernelGGL(k_cov_imugate_jac, dim3(nblk(n, 64)), dim3(64), 0, stream_, dev_, first, n, x.excl, x.rec<ImuGateRec>(), out);
        },
        [&](QueryRun &x, size_t si, int first, int) {
          const GateSlice &sl = gs.slices[si];
          CovSolveIO<COV_IMUGATE> a;
          a.rec = x.rec<ImuGateRec>(); a.slot_base = first; a.igate = out;
          a.wtile = io_dev<int32_t>(io, s_desc) + desc0[si]; a.wt_n = sl.wend - sl.wbeg; a.wt_w0 = sl.wbeg;
          launch_cov_solve(x.c, (size_t)io_host<int32_t>(io, s_desc)[desc0[si] + (size_t)a.wt_n], a);
        },
        [&](QueryRun &) {
          if (frame_stats4)
            hipLaunchKernelGGL(k_cov_imugate_reduce, dim3(nblk((int)F, 64)), dim3(64), 0, stream_, dev_, f0, (int)F, out, io_dev<double>(io, s_fs));
        });
    if (rc) return rc;
    // ---- results, in the caller's sample order.  Precedence 2, 1 (the window's factorisation failed), 4, 0.
    const Lm *lm = io_host<Lm>(io, HEAD_LM);
    const double *hres = io_host<double>(io, s_res), *hred = io_host<double>(io, s_red), *hcov = io_host<double>(io, s_cov), *hchi = io_host<double>(io, s_chi);
    const int32_t *hstat = io_host<int32_t>(io, s_stat);
    for (int w = wbeg; w < wend; ++w) {
      const bool bad = full && lm[w].chol_fail != 0;
      for (size_t b = imu_moff_[(size_t)w]; b < imu_moff_[(size_t)w + 1]; ++b) {
        const size_t i = b - m0, k = (size_t)(imu_slot_[b] - s0);
        const int st = gate_scatter(GATE_CODES, hstat[k], bad, 6, hred + k, hcov + 36 * k, hchi + k, red ? red + i : nullptr, cov36 ? cov36 + 36 * i : nullptr,
                                    chi2 ? chi2 + i : nullptr);
        if (res6) std::memcpy(res6 + 6 * i, hres + 6 * k, sizeof(double) * 6);
        if (status) status[i] = st;
      }
    }
    if (frame_stats4) std::memcpy(frame_stats4, io_host<double>(io, s_fs), sizeof(double) * 4 * F);
    return CTVIO_OK;
  }
  // ctvio_predict_landmarks_batch / ctvio_predict_landmarks (only >= 0: every prediction belongs to that window, win is not read): where
  // landmark lm[i] falls in the camera at the IMU-predicted pose of prediction pred[i], row row[i], beyond the spline, with its 2 x 2
  // covariance and gate.  The predictions are imu_predict()'s queries (grouped by window, stable), the points are grouped by the window of
  // their prediction, eight to a tile of kind TILE_PRED.  The launches of its run_query: k_cov_nav_jac on the predictions' start times,
  // k_imu_transition (end state, Phi, N), k_cov_pred_jac (value, status, record), k_cov_solve<COV_PRED>; a fourth timing slot.
  int predict_landmarks(int only, int64_t np64, const int32_t *win, const int32_t *frame, const int32_t *n_imu, const int64_t *imu_t, const double *imu_gyro,
                        const double *imu_acc, const ctvio_imu_noise *noise, int64_t nq64, const int32_t *pred, const int32_t *lmi, const int32_t *row,
                        const ctvio_row_model *rm, const double *obs2, double *state16, double *proj3, double *cov4, double *chi2, int32_t *row_out,
                        int32_t *status) {
    if (const int rc = only >= 0 ? guard(only) : guard()) return rc;
    if (!check_count(np64) || !check_count(nq64)) return fail(CTVIO_ERR_INVALID, "bad arguments");
    if (np64 == 0 || nq64 == 0) return CTVIO_OK;
    if (!n_imu || !imu_t || !imu_gyro || !imu_acc || !noise || (only < 0 && (!win || !pred)) || !lmi || !row || (!proj3 && !cov4 && !chi2 && !state16) ||
        (chi2 && !obs2))
      return fail(CTVIO_ERR_INVALID, "bad arguments");
    ProjRowModel prm{0.0, 0.0, 1, 0};
    if (rm) {
      if (rm->iterations < 1 || rm->iterations > 8 || rm->rows < 1 || !std::isfinite(rm->fy) || !std::isfinite(rm->cy))
        return fail(CTVIO_ERR_INVALID, "row model: iterations in 1 .. 8, rows >= 1, finite fy and cy");
      prm = ProjRowModel{rm->fy, rm->cy, rm->rows, rm->iterations};
    }
    ImuSamples sam;
    if (!sam.noise(*noise)) return fail(CTVIO_ERR_INVALID, sam.error);
    const int np = (int)np64, nq = (int)nq64;
    const size_t npp = (size_t)np, nn = (size_t)nq;
    const QueryOrder ordp(only, np, win, dev_.nwin);
    if (!ordp.error().empty()) return fail(CTVIO_ERR_INVALID, "prediction: " + ordp.error());
    if (!sam.streams("prediction", only, np, win, frame, meta_.data(), n_imu, imu_t, imu_gyro, imu_acc)) return fail(CTVIO_ERR_INVALID, sam.error);
    const std::vector<int64_t> &first = sam.first;   // first sample of every prediction (the caller's order)
    std::vector<int32_t> pwin(nn), rank(npp);   // the window of every point; the sorted position of every prediction
    for (int r = 0; r < np; ++r) rank[(size_t)ordp.slot[(size_t)r]] = r;
    for (int i = 0; i < nq; ++i) {
      const std::string what = "point " + std::to_string(i);
      if (pred && (pred[i] < 0 || pred[i] >= np)) return fail(CTVIO_ERR_INVALID, what + ": prediction index out of range");
      const int w = only >= 0 ? only : win[pred[i]];
      pwin[(size_t)i] = w;
      if (lmi[i] < 0 || lmi[i] >= meta_[w].L) return fail(CTVIO_ERR_INVALID, what + ": landmark index out of range");
      if (obs2 && !(std::isfinite(obs2[2 * (size_t)i]) && std::isfinite(obs2[2 * (size_t)i + 1]))) return fail(CTVIO_ERR_INVALID, what + ": non-finite candidate point");
    }
    const QueryOrder ordq(only, nq, pwin.data(), dev_.nwin);
    const bool want_cov = cov4 || chi2;
    const size_t nc = want_cov ? nn : 0;
    const std::vector<CovTile> tiles = want_cov ? query_tiles(ordq, PRJ_PER_TILE, TILE_PRED) : std::vector<CovTile>();
    // ---- io: start-time queries, propagation queries, samples, points, tiles (in, one staged copy); state16 | proj3 | cov4 | chi2 | row |
    // status | the predictions' statuses (out, one copy).  scr: mask, exclusions, point records; start records, start states, Phi | N
    CovScratch cs(want_cov, (size_t)dev_.Utot, sizeof(PredRec), nn);
    CallLayout io = head_, &scr = cs.lay;
    const int s_q = io.add("queries", sizeof(NavQuery), npp, false), s_pq = io.add("prop", sizeof(PropQuery), npp, false);
    sam.add(io);
    const int s_pts = io.add("points", sizeof(PredPoint), nn, false),
              s_tiles = io.add("tiles", sizeof(CovTile), tiles.size(), false), s_state = io.add("state16", sizeof(double), 16 * npp, true),
              s_proj = io.add("proj3", sizeof(double), 3 * nn, true), s_cov = io.add("cov4", sizeof(double), 4 * nc, true),
              s_chi = io.add("chi2", sizeof(double), nc, true), s_row = io.add("row", sizeof(int32_t), nn, false),
              s_stat = io.add("status", sizeof(int32_t), nn, false), s_pstat = io.add("pred_status", sizeof(int32_t), npp, false);
    const int s_nrec = scr.add("start_records", sizeof(NavRec), want_cov ? npp : 0, false), s_x0 = scr.add("state0", sizeof(double), 16 * npp, true),
              s_tr = scr.add("transition", sizeof(double), want_cov ? TRN_OUT * npp : 0, true);
    if (const int rc = reserve_call(io, &scr)) return rc;
    NavQuery *hq = io_host<NavQuery>(io, s_q);
    PropQuery *hp = io_host<PropQuery>(io, s_pq);
    for (int r = 0; r < np; ++r) {
      const size_t i = (size_t)ordp.slot[(size_t)r];
      const int w = ordp.win_of(r);
      hq[r] = NavQuery{w, frame ? frame[i] : meta_[w].F - 1, (long long)(imu_t[first[i]] - t0_[w])};
      hp[r] = PropQuery{w, n_imu[i], (long long)first[i], (long long)r};
    }
    PredPoint *hpt = io_host<PredPoint>(io, s_pts);
    for (int r = 0; r < nq; ++r) {
      const size_t i = (size_t)ordq.slot[(size_t)r], pi = pred ? (size_t)pred[i] : 0;   // (pred null: the single-window entry's one prediction)
      hpt[r] = PredPoint{ordq.win_of(r), rank[pi], lmi[i], row[i], (long long)(first[pi + 1] - 1), {obs2 ? obs2[2 * i] : 0.0, obs2 ? obs2[2 * i + 1] : 0.0}};
    }
    stage_tiles(io, -1, s_tiles, ordq, tiles);
    sam.stage(io, call_io_.host);
    const ImuNoise nz{noise->gyr_n, noise->acc_n, noise->gyr_w, noise->acc_w};
    double *x0 = scr.at<double>(call_scr_.dev, s_x0), *tr = scr.at<double>(call_scr_.dev, s_tr);
    NavRec *nrec = scr.at<NavRec>(call_scr_.dev, s_nrec);
    // the launches: k_cov_nav_jac on the start times (untimed), k_imu_transition (ms[3]), k_cov_pred_jac (ms[2]), with covariances k_cov_solve (ms[1])
    const int rc = run_query(
        io, s_q, s_state, want_cov ? &cs : nullptr, {{2, EV_QUERY_END, EV_COV_GRAM}, {3, EV_QUERY_BEGIN, EV_QUERY_END}},
        {span_prepare(), {1, EV_COV_GRAM, EV_CALL_END}, {2, EV_QUERY_END, EV_COV_GRAM}, {3, EV_QUERY_BEGIN, EV_QUERY_END}}, [&](QueryRun &x) {
          hipLaunchKernelGGL(k_cov_nav_jac, dim3(nblk(np, 64)), dim3(64), 0, stream_, dev_, np, io_dev<NavQuery>(io, s_q), x.excl, nrec, x0, io_dev<int32_t>(io, s_pstat));
          x.mark(EV_QUERY_BEGIN);
          hipLaunchKernelGGL(k_imu_transition, dim3(nblk(np, 4)), dim3(64), 0, stream_, dev_, np, io_dev<PropQuery>(io, s_pq), io_dev<int32_t>(io, s_pstat),
                             io_dev<long long>(io, sam.s_t), io_dev<double>(io, sam.s_gyro), io_dev<double>(io, sam.s_acc), nz, want_cov ? 1 : 0, (const double *)x0,
                             io_dev<double>(io, s_state), tr);
          x.mark(EV_QUERY_END);
          hipLaunchKernelGGL(k_cov_pred_jac, dim3(nblk(nq, 64)), dim3(64), 0, stream_, dev_, nq, io_dev<PredPoint>(io, s_pts), x.excl, prm, io_dev<int32_t>(io, s_pstat),
                             io_dev<double>(io, s_state), io_dev<double>(io, sam.s_gyro), (const NavRec *)nrec, (const double *)tr, x.rec<PredRec>(),
                             io_dev<double>(io, s_proj), io_dev<int32_t>(io, s_row), io_dev<int32_t>(io, s_stat));
          x.mark(EV_COV_GRAM);
          if (!x.excl) return;
          CovSolveIO<COV_PRED> a;
          a.tiles = io_dev<CovTile>(io, s_tiles); a.rec = x.rec<PredRec>(); a.blocks = io_dev<double>(io, s_cov);
          if (chi2) a.chi2 = io_dev<double>(io, s_chi);
          launch_cov_solve(x.c, tiles.size(), a);
        });
    if (rc) return rc;
    // ---- results (not computable: NaN; a start time outside the spline: its state NaN)
    const Lm *lm = io_host<Lm>(io, HEAD_LM);
    const double *hstate = io_host<double>(io, s_state), *hproj = io_host<double>(io, s_proj), *hcov = io_host<double>(io, s_cov), *hchi = io_host<double>(io, s_chi);
    const int32_t *hrow = io_host<int32_t>(io, s_row), *hstat = io_host<int32_t>(io, s_stat), *hps = io_host<int32_t>(io, s_pstat);
    for (int r = 0; r < np && state16; ++r) {
      double *o = state16 + 16 * (size_t)ordp.slot[(size_t)r];
      if (hps[r] != POSE_OUTSIDE) std::memcpy(o, hstate + 16 * (size_t)r, sizeof(double) * 16);
      else std::fill(o, o + 16, std::nan(""));
    }
    for (int r = 0; r < nq; ++r) {
      const size_t i = (size_t)ordq.slot[(size_t)r];
      const int st = want_cov ? merge_status(hstat[r], lm[ordq.win_of(r)].chol_fail != 0) : hstat[r];
      if (cov4) cov_block(cov4 + 4 * i, hcov + 4 * (size_t)r, 2, st);
      if (chi2) chi2[i] = gate_value(hchi[r], st);
      if (proj3) std::memcpy(proj3 + 3 * i, hproj + 3 * (size_t)r, sizeof(double) * 3);
      if (row_out) row_out[i] = hrow[r];
      if (status) status[i] = st;
    }
    return CTVIO_OK;
  }
  // ---------------------------------------------------------------------------------------- landmark depths
  // ctvio_triangulate_batch / ctvio_triangulate (single: window `only` alone) and ctvio_shift_anchor_batch: one kernel each
  // (csrc/kernels_tri.hpp) on the current state.  dev_, plan_ and the captured graph are not touched.
  static TriOpts tri_opts(const ctvio_triangulate_options &o) {
    return TriOpts{o.row_times != 0, o.only_unset != 0, o.apply != 0, 0, o.min_depth, o.init_depth};
  }
  int tri_timing() { return span_timing({{0, EV_QUERY_BEGIN, EV_QUERY_END}}); }   // ms[0]: the kernel between the query events, ms[7]: the whole call
  int triangulate(bool single, int only, const ctvio_triangulate_options *o, double *depth, int32_t *flag) {
    if (const int rc = single ? guard(only) : guard()) return rc;
    if (!o) return fail(CTVIO_ERR_INVALID, "null options");
    const int l0 = single ? meta_[only].lm0 : 0, n = single ? meta_[only].L : dev_.Ltot;
    CallLayout io = head_;
    const int s_dep = io.add("depth", sizeof(double), (size_t)n, true), s_flag = io.add("flag", sizeof(int32_t), (size_t)n, false);
    if (const int rc = reserve_call(io)) return rc;
    HIPCHK(hipEventRecord(ev_[EV_CALL_BEGIN], stream_));
    HIPCHK(hipEventRecord(ev_[EV_QUERY_BEGIN], stream_));
    if (n) hipLaunchKernelGGL(k_triangulate, dim3(nblk(n, 4)), dim3(256), 0, stream_, dev_, l0, n, tri_opts(*o), io_dev<double>(io, s_dep), io_dev<int32_t>(io, s_flag));
    HIPCHK(hipEventRecord(ev_[EV_QUERY_END], stream_));
    if (n) HIPCHK(hipMemcpyAsync(io_host<char>(io, s_dep), io_dev<char>(io, s_dep), io.bytes() - io.off(s_dep), hipMemcpyDeviceToHost, stream_));   // (depth | flag)
    HIPCHK(hipEventRecord(ev_[EV_CALL_END], stream_));
    if (const int rc = sync_call()) return rc;
    if (const int rc = tri_timing()) return rc;
    if (depth && n) std::memcpy(depth, io_host<double>(io, s_dep), sizeof(double) * (size_t)n);
    if (flag && n) std::memcpy(flag, io_host<int32_t>(io, s_flag), sizeof(int32_t) * (size_t)n);
    return CTVIO_OK;
  }
  // ctvio_landmark_points_batch / ctvio_landmark_points (single: window `only` alone): the world point of every landmark and its 3 x 3
  // covariance.  Points only (cov9 null): k_cov_point_jac alone, nothing is linearised or factored.  Otherwise k_cov_point_jac with the
  // Jacobians (one record per landmark, after k_cov_prepare: it reads 1 / Hll) and k_cov_solve on tiles of kind TILE_POINT, five landmarks
  // each in the sorted order of the rows of W (run_query).
  int landmark_points(bool single, int only, double *point3, double *cov9, int32_t *status) {
    if (const int rc = single ? guard(only) : guard()) return rc;
    const int nw = dev_.nwin, wbeg = single ? only : 0, wend = single ? only + 1 : nw;
    const int l0 = single ? meta_[only].lm0 : 0, n = single ? meta_[only].L : dev_.Ltot;
    if (n == 0) return CTVIO_OK;
    const size_t nn = (size_t)n;
    const bool want_cov = cov9 != nullptr;
    std::vector<CovTile> tiles;
    for (int w = wbeg; w < wend && want_cov; ++w)
      for (int r = 0; r < meta_[w].L; r += LMP_PER_TILE) tiles.push_back(CovTile{w, TILE_POINT, r, std::min(LMP_PER_TILE, meta_[w].L - r), 0});
    // ---- io: tiles (in, one staged copy); cov9 | point3 | status (out, one copy).  The records: one per landmark of the batch
    CovScratch scr(want_cov, (size_t)dev_.Utot, sizeof(PointRec), (size_t)dev_.Ltot);
    CallLayout io = head_;
    const int s_tiles = io.add("tiles", sizeof(CovTile), tiles.size(), false), s_cov = io.add("cov9", sizeof(double), want_cov ? 9 * nn : 0, true),
              s_pt = io.add("point3", sizeof(double), 3 * nn, true), s_stat = io.add("status", sizeof(int32_t), nn, false);
    if (const int rc = reserve_call(io, want_cov ? &scr.lay : nullptr)) return rc;
    if (want_cov) std::memcpy(io_host<CovTile>(io, s_tiles), tiles.data(), sizeof(CovTile) * tiles.size());
    // (points only: nothing goes in, and the kernel's time is reported as the triangulation's is, ms[0])
    const int rc = run_query(
        io, s_tiles, s_cov, want_cov ? &scr : nullptr,
        [&](QueryRun &x) {
          hipLaunchKernelGGL(k_cov_point_jac, dim3(nblk(n, 64)), dim3(64), 0, stream_, dev_, l0, n, x.excl ? 1 : 0, x.rec<PointRec>(), io_dev<double>(io, s_pt),
                             io_dev<int32_t>(io, s_stat));
        },
        [&](QueryRun &x) {
          CovSolveIO<COV_BASE> a;
          a.tiles = io_dev<CovTile>(io, s_tiles); a.lrec = x.rec<PointRec>(); a.lm_cov = io_dev<double>(io, s_cov); a.lm_base = l0;
          launch_cov_solve(x.c, tiles.size(), a);
        },
        0);
    if (rc) return rc;
    // ---- results (not computable: NaN)
    const Lm *lm = io_host<Lm>(io, HEAD_LM);
    const double *hcov = io_host<double>(io, s_cov);
    const int32_t *hstat = io_host<int32_t>(io, s_stat);
    if (point3) std::memcpy(point3, io_host<double>(io, s_pt), sizeof(double) * 3 * nn);
    size_t i = 0;
    for (int w = wbeg; w < wend; ++w)
      for (int l = 0; l < meta_[w].L; ++l, ++i) {
        const int st = want_cov ? merge_status(hstat[i], lm[w].chol_fail != 0) : hstat[i];
        if (want_cov) cov_block(cov9 + 9 * i, hcov + 9 * i, 3, st);
        if (status) status[i] = st;
      }
    return CTVIO_OK;
  }
  int shift_anchor(const ctvio_triangulate_options *o, int64_t n64, const int32_t *win, const int32_t *lm, const int64_t *t_new, const int32_t *row_new,
                   double *depth_new, int32_t *flag) {
    if (const int rc = guard()) return rc;
    if (!o) return fail(CTVIO_ERR_INVALID, "null options");
    if (!check_count(n64) || (n64 && (!win || !lm || !t_new))) return fail(CTVIO_ERR_INVALID, "bad arguments");
    if (!row_new && o->row_times) return fail(CTVIO_ERR_INVALID, "row_new may be null only with row_times = 0");
    const int n = (int)n64;
    const size_t nn = (size_t)n;
    for (int i = 0; i < n; ++i) {
      if (win[i] < 0 || win[i] >= dev_.nwin) return fail(CTVIO_ERR_INVALID, "query " + std::to_string(i) + ": window id out of range");
      if (lm[i] < 0 || lm[i] >= meta_[win[i]].L) return fail(CTVIO_ERR_INVALID, "query " + std::to_string(i) + ": landmark index out of range");
    }
    if (n == 0) return CTVIO_OK;
    // in: relative times | windows, landmarks, rows (one staged copy); out: depth | flag (one copy)
    CallLayout io = head_;
    const int s_rel = io.add("t_rel", sizeof(long long), nn, false), s_q = io.add("win_lm_row", sizeof(int32_t), 3 * nn, false),
              s_dep = io.add("depth_new", sizeof(double), nn, true), s_flag = io.add("flag", sizeof(int32_t), nn, false);
    if (const int rc = reserve_call(io)) return rc;
    long long *rel = io_host<long long>(io, s_rel);
    int32_t *hq = io_host<int32_t>(io, s_q), *dq = io_dev<int32_t>(io, s_q);
    for (int i = 0; i < n; ++i) rel[i] = (long long)(t_new[i] - t0_[win[i]]);
    std::memcpy(hq, win, sizeof(int32_t) * nn); std::memcpy(hq + nn, lm, sizeof(int32_t) * nn);
    if (row_new) std::memcpy(hq + 2 * nn, row_new, sizeof(int32_t) * nn); else std::memset(hq + 2 * nn, 0, sizeof(int32_t) * nn);
    HIPCHK(hipEventRecord(ev_[EV_CALL_BEGIN], stream_));
    HIPCHK(hipMemcpyAsync(io_dev<char>(io, s_rel), rel, io.off(s_dep) - io.off(s_rel), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipEventRecord(ev_[EV_QUERY_BEGIN], stream_));
    hipLaunchKernelGGL(k_shift_anchor, dim3(nblk(n, 256)), dim3(256), 0, stream_, dev_, n, dq, dq + nn, io_dev<long long>(io, s_rel), dq + 2 * nn, tri_opts(*o),
                       io_dev<double>(io, s_dep), io_dev<int32_t>(io, s_flag));
    HIPCHK(hipEventRecord(ev_[EV_QUERY_END], stream_));
    HIPCHK(hipMemcpyAsync(io_host<char>(io, s_dep), io_dev<char>(io, s_dep), io.bytes() - io.off(s_dep), hipMemcpyDeviceToHost, stream_));   // (depth | flag)
    HIPCHK(hipEventRecord(ev_[EV_CALL_END], stream_));
    if (const int rc = sync_call()) return rc;
    if (const int rc = tri_timing()) return rc;
    if (depth_new) std::memcpy(depth_new, io_host<double>(io, s_dep), sizeof(double) * nn);
    if (flag) std::memcpy(flag, io_host<int32_t>(io, s_flag), sizeof(int32_t) * nn);
    return CTVIO_OK;
  }
  int last_timing(double *ms8, int32_t *n8) {
    if (ms8) std::copy(timing_.ms, timing_.ms + 8, ms8);
    if (n8) std::copy(timing_.n, timing_.n + 8, n8);
    return CTVIO_OK;
  }
  int set_profiling(int on) { profiling_requested_ = on != 0; return CTVIO_OK; }

 private:
  ctvio_options opt_;
  const DebugSwitches dbg_;   // environment switches as they were when the handle was created
  int marg_ran_on_host_ = 0;  // the last ctvio_marginalize(_batch) call: 1 if the factorisation ran on the host
  hipStream_t stream_ = nullptr;
  hipEvent_t ev_[EV_COUNT] = {};
  bool uploaded_ = false, profiling_ = false, profiling_requested_ = false;
  Timing timing_{};          // what ctvio_last_timing reports: the last solve, covariance, triangulation or anchor-shift call
  std::vector<hipEvent_t> pev_;
  std::vector<int> pev_phase_;
  size_t pev_used_ = 0;
  std::vector<std::unique_ptr<HostWindow>> own_;   // windows recorded by ctvio_add_window (owning copies)
  std::vector<WinMeta> meta_;
  std::vector<int64_t> t0_;
  Dev dev_;
  BatchFacts facts_;         // the uploaded batch as the offset pass saw it (+ its factorisation): what make_plan reads
  LaunchPlan plan_;          // the launch list of the uploaded batch
  size_t state_doubles_ = 0;
  Arena in_, work_;          // uploaded inputs (pinned mirror) / device-only work buffers
  WorkerPool pool_;          // the handle's packing threads (created on first use, kept)
  Arena call_io_, call_scr_;   // scratch of the per-call entries: copied in or out (pinned mirror) / device only
  CallLayout head_;            // the fixed head of call_io_ (HEAD_*), laid out by the upload
  // CTVIO_POISON: a reused handle's scratch holds the numbers of earlier calls in another layout, a fresh one zeros.  A kernel that reads
  // an entry it never wrote and masks it by a product instead of a select is right on zeros only; with the switch every double buffer
  // the next call reuses starts as a quiet NaN (1) or as a large finite value (2, caught where fmax / fmin or a comparison would drop a
  // NaN).  Integer buffers are never poisoned.  With the switch off: nothing (one branch per call).
  hipError_t poison(void *p, size_t bytes) {
    if (!dbg_.poison || bytes < 4) return hipSuccess;
    const uint32_t pattern = dbg_.poison == 2 ? 0x5F5F5F5Fu : 0x7FF8DEADu;
    return hipMemsetD32Async((hipDeviceptr_t)p, (int)pattern, bytes / 4, stream_);
  }
  bool marg_attr_set_ = false;
  double *snap_ = nullptr;   // state snapshot (inside work_)
  int graph_captures_ = 0;                // how many times the pass was captured (ctvio_graph_captures: a stream of equal batches captures once)
  hipGraphExec_t graph_exec_ = nullptr;   // one LM pass (launch_pass) as a graph, valid while dev_ == graph_dev_ and plan_ == graph_plan_
  Dev graph_dev_;
  LaunchPlan graph_plan_;
  bool snap_valid_ = false;
  const double *h_ld_ = nullptr;        // the line delays as uploaded (same arena)
  std::vector<int32_t> gate_slot_;   // [sum V] the absolute block slot of every caller's block, window after window (gate_voff_: nwin + 1 offsets)
  std::vector<size_t> gate_voff_;
  std::vector<int32_t> imu_slot_;    // [sum M] the absolute packed slot of every caller's IMU sample, window after window (imu_moff_: nwin + 1 offsets)
  std::vector<size_t> imu_moff_;
  const int32_t *h_lm_pos_ = nullptr;   // host mirror of Dev::lm_pos (inside in_.host: valid while the batch is uploaded)
};

}  // namespace ctv

// ================================================================================================ C ABI
struct ctvio_solver {
  ctv::SolverImpl impl;
};

extern "C" {

void ctvio_default_options(ctvio_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->device = 0; o->precision = CTVIO_FP64; o->use_mfma = 1; o->check_every = 4;
  o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
  o->initial_radius = 1e4; o->max_radius = 1e16; o->min_radius = 1e-32; o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32; o->max_consecutive_invalid_steps = 5;
  o->deterministic = -1; o->host_threads = 0; o->use_graph = 1; o->line_search = 1;
}
const char *ctvio_status_string(int32_t s) {
  switch (s) {
    case CTVIO_OK: return "ok";
    case CTVIO_ERR_INVALID: return "invalid argument";
    case CTVIO_ERR_NO_DEVICE: return "no HIP device (the product path has no CPU fallback)";
    case CTVIO_ERR_HIP: return "HIP runtime error";
    case CTVIO_ERR_STATE: return "call order violated";
    case CTVIO_ERR_INTERNAL: return "internal consistency check failed";
    default: return "unknown status";
  }
}
const char *ctvio_last_error(void) { return ctv::g_err.c_str(); }
int32_t ctvio_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int32_t ctvio_create(const ctvio_options *opt, ctvio_solver **out) {
  if (!out) return ctv::fail(CTVIO_ERR_INVALID, "null out");
  *out = nullptr;
  ctvio_options o;
  if (opt) o = *opt; else ctvio_default_options(&o);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ctv::fail(CTVIO_ERR_NO_DEVICE, "hipGetDeviceCount found no device");
  if (o.device < 0 || o.device >= n) return ctv::fail(CTVIO_ERR_INVALID, "device ordinal out of range");
  if (o.precision != CTVIO_FP64) return ctv::fail(CTVIO_ERR_INVALID, "precision: only CTVIO_FP64 exists (the mixed fp32 mode was removed: it missed the 1e-4 contract)");
  if (o.use_mfma != 1 && o.use_mfma != 2) return ctv::fail(CTVIO_ERR_INVALID, "use_mfma: 1 or 2 (the vector-ALU cross-check kernels of use_mfma = 0 were removed: the oracle is the cross-check)");
  std::unique_ptr<ctvio_solver> s(new ctvio_solver{ctv::SolverImpl(o)});
  if (const int rc = s->impl.init()) return rc;
  *out = s.release();
  return CTVIO_OK;
}
void ctvio_destroy(ctvio_solver *s) { delete s; }
// every entry point: null check, then the solver's device becomes current on this thread -- HIP's current device is per thread
// (default 0), and a multi-GPU rank that drives several solver handles from worker threads would otherwise launch on device 0
#define CHK_S if (!s) return ctv::fail(CTVIO_ERR_INVALID, "null solver"); if (int rc_bind_ = s->impl.bind()) return rc_bind_
int32_t ctvio_clear(ctvio_solver *s) { CHK_S; return s->impl.clear(); }
int32_t ctvio_add_window(ctvio_solver *s, const ctvio_window *w, int32_t *id) { CHK_S; return s->impl.add_window(w, id); }
int32_t ctvio_upload(ctvio_solver *s) { CHK_S; return s->impl.upload(); }
int32_t ctvio_set_batch(ctvio_solver *s, int32_t n, const ctvio_window *wins) { CHK_S; return s->impl.set_batch(n, wins); }
int32_t ctvio_num_windows(const ctvio_solver *s) { return s ? s->impl.num_windows() : 0; }
int32_t ctvio_solve(ctvio_solver *s, int32_t max_iterations, ctvio_summary *out) { CHK_S; return s->impl.solve(max_iterations, out); }
int32_t ctvio_get_state(ctvio_solver *s, int32_t id, double *quat, double *pos, double *bias, double *rho, double *ld) {
  CHK_S; return s->impl.get_state(id, quat, pos, bias, rho, ld);
}
int32_t ctvio_get_batch_state(ctvio_solver *s, double *quat, double *pos, double *bias, double *rho, double *ld) {
  CHK_S; return s->impl.get_batch_state(quat, pos, bias, rho, ld);
}
int32_t ctvio_set_state(ctvio_solver *s, int32_t id, const double *quat, const double *pos, const double *bias, const double *rho, double ld) {
  CHK_S; return s->impl.set_state(id, quat, pos, bias, rho, ld);
}
int32_t ctvio_linearize(ctvio_solver *s, int32_t id, double *Hpp, double *W, double *Hll, double *g, double *cost) {
  CHK_S; return s->impl.linearize(id, Hpp, W, Hll, g, cost);
}
int32_t ctvio_cost(ctvio_solver *s, int32_t id, double *cost) { CHK_S; return s->impl.cost(id, cost); }
int32_t ctvio_lm_step(ctvio_solver *s, int32_t id, double mu, double *delta, double *model_cost_change) {
  CHK_S; return s->impl.lm_step(id, mu, delta, model_cost_change);
}
int32_t ctvio_marginalize(ctvio_solver *s, int32_t id, const int8_t *role, double eps, int32_t *n_keep, int32_t *kept, double *J0, double *r0) {
  CHK_S; return s->impl.marginalize(id, role, eps, n_keep, kept, J0, r0);
}
int32_t ctvio_covariance_batch(ctvio_solver *s, const int32_t *n_sel, const int32_t *sel, double *cov, double *var_rho, int32_t *singular) {
  CHK_S; return s->impl.covariance(-1, n_sel, sel, cov, var_rho, singular);
}
int32_t ctvio_covariance(ctvio_solver *s, int32_t id, int32_t n_sel, const int32_t *sel, double *cov, double *var_rho, int32_t *singular) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.covariance(id, &n_sel, sel, cov, var_rho, singular);
}
int32_t ctvio_pose_covariance_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int64_t *t_ns, const double *q_SI, const double *p_SI,
                                    double *cov36, int32_t *status) {
  CHK_S; return s->impl.pose_covariance(-1, n, win, t_ns, q_SI, p_SI, cov36, status);
}
int32_t ctvio_pose_covariance(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_ns, const double *q_SI, const double *p_SI, double *cov36,
                              int32_t *status) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.pose_covariance(id, n, nullptr, t_ns, q_SI, p_SI, cov36, status);
}
int32_t ctvio_landmark_points_batch(ctvio_solver *s, double *point3, double *cov9, int32_t *status) {
  CHK_S; return s->impl.landmark_points(false, 0, point3, cov9, status);
}
int32_t ctvio_landmark_points(ctvio_solver *s, int32_t id, double *point3, double *cov9, int32_t *status) {
  CHK_S; return s->impl.landmark_points(true, id, point3, cov9, status);
}
int32_t ctvio_nav_state_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int64_t *t_ns, const int32_t *frame, double *state16,
                              double *cov225, int32_t *status) {
  CHK_S; return s->impl.nav_state(-1, n, win, t_ns, frame, state16, cov225, status);
}
int32_t ctvio_nav_state(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_ns, const int32_t *frame, double *state16, double *cov225,
                        int32_t *status) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.nav_state(id, n, nullptr, t_ns, frame, state16, cov225, status);
}
int32_t ctvio_body_rates_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int64_t *t_ns, const int32_t *frame, const double *meas6,
                               const double *noise6, double *rates9, double *cov225, double *chi2, int32_t *status) {
  CHK_S; return s->impl.body_rates(-1, n, win, t_ns, frame, meas6, noise6, rates9, cov225, chi2, status);
}
int32_t ctvio_body_rates(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_ns, const int32_t *frame, const double *meas6,
                         const double *noise6, double *rates9, double *cov225, double *chi2, int32_t *status) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.body_rates(id, n, nullptr, t_ns, frame, meas6, noise6, rates9, cov225, chi2, status);
}
void ctvio_default_imu_noise(ctvio_imu_noise *o) {
  if (!o) return;
  o->gyr_n = 4.0e-3; o->acc_n = 8.0e-2; o->gyr_w = 2.0e-6; o->acc_w = 4.0e-5;
}
int32_t ctvio_imu_predict_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int32_t *frame, const int32_t *n_imu, const int64_t *imu_t,
                                const double *imu_gyro, const double *imu_acc, const ctvio_imu_noise *noise, int32_t last_only, double *state16,
                                double *cov225, int32_t *status) {
  CHK_S; return s->impl.imu_predict(-1, n, win, frame, n_imu, imu_t, imu_gyro, imu_acc, noise, last_only, state16, cov225, status);
}
int32_t ctvio_imu_predict(ctvio_solver *s, int32_t id, int32_t frame, int32_t m, const int64_t *imu_t, const double *imu_gyro, const double *imu_acc,
                          const ctvio_imu_noise *noise, int32_t last_only, double *state16, double *cov225, int32_t *status) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  if (frame < -1) return ctv::fail(CTVIO_ERR_INVALID, "bias state out of range");
  return s->impl.imu_predict(id, 1, nullptr, frame >= 0 ? &frame : nullptr, &m, imu_t, imu_gyro, imu_acc, noise, last_only, state16, cov225, status);
}
int32_t ctvio_relative_pose_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int64_t *t_a_ns, const int64_t *t_b_ns, const double *q_SI,
                                  const double *p_SI, double *rel7, double *cov36, int32_t *status) {
  CHK_S; return s->impl.relative_pose(-1, n, win, t_a_ns, t_b_ns, q_SI, p_SI, rel7, cov36, status);
}
int32_t ctvio_relative_pose(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_a_ns, const int64_t *t_b_ns, const double *q_SI,
                            const double *p_SI, double *rel7, double *cov36, int32_t *status) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.relative_pose(id, n, nullptr, t_a_ns, t_b_ns, q_SI, p_SI, rel7, cov36, status);
}
int32_t ctvio_project_landmarks_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int32_t *lm, const int64_t *t_ns, const int32_t *row,
                                      const ctvio_row_model *rm, const double *obs2, double *proj3, double *cov4, double *chi2, int32_t *row_out,
                                      int32_t *status) {
  CHK_S; return s->impl.project_landmarks(-1, n, win, lm, t_ns, row, rm, obs2, proj3, cov4, chi2, row_out, status);
}
int32_t ctvio_project_landmarks(ctvio_solver *s, int32_t id, int32_t n, const int32_t *lm, const int64_t *t_ns, const int32_t *row,
                                const ctvio_row_model *rm, const double *obs2, double *proj3, double *cov4, double *chi2, int32_t *row_out,
                                int32_t *status) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.project_landmarks(id, n, nullptr, lm, t_ns, row, rm, obs2, proj3, cov4, chi2, row_out, status);
}
int32_t ctvio_predict_landmarks_batch(ctvio_solver *s, int64_t n_pred, const int32_t *win, const int32_t *frame, const int32_t *n_imu, const int64_t *imu_t,
                                      const double *imu_gyro, const double *imu_acc, const ctvio_imu_noise *noise, int64_t n_pts, const int32_t *pred,
                                      const int32_t *lm, const int32_t *row, const ctvio_row_model *rm, const double *obs2, double *state16, double *proj3,
                                      double *cov4, double *chi2, int32_t *row_out, int32_t *status) {
  CHK_S;
  return s->impl.predict_landmarks(-1, n_pred, win, frame, n_imu, imu_t, imu_gyro, imu_acc, noise, n_pts, pred, lm, row, rm, obs2, state16, proj3, cov4, chi2,
                                   row_out, status);
}
int32_t ctvio_predict_landmarks(ctvio_solver *s, int32_t id, int32_t frame, int32_t m, const int64_t *imu_t, const double *imu_gyro, const double *imu_acc,
                                const ctvio_imu_noise *noise, int32_t n_pts, const int32_t *lm, const int32_t *row, const ctvio_row_model *rm,
                                const double *obs2, double *state16, double *proj3, double *cov4, double *chi2, int32_t *row_out, int32_t *status) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.predict_landmarks(id, 1, nullptr, frame >= 0 ? &frame : nullptr, &m, imu_t, imu_gyro, imu_acc, noise, n_pts, nullptr, lm, row, rm, obs2, state16,
                                   proj3, cov4, chi2, row_out, status);
}
void ctvio_default_gate_options(ctvio_gate_options *o) {
  if (!o) return;
  o->min_redundancy = 0.01;
}
int32_t ctvio_visual_gate_batch(ctvio_solver *s, const ctvio_gate_options *o, double *res2, double *weight, double *depth, double *redundancy, double *cov4,
                                double *chi2, int32_t *status, double *lm_stats3, int32_t *lm_count) {
  CHK_S; return s->impl.visual_gate(-1, o, res2, weight, depth, redundancy, cov4, chi2, status, lm_stats3, lm_count);
}
int32_t ctvio_visual_gate(ctvio_solver *s, int32_t id, const ctvio_gate_options *o, double *res2, double *weight, double *depth, double *redundancy, double *cov4,
                          double *chi2, int32_t *status, double *lm_stats3, int32_t *lm_count) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.visual_gate(id, o, res2, weight, depth, redundancy, cov4, chi2, status, lm_stats3, lm_count);
}
int32_t ctvio_set_visual_active_batch(ctvio_solver *s, const uint8_t *active) { CHK_S; return s->impl.set_visual_active(-1, active); }
int32_t ctvio_set_visual_active(ctvio_solver *s, int32_t id, const uint8_t *active) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.set_visual_active(id, active);
}
int32_t ctvio_get_visual_active_batch(ctvio_solver *s, uint8_t *active) { CHK_S; return s->impl.get_visual_active(-1, active); }
int32_t ctvio_get_visual_active(ctvio_solver *s, int32_t id, uint8_t *active) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.get_visual_active(id, active);
}
void ctvio_default_cull_options(ctvio_cull_options *o) {
  if (!o) return;
  o->min_redundancy = 0.01;
  o->chi2_max = 9.21;
  o->mean_error_max = 0.0;
  o->worst_only = 0;
  o->drop_uncomputable = 1;
}
int32_t ctvio_cull_visual_batch(ctvio_solver *s, const ctvio_cull_options *o, int32_t *n_culled, uint8_t *active) {
  CHK_S; return s->impl.cull_visual(-1, o, n_culled, active);
}
int32_t ctvio_cull_visual(ctvio_solver *s, int32_t id, const ctvio_cull_options *o, int32_t *n_culled, uint8_t *active) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.cull_visual(id, o, n_culled, active);
}
int32_t ctvio_imu_gate_batch(ctvio_solver *s, const ctvio_gate_options *o, double *res6, double *redundancy, double *cov36, double *chi2, int32_t *status,
                             double *frame_stats4) {
  CHK_S; return s->impl.imu_gate(-1, o, res6, redundancy, cov36, chi2, status, frame_stats4);
}
int32_t ctvio_imu_gate(ctvio_solver *s, int32_t id, const ctvio_gate_options *o, double *res6, double *redundancy, double *cov36, double *chi2, int32_t *status,
                       double *frame_stats4) {
  CHK_S;
  if (id < 0) return ctv::fail(CTVIO_ERR_INVALID, "window id out of range");
  return s->impl.imu_gate(id, o, res6, redundancy, cov36, chi2, status, frame_stats4);
}
void ctvio_default_triangulate_options(ctvio_triangulate_options *o) {
  if (!o) return;
  o->row_times = 1; o->only_unset = 1; o->apply = 1;
  o->min_depth = 0.1;    // feature_manager.cpp:218
  o->init_depth = 5.0;   // parameters.cpp:44 INIT_DEPTH
}
int32_t ctvio_triangulate_batch(ctvio_solver *s, const ctvio_triangulate_options *o, double *depth, int32_t *flag) {
  CHK_S; return s->impl.triangulate(false, 0, o, depth, flag);
}
int32_t ctvio_triangulate(ctvio_solver *s, int32_t id, const ctvio_triangulate_options *o, double *depth, int32_t *flag) {
  CHK_S; return s->impl.triangulate(true, id, o, depth, flag);
}
int32_t ctvio_shift_anchor_batch(ctvio_solver *s, const ctvio_triangulate_options *o, int64_t n, const int32_t *win, const int32_t *lm,
                                 const int64_t *t_new, const int32_t *row_new, double *depth_new, int32_t *flag) {
  CHK_S; return s->impl.shift_anchor(o, n, win, lm, t_new, row_new, depth_new, flag);
}
int32_t ctvio_residual_summary(ctvio_solver *s, int32_t id, double *sums, int32_t *counts4) { CHK_S; return s->impl.residual_summary(id, sums, counts4); }
int32_t ctvio_marginalize_batch(ctvio_solver *s, const int8_t *role, double eps, int32_t *n_keep, int32_t *kept, double *J0, double *r0) {
  CHK_S; return s->impl.marginalize_batch(role, eps, n_keep, kept, J0, r0);
}
int32_t ctvio_gauge_restore(ctvio_solver *s, int32_t n, const int32_t *ids, const int32_t *knot, const double *q0, const double *t0) {
  CHK_S; return s->impl.gauge_restore(n, ids, knot, q0, t0);
}
int32_t ctvio_spline_eval(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_ns, double *pose7, double *vel3, double *omega3, double *acc3) {
  CHK_S; return s->impl.spline_eval(id, n, t_ns, pose7, vel3, omega3, acc3);
}
int32_t ctvio_spline_eval_batch(ctvio_solver *s, int64_t n, const int32_t *win, const int64_t *t_ns, double *pose7, double *vel3, double *omega3,
                                double *acc3, double *kernel_ms) {
  CHK_S; return s->impl.spline_eval_batch(n, win, t_ns, pose7, vel3, omega3, acc3, kernel_ms);
}
int32_t ctvio_sensor_pose(ctvio_solver *s, int32_t id, int32_t n, const int64_t *t_ns, const double *q_SI, const double *p_SI, double *pose7) {
  CHK_S;
  if (!q_SI || !p_SI || (n && !pose7)) return ctv::fail(CTVIO_ERR_INVALID, "ctvio_sensor_pose: null argument");
  return s->impl.spline_eval(id, n, t_ns, pose7, nullptr, nullptr, nullptr, q_SI, p_SI);
}
// ---- multi-device host entry: w mod G, one host thread + solver handle per device
int32_t ctvio_shard_of(int32_t window_id, int32_t n_devices) { return n_devices > 0 ? window_id % n_devices : 0; }
int32_t ctvio_shard_count(int32_t n, int32_t device, int32_t n_devices) {
  if (n_devices <= 0 || device < 0 || device >= n_devices || n <= 0) return 0;
  return n / n_devices + (device < n % n_devices ? 1 : 0);
}
namespace {
// (memcmp over the struct would compare its tail padding: indeterminate bytes of a caller's stack object)
bool same_options(const ctvio_options &a, const ctvio_options &b) {
  return a.device == b.device && a.precision == b.precision && a.use_mfma == b.use_mfma && a.check_every == b.check_every &&
         a.function_tolerance == b.function_tolerance && a.gradient_tolerance == b.gradient_tolerance && a.parameter_tolerance == b.parameter_tolerance &&
         a.initial_radius == b.initial_radius && a.max_radius == b.max_radius && a.min_radius == b.min_radius &&
         a.min_relative_decrease == b.min_relative_decrease && a.min_lm_diagonal == b.min_lm_diagonal && a.max_lm_diagonal == b.max_lm_diagonal &&
         a.max_consecutive_invalid_steps == b.max_consecutive_invalid_steps && a.deterministic == b.deterministic && a.host_threads == b.host_threads &&
         a.use_graph == b.use_graph && a.line_search == b.line_search;
}
std::mutex g_shard_mu;
std::vector<ctvio_solver *> g_shard_solvers;   // one per shard, created on first use (and again when the options change)
std::vector<ctvio_options> g_shard_opts;       // the options each handle was created with
// One persistent host thread per shard (shard 0 runs on the caller's thread): a call posts its per-shard job and waits -- no thread is
// created or joined per call.  The threads live until ctvio_sharded_release.
struct ShardWorker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<void()> job;
  bool has_job = false, done = true, quit = false;
  ~ShardWorker() { stop(); }   // (a process that never calls ctvio_sharded_release: the idle thread is told to quit and joined at exit)
  void loop() {
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return has_job || quit; });
        if (quit) return;
        f = std::move(job);
        has_job = false;
      }
      f();
      { std::lock_guard<std::mutex> lk(mu); done = true; }
      cv.notify_all();
    }
  }
  void post(std::function<void()> f) {
    { std::lock_guard<std::mutex> lk(mu); job = std::move(f); has_job = true; done = false; }
    cv.notify_all();
  }
  void wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return done; }); }
  void stop() {
    { std::lock_guard<std::mutex> lk(mu); quit = true; }
    cv.notify_all();
    if (th.joinable()) th.join();
  }
};
std::vector<std::unique_ptr<ShardWorker>> g_shard_workers;   // [g - 1] for shard g >= 1
}
// The number of shards ctvio_solve_sharded uses: min(requested or all devices, devices present, windows).  With the TEST-ONLY
// environment switch CTVIO_SHARD_OVERSUBSCRIBE=1 the device count does not clamp it (shard g runs on device g mod #devices), so that
// the multi-shard path can be exercised on a box with one GPU.
int32_t ctvio_shards_used(int32_t n_devices, int32_t n) {
  const int ndev = ctvio_device_count();
  if (ndev <= 0 || n <= 0) return 0;
  if (ctv::read_debug_switches().shard_oversubscribe && n_devices > 0) return std::min(n_devices, n);
  return std::min(n_devices > 0 ? std::min(n_devices, ndev) : ndev, n);
}
void ctvio_sharded_release(void) {
  std::lock_guard<std::mutex> lk(g_shard_mu);
  for (auto &wk : g_shard_workers) wk->stop();
  g_shard_workers.clear();
  for (auto *sv : g_shard_solvers) if (sv) ctvio_destroy(sv);
  g_shard_solvers.clear();
  g_shard_opts.clear();
}
int32_t ctvio_solve_sharded(const ctvio_options *opt, int32_t n_devices, int32_t n, const ctvio_window *wins, int32_t max_iterations,
                            ctvio_summary *out, double *quat, double *pos, double *bias, double *rho, double *ld) {
  if (n <= 0 || !wins) return ctv::fail(CTVIO_ERR_INVALID, "empty batch");
  const int ndev = ctvio_device_count();
  if (ndev <= 0) return ctv::fail(CTVIO_ERR_NO_DEVICE, "hipGetDeviceCount found no device");
  const int G = ctvio_shards_used(n_devices, n);
  std::lock_guard<std::mutex> lk(g_shard_mu);   // one sharded solve at a time per process (the handles are shared)
  if ((int)g_shard_solvers.size() < G) { g_shard_solvers.resize((size_t)G, nullptr); g_shard_opts.resize((size_t)G); }
  // offsets of every window in the caller's concatenated state arrays
  std::vector<size_t> k0((size_t)n + 1, 0), f0((size_t)n + 1, 0), l0((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) { k0[i + 1] = k0[i] + (size_t)std::max(wins[i].K, 0); f0[i + 1] = f0[i] + (size_t)std::max(wins[i].F, 0); l0[i + 1] = l0[i] + (size_t)std::max(wins[i].L, 0); }
  std::vector<int> rcs((size_t)G, CTVIO_OK);
  std::vector<std::string> errs((size_t)G);
  auto work_body = [&](int g) {
    auto failed = [&](int rc) { rcs[g] = rc; errs[g] = "shard " + std::to_string(g) + ": " + ctvio_last_error(); };   // (thread-local error text)
    ctvio_options o;
    if (opt) o = *opt; else ctvio_default_options(&o);
    o.device = g % ndev;
    if (g_shard_solvers[g] && !same_options(o, g_shard_opts[g])) {   // the caller changed the options: a fresh handle
      ctvio_destroy(g_shard_solvers[g]);
      g_shard_solvers[g] = nullptr;
    }
    if (!g_shard_solvers[g]) {
      if (const int rc = ctvio_create(&o, &g_shard_solvers[g])) return failed(rc);
      g_shard_opts[g] = o;
    }
    ctvio_solver *sv = g_shard_solvers[g];
    std::vector<ctvio_window> mine;
    std::vector<int> ids;
    for (int i = g; i < n; i += G) { mine.push_back(wins[i]); ids.push_back(i); }
    const int nm = (int)mine.size();
    if (const int rc = ctvio_set_batch(sv, nm, mine.data())) return failed(rc);
    std::vector<ctvio_summary> sm((size_t)nm);
    if (const int rc = ctvio_solve(sv, max_iterations, sm.data())) return failed(rc);
    size_t K = 0, F = 0, L = 0;
    for (const auto &w : mine) { K += w.K; F += w.F; L += w.L; }
    std::vector<double> q(4 * K), p(3 * K), b(6 * F), r(std::max<size_t>(L, 1)), l((size_t)nm);
    if (const int rc = ctvio_get_batch_state(sv, q.data(), p.data(), b.data(), r.data(), l.data())) return failed(rc);
    size_t ka = 0, fa = 0, la = 0;
    for (int j = 0; j < nm; ++j) {
      const int i = ids[j];
      const ctvio_window &w = mine[j];
      if (out) out[i] = sm[j];
      if (quat) std::memcpy(quat + 4 * k0[i], q.data() + 4 * ka, sizeof(double) * 4 * w.K);
      if (pos) std::memcpy(pos + 3 * k0[i], p.data() + 3 * ka, sizeof(double) * 3 * w.K);
      if (bias) std::memcpy(bias + 6 * f0[i], b.data() + 6 * fa, sizeof(double) * 6 * w.F);
      if (rho && w.L) std::memcpy(rho + l0[i], r.data() + la, sizeof(double) * w.L);
      if (ld) ld[i] = l[j];
      ka += w.K; fa += w.F; la += w.L;
    }
  };
  auto work = [&](int g) {   // (an exception escaping a std::thread would terminate the process)
    try { work_body(g); }
    catch (const std::exception &e) { rcs[g] = CTVIO_ERR_HIP; errs[g] = "shard " + std::to_string(g) + ": " + e.what(); }
    catch (...) { rcs[g] = CTVIO_ERR_HIP; errs[g] = "shard " + std::to_string(g) + ": unknown exception"; }
  };
  while ((int)g_shard_workers.size() < G - 1) {
    g_shard_workers.emplace_back(new ShardWorker());
    ShardWorker *wk = g_shard_workers.back().get();
    wk->th = std::thread([wk] { wk->loop(); });
  }
  // (jobs hold references to this frame: whatever was posted is waited for before the function unwinds, also when a later post throws)
  int posted = 0;
  try {
    for (int g = 1; g < G; ++g) { g_shard_workers[g - 1]->post([&work, g] { work(g); }); posted = g; }
    work(0);
  } catch (...) {
    for (int g = 1; g <= posted; ++g) g_shard_workers[g - 1]->wait();
    return ctv::fail(CTVIO_ERR_HIP, "ctvio_solve_sharded: could not hand a shard to its worker thread");
  }
  for (int g = 1; g < G; ++g) g_shard_workers[g - 1]->wait();
  for (int g = 0; g < G; ++g) if (rcs[g] != CTVIO_OK) return ctv::fail(rcs[g], errs[g]);
  return CTVIO_OK;
}

int32_t ctvio_last_timing(ctvio_solver *s, double *ms8, int32_t *launches8) { CHK_S; return s->impl.last_timing(ms8, launches8); }
int32_t ctvio_snapshot_state(ctvio_solver *s) { CHK_S; return s->impl.snapshot(0); }
int32_t ctvio_restore_state(ctvio_solver *s) { CHK_S; return s->impl.snapshot(1); }
int32_t ctvio_set_profiling(ctvio_solver *s, int32_t on) { CHK_S; return s->impl.set_profiling(on); }
void *ctvio_stream(ctvio_solver *s) { return s ? s->impl.stream() : nullptr; }
int32_t ctvio_graph_captures(const ctvio_solver *s) { return s ? s->impl.graph_captures() : 0; }
int32_t ctvio_marginalize_ran_on_host(const ctvio_solver *s) { return s ? s->impl.marg_ran_on_host() : 0; }

}  // extern "C"
