// kernels_imu.hpp -- IMU linearisation: k_imu_linearize_f64 (the product path's walk over groups, fast body), the general body / k_imu_linearize_rest,
// assemble_imu_window (the bias rows of the group tiles: run by k_misc).
// Part of kernels.hpp (included from there, in order; not a stand-alone header).
#pragma once

namespace ctv {

// ------------------------------------------------------------------------------------------------ IMU
template <class T, int N> struct alignas(N * sizeof(T)) VecN { T v[N]; };

typedef double f64x4 __attribute__((ext_vector_type(4)));

// The zeroing of the normal equations' accumulated parts, done by the IMU groups of the window instead of a pass of its own (k_zero_normal
// is HBM-bound, ~100 us per 2048 windows; the stores cost this compute-bound kernel nothing): group gi of the window clears its
// share of Hpp -- only the bias rows and the line-delay row when the single visual-assembly part overwrites the knot x knot block with plain
// stores (zero_mode 1), everything otherwise (zero_mode 2) -- and the first group the gradient and the max-norm cell.  Every accumulating
// kernel (k_assemble_vis*, k_assemble_imu, k_misc) is launched after the linearisation kernels.  zero_mode 0: k_zero_normal did it.
__device__ __forceinline__ void imu_zero_share(const Dev &d, int mode, const ImuGroup &grp, int gidx, int zero_mode) {
  if (!zero_mode) return;
  const int w = grp.win, lane = threadIdx.x;
  const WinMeta &m = d.wins[w];
  const int tg = lin_target(d.lm[w], mode);
  double *Hpp = d.HppS[tg] + m.H0, *g = d.gS[tg] + m.u0;
  const int nH = m.P * m.ldh, first = (m.vis_lds && zero_mode == 1) ? 6 * m.K * m.ldh : 0;   // (ldh is a multiple of 16: both even)
  const int gi = gidx - m.grp0, per = (((nH - first) / 2 + m.ngrp - 1) / m.ngrp) * 2;
  const int lo = first + gi * per, hi = min(lo + per, nH);
  for (int i = lo + 2 * lane; i < hi; i += 128) *reinterpret_cast<double2 *>(Hpp + i) = double2{0.0, 0.0};
  if (gi == 0) {
    for (int i = lane; i < m.P; i += 64) g[i] = 0.0;
    if (lane == 0) { if (mode == LIN_SPEC) d.lm[w].cand_gmax_bits = 0ull; else d.lm[w].gmax_bits = 0ull; }
  }
}

// All-fp64 product path: one wave per IMU group, 64 samples per pass (one per lane), A^T A on the fp64 matrix cores.
// The 6 x 30 Jacobian of a sample stays in REGISTERS in factored form (ImuJac); its six rows are streamed through LDS one
// row index at a time -- phase a: row a of all 64 samples ([64][33] doubles = 16.9 KB, so 8 waves fit a CU and every lane
// evaluates a sample), then 16 K-steps of v_mfma_f64_16x16x4_f64 per output tile.  Accelerometer rows feed the three lower
// 16 x 16 tiles of the 32-column space, gyro rows (non-zero in rotation, gyro-bias and residual columns only) one 16 x 16
// tile on compacted columns.  MFMA operand layout (measured, tools/mfma_f64_layout.hip): A lane l = X[k = l/16][i = l%16],
// B lane l = Y[k = l/16][j = l%16], D register r of lane l = D[(l/16) + 4r][l%16].
__device__ __forceinline__ void imu_linearize_f64_body(const Dev &d, int mode, double *A /* LDS [64][33] */, int gidx, int zero_mode) {
  const ImuGroup grp = d.groups[gidx];
  const int w = grp.win;
  if (!lin_run(d.lm[w], mode)) return;
  const bool jac = !lin_cost_only(d.lm[w], mode, d.prm);   // (uniform) the last allowed iteration only costs its candidate
  if (jac) imu_zero_share(d, mode, grp, gidx, zero_mode);
  const WinMeta &m = d.wins[w];
  const int lane = threadIdx.x, q4 = lane >> 4, l15 = lane & 15;
  const bool at_cand = mode == LIN_SPEC;
  double csum = 0.0;
  const double *s_quat = at_cand ? d.cquat : d.quat, *s_pos = at_cand ? d.cpos : d.pos, *s_bias = at_cand ? d.cbias : d.bias;
  Knots4 k;
  LocalFrame lf;
  lf.init(s_quat, s_pos, m.knot0 + grp.s);
  lf.load(s_quat, s_pos, m.knot0 + grp.s, k);
  const M3 RrefT = lf.RrefT();
  SegConstLazy sc;   // Jr^-1 of the three knot pairs: fetched from the table where it is used
  seg_const_lazy(d.lkd + 3 * (m.knot0 + grp.s), d.kjri + 9 * (m.knot0 + grp.s), sc);
  double bias[6], wgt[6];
  const double *bp = s_bias + 6 * (m.bias0 + grp.bias);
#pragma unroll
  for (int i = 0; i < 6; ++i) { bias[i] = bp[i]; wgt[i] = m.imu_w[i]; }
  const V3 grav = lf.rotate(m.gravity);
  const double idt = m.inv_dt;
  f64x4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc10 = {0.0, 0.0, 0.0, 0.0}, acc11 = {0.0, 0.0, 0.0, 0.0}, gacc = {0.0, 0.0, 0.0, 0.0};
  const size_t Mt = (size_t)d.Mtot;
  if (!jac) {   // residuals only (a separate, small code path: the full one below keeps its compile-time `want_jac = true`)
    for (int c0 = 0; c0 < grp.count; c0 += 64) {
      const bool live = c0 + lane < grp.count;
      const int idx = m.imu0 + grp.start + min(c0 + lane, grp.count - 1);
      double gy[3], ac[3], r[6], wl[6];
#pragma unroll
      for (int i = 0; i < 3; ++i) { gy[i] = d.imu_meas[(size_t)i * Mt + idx]; ac[i] = d.imu_meas[(size_t)(3 + i) * Mt + idx]; }
#pragma unroll
      for (int i = 0; i < 6; ++i) wl[i] = live ? wgt[i] : 0.0;
      ImuJac J;
      imu_eval_core(k, sc, d.imu_u[idx], idt, grav, bias, gy, ac, wl, RrefT, r, false, J);
#pragma unroll
      for (int i = 0; i < 6; ++i) csum += 0.5 * r[i] * r[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) csum += __shfl_xor(csum, off);
    if (lane == 0) d.imu_cost[gidx] = csum;
    return;
  }
  for (int c0 = 0; c0 < grp.count; c0 += 64) {
    const int nval = min(64, grp.count - c0);
    const bool live = lane < nval;
    const int idx = m.imu0 + grp.start + min(c0 + lane, grp.count - 1);   // clamped: every lane evaluates (uniform control flow around the MFMAs)
    double gy[3], ac[3], r[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) { gy[i] = d.imu_meas[(size_t)i * Mt + idx]; ac[i] = d.imu_meas[(size_t)(3 + i) * Mt + idx]; }
    // lanes past the end of the group evaluate a clamped sample with ZERO weights: every row of w .* [J | r] is then exactly
    // zero (one select per weight instead of one per stored entry: 288 v_cndmask per pass)
    double wl[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) wl[i] = live ? wgt[i] : 0.0;
    const int kmax = (nval + 3) & ~3;
    ImuJac J;
    imu_eval_core(k, sc, d.imu_u[idx], idt, grav, bias, gy, ac, wl, RrefT, r, true, J);
#pragma unroll
    for (int i = 0; i < 6; ++i) csum += 0.5 * r[i] * r[i];   // (dead lanes: zero weights, zero residual)
    // ---- accelerometer rows: 32 columns, tiles (0,0), (1,0), (1,1)
#pragma unroll
    for (int a = 0; a < 3; ++a) {   // unrolled: the row index must be static (a dynamic index would push ImuJac to scratch)
      double row[32];
      imu_row_accel(J, wl, r, a, row);
      __builtin_amdgcn_wave_barrier();   // the previous phase's operand reads are complete (consumed by its MFMAs)
#pragma unroll
      for (int c = 0; c < 32; ++c) A[lane * 33 + c] = row[c];
      lds_wave_sync();   // the rows are in LDS
      for (int k0 = 0; k0 < kmax; k0 += 4) {
        const double lo = A[(k0 + q4) * 33 + l15], hi = A[(k0 + q4) * 33 + 16 + l15];
        acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(lo, lo, acc00, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(hi, lo, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(hi, hi, acc11, 0, 0, 0);
      }
    }
    // ---- gyro rows: 16 compacted columns, one tile
#pragma unroll
    for (int a = 0; a < 3; ++a) {   // unrolled: the row index must be static (a dynamic index would push ImuJac to scratch)
      double row[16];
      imu_row_gyro(J, wl, r, a, row);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int c = 0; c < 16; ++c) A[lane * 17 + c] = row[c];
      lds_wave_sync();
      for (int k0 = 0; k0 < kmax; k0 += 4) {
        const double v = A[(k0 + q4) * 17 + l15];
        gacc = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, gacc, 0, 0, 0);
      }
    }
  }
  // ---- the group's share of the cost: fixed-order sum over the lanes (butterfly), one store
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) csum += __shfl_xor(csum, off);
  if (lane == 0) d.imu_cost[gidx] = csum;
  // ---- combine in LDS into the full symmetric 32 x 32 tile, then one coalesced store
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = q4 + 4 * r, col = l15;
    A[row * 32 + col] = acc00[r];
    A[(16 + row) * 32 + 16 + col] = acc11[r];
    A[(16 + row) * 32 + col] = acc10[r];
    A[col * 32 + 16 + row] = acc10[r];     // mirror of the off-diagonal tile
  }
  lds_wave_sync();
  {
    const int tc = l15 < 12 ? l15 : (l15 < 15 ? l15 + 12 : 30);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int grow = q4 + 4 * r;
      const int tr = grow < 12 ? grow : (grow < 15 ? grow + 12 : 30);
      A[tr * 32 + tc] += gacc[r];
    }
  }
  lds_wave_sync();
  double *tile = d.imu_tiles + (size_t)gidx * 1024;
#pragma unroll
  for (int i = 0; i < 16; ++i) tile[i * 64 + lane] = A[i * 64 + lane];
}

// The MFMA chains of one row phase, two K-steps per trip: the operands of step k + 1 are requested before the MFMAs of step k are issued
// (clock stamps of one group, 3 gyro + 3 accelerometer row phases of a full pass: 6980 + 11372 cycles with the read of step k issued right
// before its MFMA, 6364 + 10384 like this; three steps ahead -- four steps per trip, K rounded to 16 rows -- 6332 + 10828 and the partial
// passes lose to the rounding: not kept; a second gyro accumulator changes nothing either: the chain is not waiting for its own results).
// K is rounded up to a multiple of 8 rows: the rows past the last sample are zero rows (dead lanes write zeros), the buffer has 8 spare rows
// for the last prefetch.
// (The operand fetches and their waits are inline assembly: left to itself the compiler re-loads the carried operand at the top of the
//  next trip -- one ds_read2, one wait, two MFMAs, the very serialisation this removes; volatile loads become flat loads with a full wait
//  each.  The waits carry the operand as an in/out so that the MFMA that consumes it stays behind them; a final lgkmcnt(0) leaves nothing
//  in flight that the compiler's own wait counting does not know about.)
__device__ __forceinline__ void imu_chain_gyro(const double *A, int q4, int l15, int kmax, f64x4 &gacc) {
  unsigned addr = (unsigned)(size_t)(A + q4 * 17 + l15);
  double v0, v1;
  asm volatile("ds_read_b64 %0, %1" : "=v"(v0) : "v"(addr));
  for (int k0 = 0; k0 < kmax; k0 += 8) {
    asm volatile("ds_read_b64 %0, %1 offset:544" : "=v"(v1) : "v"(addr));          // step k0 + 4 (4 rows of 17 doubles on)
    asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(v0));
    gacc = __builtin_amdgcn_mfma_f64_16x16x4f64(v0, v0, gacc, 0, 0, 0);
    addr += 8 * 17 * 8;
    asm volatile("ds_read_b64 %0, %1" : "=v"(v0) : "v"(addr));                     // step k0 + 8
    asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(v1));
    gacc = __builtin_amdgcn_mfma_f64_16x16x4f64(v1, v1, gacc, 0, 0, 0);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v0));
}
// World-frame accelerometer row b of the pass (A: [72][17], as the gyro's) with the position weights L[72][4] = w lamA_k of every sample:
// acc00 += Y_b^T Y_b as above, and x += sum_s w lamA_k(s) Y_s[b][c] -- an M = 4 product, one v_mfma_f64_4x4x4_4b_f64 per K-step (layout,
// tools/mfma4_layout.hip: A lane = i + 4 block + 16 k, B lane = j + 4 block + 16 k, D lane = j + 4 block + 16 i): its A operand is
// L[sample 4 t + lane / 16][lane & 3], its B operand the very register the 16x16x4 reads, and lane l of x ends up with knot l / 16, column l & 15.
__device__ __forceinline__ void imu_chain_world(const double *A, const double *L, int q4, int l15, int kmax, f64x4 &acc00, double &x) {
  unsigned addr = (unsigned)(size_t)(A + q4 * 17 + l15), laddr = (unsigned)(size_t)(L + q4 * 4 + (l15 & 3));
  double v0, v1, a0, a1;
  asm volatile("ds_read_b64 %0, %1" : "=v"(v0) : "v"(addr));
  asm volatile("ds_read_b64 %0, %1" : "=v"(a0) : "v"(laddr));
  for (int k0 = 0; k0 < kmax; k0 += 8) {
    asm volatile("ds_read_b64 %0, %1 offset:544" : "=v"(v1) : "v"(addr));          // step k0 + 4
    asm volatile("ds_read_b64 %0, %1 offset:128" : "=v"(a1) : "v"(laddr));
    asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(v0), "+v"(a0));
    acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(v0, v0, acc00, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f64_4x4x4f64(a0, v0, x, 0, 0, 0);
    addr += 8 * 17 * 8;
    laddr += 8 * 4 * 8;
    asm volatile("ds_read_b64 %0, %1" : "=v"(v0) : "v"(addr));                     // step k0 + 8
    asm volatile("ds_read_b64 %0, %1" : "=v"(a0) : "v"(laddr));
    asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(v1), "+v"(a1));
    acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(v1, v1, acc00, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f64_4x4x4f64(a1, v1, x, 0, 0, 0);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v0), "+v"(a0));
}

// The fast body's groups: every knot-pair log below 0.5 rad, isotropic accelerometer weights.  Asked in two places (the fast body about its
// own group, k_imu_linearize_rest about every group of its window) that must agree to the bit: the operations are spelled out (no
// contraction choices left to the compiler).
__device__ __forceinline__ bool imu_fast_pred(const double kd[9], const double *imu_w) {
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) mx = fmax(mx, __fma_rn(kd[3 * i + 2], kd[3 * i + 2], __fma_rn(kd[3 * i + 1], kd[3 * i + 1], __dmul_rn(kd[3 * i], kd[3 * i]))));
  return mx < 0.25 && imu_w[3] == imu_w[4] && imu_w[3] == imu_w[5];
}
// ---- The product path's body for the usual group (imu_group_fast: knot-pair logs below 0.5 rad, isotropic accelerometer weights).
// Same wave-per-group scheme and row streaming as the general body above, with
//   * the evaluation in stages (factors.hpp, staged form): values, gyro rows -> three row phases, accelerometer rows -> three row
//     phases, so the two sensors' 3 x 12 blocks are never live together; small-angle series, no branch in the loop;
//   * global frame (the local frame of the general body is an fp32 device), the pair logs in SGPRs;
//   * PAIR-LOG COORDINATES (factors.hpp): a sample's rows are streamed as w [D0 | M_0 M_1 M_2 | bias | r] -- the derivatives with respect
//     to the three pair logs, 16 compact columns for either sensor -- and Jr^-1 of the knot pairs, a constant of the group, is applied ONCE
//     per group in the combine stage: tile = T^T G^ T, five 16 x 16 x 16 products on the matrix cores with the accumulators as operands
//     (20 MFMAs per ~100 samples instead of six M Jr^-1 products, ~380 fp64 instructions, per sample);
//   * the accelerometer rows ROTATED INTO THE WORLD FRAME (isotropic weights: the Gram matrix does not change): the position columns
//     w lamA_k R(t)^T become w lamA_k I3, so T1^T T0 is the lamA-weighted sum of the rows -- an M = 4 product, one v_mfma_f64_4x4x4 (16
//     cycles) per K-step in place of a 16x16x4 (64 cycles), and the rows are 16 columns wide instead of 28;
//     T1^T T1 = w^2 sum_s lamA_k lamA_k' I3 from ten per-lane sums as before;
//   * the next pass's measurements requested before the current pass is evaluated.
// (fp64 MFMA and fp64 VALU instructions share one datapath on gfx950 -- tools/mfma_valu_overlap.hip: one wave's MFMAs and FMAs add up,
//  two waves on a SIMD do not overlap them either -- so the kernel's time is the SUM of its vector and matrix work: both are cut here.)
// A wave WALKS its groups g0, g0 + stride, ... (k_imu_linearize_f64: 2048 waves for the whole batch) and everything the NEXT group's
// record locates -- pair logs and Jr^-1, first knot's rotation, knot positions, bias, gravity, weights, 1 / dt, the window's LM flags, one
// element per lane -- is requested while the CURRENT group is evaluated, and the record after that is on its way as well; the next group's
// first 64 samples are requested by the current group's last pass.  A group's own prologue (three dependent round trips group -> window ->
// data at one wave per SIMD: ~10 k of a group's 55 k cycles, measured) shrinks to a few dozen v_readlane.
struct ImuPre { double pc, kq; int fl; };
__device__ __forceinline__ void imu_prefetch(const Dev &d, int mode, const ImuGroup &g, int lane, ImuPre &o) {
  const bool at_cand = mode == LIN_SPEC;
  const double *s_quat = at_cand ? d.cquat : d.quat, *s_pos = at_cand ? d.cpos : d.pos, *s_bias = at_cand ? d.cbias : d.bias;
  const WinMeta &m = d.wins[g.win];
  const Lm &lm = d.lm[g.win];
  const double *kd = d.lkd + 3 * g.kabs, *kj = d.kjri + 9 * g.kabs;
  const double *q = s_quat + 4 * g.kabs, *pp = s_pos + 3 * g.kabs, *bp = s_bias + 6 * g.babs;
  // pc: lanes 0..8 the pair logs, 9..35 Jr^-1 (row major per pair)
  o.pc = *(lane < 9 ? kd + lane : kj + (min(lane, 35) - 9));
  // kq: 0..3 q_0 | 4..15 the four knot positions | 21..23 gravity | 24..29 bias | 30..35 weights | 36 1 / dt   (unconditional loads on valid addresses)
  const double *src = lane < 4 ? q + lane : lane < 16 ? pp + (lane - 4) : lane < 21 ? q : lane < 24 ? m.gravity + (lane - 21)
                      : lane < 30 ? bp + (lane - 24) : lane < 36 ? m.imu_w + (lane - 30) : &m.inv_dt;
  o.kq = *src;
  // fl: lanes 0..3 the window's LM flags (not written by any linearisation kernel)
  const int32_t *fp = lane == 0 ? &lm.status : lane == 1 ? &lm.step_valid : lane == 2 ? &lm.iter : &lm.ls_active;
  o.fl = *fp;
}
__device__ __forceinline__ void imu_linearize_f64_fast(const Dev &d, int mode, double *A /* LDS [72][33] + 64 */, int g0, int stride, int zero_mode) {
  const int lane = threadIdx.x, q4 = lane >> 4, l15 = lane & 15;
  const size_t Mt = (size_t)d.Mtot;
  int gidx = g0;
  ImuGroup grp = d.groups[gidx];
  ImuPre cur;
  imu_prefetch(d, mode, grp, lane, cur);                 // (the walk's first group: its round trips are exposed once)
  double gyn[3], acn[3], un;   // the next pass's measurements, in flight while the current pass is evaluated
  {
    const int idx = grp.iabs + min(lane, grp.count - 1);
#pragma unroll
    for (int i = 0; i < 3; ++i) { gyn[i] = d.imu_meas[(size_t)i * Mt + idx]; acn[i] = d.imu_meas[(size_t)(3 + i) * Mt + idx]; }
    un = d.imu_u[idx];
  }
  bool has_next = gidx + stride < d.Gtot;
  ImuGroup grpn = d.groups[has_next ? gidx + stride : gidx];
  for (;;) {
  // ---- the group after the next one's record and the next one's constants: on their way during this group
  const bool has_next2 = has_next && gidx + 2 * stride < d.Gtot;
  const ImuGroup grpn2 = d.groups[has_next2 ? gidx + 2 * stride : gidx];
  ImuPre nxt;
  imu_prefetch(d, mode, grpn, lane, nxt);
  bool nmeas = false;          // the next group's first pass has been requested (by this group's last pass)
  do {
  const int w = grp.win;
  const int base = grp.iabs;
  // the group's constants: knot-pair logs (used a dozen times per pass) in scalar registers, the rest (used once or twice per
  // pass) in LDS behind the row buffer -- [0..11] knot positions relative to knot 0, [12..20] R_0^T, [21..23] gravity, [24..29] bias,
  // [30..35] weights.  (All of them in scalar registers overflow the SGPR file: 250 v_readlane per pass to fetch them back.)
  // Jr^-1 of the three pairs stays where the prefetch left it -- lanes 9..35 of cur.pc -- until the combine stage builds T from it.
  SegConstS sc;   // (JrI is not filled: the staged form reads the logs only)
#pragma unroll
  for (int i = 0; i < 3; ++i) sc.d[i] = mk(readlane_d(cur.pc, 3 * i), readlane_d(cur.pc, 3 * i + 1), readlane_d(cur.pc, 3 * i + 2));
  // ---- the window: LM state
  const int f_status = __builtin_amdgcn_readlane(cur.fl, 0), f_valid = __builtin_amdgcn_readlane(cur.fl, 1), f_iter = __builtin_amdgcn_readlane(cur.fl, 2),
            f_ls = __builtin_amdgcn_readlane(cur.fl, 3);
  if (!(f_status == 0 && (mode != LIN_SPEC || f_valid != 0))) break;                                   // lin_run
  const bool jac = !(mode == COST_AT_X || (mode == LIN_SPEC && f_iter >= d.prm.max_iters && f_ls == 0));   // lin_cost_only: (uniform) the last allowed iteration only costs its candidate
  // is this group the fast body's?  (imu_group_fast, decided HERE from the pair logs and the weights already in registers)
  {
    const double kd9[9] = {sc.d[0].x, sc.d[0].y, sc.d[0].z, sc.d[1].x, sc.d[1].y, sc.d[1].z, sc.d[2].x, sc.d[2].y, sc.d[2].z};
    const double w6[6] = {0.0, 0.0, 0.0, readlane_d(cur.kq, 33), readlane_d(cur.kq, 34), readlane_d(cur.kq, 35)};
    if (!imu_fast_pred(kd9, w6)) break;   // (uniform) left to k_imu_linearize_rest
  }
  long long *dbg = (d.dbg && gidx == 5000 && jac) ? d.dbg + 64 : nullptr;   // CTVIO_DEBUG_STAMPS: clock64 of lane 0 at the phase boundaries
  int dbi = 0;
  CTV_STAMP(dbg, dbi, 16, lane == 0);
  double *gc = A + 72 * 33;   // (8 spare rows behind the 64: the chains' last prefetch)
  {
    double gcv = cur.kq;      // lanes 21..35: gravity, bias, weights as requested
    const M3 R0 = q2R(qmk(readlane_d(cur.kq, 0), readlane_d(cur.kq, 1), readlane_d(cur.kq, 2), readlane_d(cur.kq, 3)));
    const double pk = __shfl(cur.kq, 4 + min(lane, 11)), p0 = __shfl(cur.kq, 4 + min(lane, 11) % 3);
    if (lane < 12) gcv = pk - p0;
    else if (lane < 21) {   // R_0^T, row major (a select chain: no dynamically indexed register array)
      const int e = lane - 12, src = 3 * (e % 3) + e / 3;
#pragma unroll
      for (int i = 0; i < 9; ++i) gcv = src == i ? R0.m[i] : gcv;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 36) gc[lane] = gcv;
    lds_wave_sync();
  }
  const double idt = readlane_d(cur.kq, 36);
  double csum = 0.0;
  if (!jac) {   // residuals only
    for (int c0 = 0; c0 < grp.count; c0 += 64) {
      const bool live = c0 + lane < grp.count;
      const int idx = base + min(c0 + lane, grp.count - 1);
      double gy[3], ac[3], r[6], wl[6];
#pragma unroll
      for (int i = 0; i < 3; ++i) { gy[i] = d.imu_meas[(size_t)i * Mt + idx]; ac[i] = d.imu_meas[(size_t)(3 + i) * Mt + idx]; }
#pragma unroll
      for (int i = 0; i < 6; ++i) wl[i] = live ? gc[30 + i] : 0.0;
      ImuMid3 md;
      imu_eval_values3(gc, sc, d.imu_u[idx], idt, gy, ac, wl, r, md);
#pragma unroll
      for (int i = 0; i < 6; ++i) csum += 0.5 * r[i] * r[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) csum += __shfl_xor(csum, off);
    if (lane == 0) d.imu_cost[gidx] = csum;
    break;
  }
  f64x4 acc00 = {0.0, 0.0, 0.0, 0.0}, gacc = {0.0, 0.0, 0.0, 0.0};
  double xpos[3] = {0.0, 0.0, 0.0};   // lane (k, c): sum_s w lamA_k(s) Y_s[b][c], b = 0..2
  double spp[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double *Lw = A + 1280;   // [72][4] behind the [72][17] rows
  for (int c0 = 0; c0 < grp.count; c0 += 64) {
    CTV_STAMP(dbg, dbi, 16, lane == 0, csum);
    const int nval = min(64, grp.count - c0);
    const bool live = lane < nval;
    double gy[3], ac[3], r[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) { gy[i] = gyn[i]; ac[i] = acn[i]; }
    const double u = un;
    {
      // the next pass's samples -- after the group's last pass the NEXT GROUP's first ones (without one, a valid sample that is dropped)
      const bool last = c0 + 64 >= grp.count;
      const int idx = (last && has_next) ? grpn.iabs + min(lane, grpn.count - 1) : base + min(c0 + 64 + lane, grp.count - 1);
      nmeas = last;
#pragma unroll
      for (int i = 0; i < 3; ++i) { gyn[i] = d.imu_meas[(size_t)i * Mt + idx]; acn[i] = d.imu_meas[(size_t)(3 + i) * Mt + idx]; }
      un = d.imu_u[idx];
    }
    // lanes past the end of the group evaluate a clamped sample with ZERO weights: every row of w .* [J | r] is then exactly zero
    double wl[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) wl[i] = live ? gc[30 + i] : 0.0;
    const int kmax = (nval + 3) & ~3;
    ImuMid3 md;
    imu_eval_values3(gc, sc, u, idt, gy, ac, wl, r, md);
#pragma unroll
    for (int i = 0; i < 6; ++i) csum += 0.5 * r[i] * r[i];   // (dead lanes: zero weights, zero residual)
    CTV_STAMP(dbg, dbi, 16, lane == 0, csum);
    {
      M3 Mw[3];
      imu_pair_gyro3(md, Mw);
      CTV_STAMP(dbg, dbi, 16, lane == 0, Mw[2].m[8]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {   // unrolled: the row index must be static
        double row[16];
        imu_row_gyro_pl(Mw, wl, r, a, row);
        __builtin_amdgcn_wave_barrier();   // the previous phase's operand reads are complete (consumed by its MFMAs)
#pragma unroll
        for (int c = 0; c < 16; ++c) A[lane * 17 + c] = row[c];
        lds_wave_sync();   // the rows are in LDS
        imu_chain_gyro(A, q4, l15, kmax, gacc);
      }
    }
    CTV_STAMP(dbg, dbi, 16, lane == 0, gacc[0]);
    {
      double Y[3][16];
      imu_world_accel3(md, gc, wl, r, Y);
      CTV_STAMP(dbg, dbi, 16, lane == 0, Y[2][15]);
      double la[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) la[kk] = wl[3] * md.lamA[kk];
      {
        int e = 0;
#pragma unroll
        for (int ka = 0; ka < 4; ++ka)
#pragma unroll
          for (int kb = 0; kb <= ka; ++kb) { spp[e] += la[ka] * la[kb]; ++e; }
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int c = 0; c < 16; ++c) A[lane * 17 + c] = Y[a][c];
        if (a == 0) {   // the position weights of the pass: the same for its three row phases
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) Lw[lane * 4 + kk] = la[kk];
        }
        lds_wave_sync();
        imu_chain_world(A, Lw, q4, l15, kmax, acc00, xpos[a]);
      }
    }
  }
  CTV_STAMP(dbg, dbi, 16, lane == 0, acc00[0] + xpos[0]);
  // ---- combine in LDS into the full symmetric 32 x 32 tile in the local column order [rot 12 | pos 12 | bg 3 | ba 3 | r | -]
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 16; ++i) A[i * 64 + lane] = 0.0;
  double *S = A + 1024, *Tp = A + 1792, *Xs = A + 2048;   // the sums below [11][64] + 11 | T [16][16] | the position sums [12][17]
#pragma unroll
  for (int i = 0; i < 4; ++i) Tp[i * 64 + lane] = 0.0;
#pragma unroll
  for (int b = 0; b < 3; ++b) Xs[(3 * q4 + b) * 17 + l15] = xpos[b];
  {
    // eleven sums over the 64 lanes in a fixed order -- the ten of the pos x pos block and the group's share of the cost -- through the
    // free half of the buffer: lane (e, part) adds 16 lanes' values, two butterfly steps join the four parts (one LDS round trip for all
    // of them instead of a six-step butterfly per value)
#pragma unroll
    for (int e = 0; e < 10; ++e) S[e * 64 + lane] = spp[e];
    S[10 * 64 + lane] = csum;
    lds_wave_sync();
    const int e = min(lane >> 2, 10), part = lane & 3;
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += S[e * 64 + part * 16 + i];
    t += __shfl_xor(t, 1);
    t += __shfl_xor(t, 2);
    __builtin_amdgcn_wave_barrier();
    if (lane < 40 && part == 0) S[704 + e] = t;
    if (lane == 40) d.imu_cost[gidx] = t;
    // the group's transform T (factors.hpp, pair-log coordinates): lanes 9..35 still hold Jr^-1 of the three pairs, one entry each
    if (lane >= 9 && lane < 36) {
      const int i = (lane - 9) / 9, ab = (lane - 9) % 9;
      int plus, minus;
      imu_pairlog_slots(i, ab / 3, ab % 3, plus, minus);
      Tp[plus] = cur.pc;
      Tp[minus] = -cur.pc;
    }
    if (lane < 3 || (lane >= 12 && lane < 16)) Tp[17 * lane] = 1.0;
  }
  lds_wave_sync();
  {
    // T^T G^ T for the gyro and the accelerometer Gram matrices and (position sums) T, on the matrix cores with the accumulators as they
    // are: K-step r pairs accumulator register r (row q4 + 4 r of G^, symmetric) with the same row of T -- no trip through LDS for G^.
    double Tr[4], Xa[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Tr[r] = Tp[(q4 + 4 * r) * 16 + l15];
      Xa[r] = Xs[min(l15, 11) * 17 + q4 + 4 * r];
      Xa[r] = l15 < 12 ? Xa[r] : 0.0;
    }
    f64x4 zg = {0.0, 0.0, 0.0, 0.0}, za = {0.0, 0.0, 0.0, 0.0}, hg = {0.0, 0.0, 0.0, 0.0}, ha = {0.0, 0.0, 0.0, 0.0}, hx = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      zg = __builtin_amdgcn_mfma_f64_16x16x4f64(gacc[r], Tr[r], zg, 0, 0, 0);
      za = __builtin_amdgcn_mfma_f64_16x16x4f64(acc00[r], Tr[r], za, 0, 0, 0);
      hx = __builtin_amdgcn_mfma_f64_16x16x4f64(Xa[r], Tr[r], hx, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      hg = __builtin_amdgcn_mfma_f64_16x16x4f64(Tr[r], zg[r], hg, 0, 0, 0);
      ha = __builtin_amdgcn_mfma_f64_16x16x4f64(Tr[r], za[r], ha, 0, 0, 0);
    }
    // T0 (accelerometer rows: rot 12 | ba 3 | r) and the gyro tile (rot 12 | bg 3 | r) share the accumulator layout: where neither index
    // is a bias one the two land on the same entry and are added in registers; a bias index sends them to the ba / bg columns.
    // (T^T (G^ T) is symmetric up to rounding only: the lower triangle is stored on both sides, so the tile stays symmetric to the bit.)
    const int c0 = l15 < 12 ? l15 : (l15 < 15 ? l15 + 15 : 30);   // T0 index -> local column (ba at 27..29)
    const int cg = l15 < 12 ? l15 : (l15 < 15 ? l15 + 12 : 30);   // gyro tile index -> local column (bg at 24..26)
    const bool cb = l15 >= 12 && l15 < 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = q4 + 4 * r;
      const int r0 = t < 12 ? t : (t < 15 ? t + 15 : 30), rg = t < 12 ? t : (t < 15 ? t + 12 : 30);
      const bool shared = !cb && !(t >= 12 && t < 15);
      if (t >= l15) {
        const double v = shared ? ha[r] + hg[r] : ha[r];
        A[r0 * 32 + c0] = v;
        A[c0 * 32 + r0] = v;
        if (!shared) { A[rg * 32 + cg] = hg[r]; A[cg * 32 + rg] = hg[r]; }
      }
      if (t < 12) { A[(12 + t) * 32 + c0] = hx[r]; A[c0 * 32 + 12 + t] = hx[r]; }
    }
    // lane (ka, kb, b) < 48 places one entry of the pos x pos block
    const int ka = lane / 12, kb = (lane / 3) & 3, b = lane % 3;
    const int hi = max(ka, kb), lo = min(ka, kb);
    if (lane < 48) A[(12 + 3 * ka + b) * 32 + 12 + 3 * kb + b] = S[704 + hi * (hi + 1) / 2 + lo];
  }
  lds_wave_sync();
  double *tile = d.imu_tiles + (size_t)gidx * 1024;
#pragma unroll
  for (int i = 0; i < 8; ++i)   // 16 bytes per lane: 8 stores of 1 KiB (under load a store costs ~100 cycles whatever its width)
    *reinterpret_cast<double2 *>(tile + i * 128 + 2 * lane) = *reinterpret_cast<const double2 *>(A + i * 128 + 2 * lane);
  // (last: the memory counter is in-order, a load issued after these stores would wait for their acknowledgement)
  imu_zero_share(d, mode, grp, gidx, zero_mode);
  CTV_STAMP(dbg, dbi, 16, lane == 0);
  } while (false);
  // ---- on to the wave's next group
  if (!has_next) break;
  lds_wave_sync();   // (the tile copy-out has read the LDS buffer before the next group writes its constants)
  if (!nmeas) {                             // this group left early: the next one's first pass has not been asked for yet
    const int idx = grpn.iabs + min(lane, grpn.count - 1);
#pragma unroll
    for (int i = 0; i < 3; ++i) { gyn[i] = d.imu_meas[(size_t)i * Mt + idx]; acn[i] = d.imu_meas[(size_t)(3 + i) * Mt + idx]; }
    un = d.imu_u[idx];
  }
  gidx += stride;
  grp = grpn; grpn = grpn2; cur = nxt;
  has_next = has_next2;
  }
}

// One wave per SIMD: the evaluation needs ~430 fp64-pair registers; with a 512-register budget the overflow lives in AGPRs.
// (Two waves per SIMD with the overflow spilled to scratch was measured 3x slower: 1690 vs 540 us per 1024 windows.)
// The fast body evaluates the small-angle series only: a group whose knot-pair logs reach 0.5 rad (28.6 degrees between two knots 50 ms
// apart) takes the general body.  It also takes the pos x pos block from R(t)^T W^2 R(t) = w^2 I: isotropic accelerometer weights (the
// reference's: one scalar per sensor) -- any other weighting takes the general body as well.
__device__ __forceinline__ bool imu_group_fast(const Dev &d, int gidx) {
  const ImuGroup grp = d.groups[gidx];
  const double *kd = d.lkd + 3 * grp.kabs;
  const double kd9[9] = {kd[0], kd[1], kd[2], kd[3], kd[4], kd[5], kd[6], kd[7], kd[8]};
  return imu_fast_pred(kd9, d.wins[grp.win].imu_w);
}
// The groups the fast body leaves out are picked up by k_imu_linearize_rest (one wave per WINDOW: its lanes look at the window's groups,
// the wave then takes the flagged ones in turn -- 12 us per launch when there is nothing to do, which is the rule): the two bodies in
// one kernel cost the fast one registers.
// (general_only: every group through the general body -- ctvio_options.use_mfma = 2, the tests' way into it)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_imu_linearize_f64(Dev d, int mode, int general_only, int zero_mode) {
  extern __shared__ __attribute__((aligned(32))) unsigned char smraw[];
  if (!general_only) imu_linearize_f64_fast(d, mode, reinterpret_cast<double *>(smraw), blockIdx.x, gridDim.x, zero_mode);   // (skips the groups that are not its own)
}
__device__ __forceinline__ void imu_rest_body(const Dev &d, int mode, int general_only, int zero_mode, unsigned char *smraw /* LDS [64][33] doubles */, int w) {
  const WinMeta &m = d.wins[w];
  for (int g0 = 0; g0 < m.ngrp; g0 += 64) {
    const int gl = g0 + (int)threadIdx.x;
    const bool need = gl < m.ngrp && (general_only || !imu_group_fast(d, m.grp0 + gl));
    unsigned long long todo = __ballot(need);
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      imu_linearize_f64_body(d, mode, reinterpret_cast<double *>(smraw), m.grp0 + g0 + b, zero_mode);
      lds_wave_sync();
    }
  }
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_imu_linearize_rest(Dev d, int mode, int general_only, int zero_mode) {
  extern __shared__ __attribute__((aligned(32))) unsigned char smraw[];
  imu_rest_body(d, mode, general_only, zero_mode, smraw, blockIdx.x);
}

// Bias rows (6 x 24 against the knots), bias block (6 x 6 lower triangle) and gradient of a window's group tiles: 195 entries per group -- one
// load, one atomic each.  Lanes follow GLOBAL columns: a bias row's 24 knot columns are the contiguous run 6 s .. 6 s + 23 of its Hpp row (the
// tile's local order is [rot 12 | pos 12]: read through imu_knot_major_to_col), so a wave instruction adds into runs of 192 B instead of runs
// of 24 B, 48 B apart; the knot part of the gradient is one such run of g.  Wave w takes the groups w, w + 4, ...: consecutive groups share
// their bias rows and three of their four knots, and same-address atomics inside one instruction serialise.
__device__ __forceinline__ int imu_knot_major_to_col(int j) {   // j = 6 knot + c  ->  local column ([rot | pos] order)
  const int k = j / 6, c = j - 6 * k;
  return c < 3 ? 3 * k + c : 9 + 3 * k + c;
}
// (Taking four entries per lane at a time -- the group records, then the tile values requested together, then the atomics -- was built and measured:
//  107.4 us against 104.5 us for this loop and 107.1 / 107.6 us for the parent's lane map.)
__device__ __forceinline__ void imu_bias_rows_accumulate(const Dev &d, const WinMeta &m, double *Hpp, double *g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ldh = m.ldh;
  const int nmine = (m.ngrp - wave + 3) >> 2;   // groups wave, wave + 4, ... < ngrp
  for (int i = lane; i < 195 * nmine; i += 64) {
    const int q = i / 195, t = i - 195 * q, gi = m.grp0 + wave + 4 * q;
    const ImuGroup grp = d.groups[gi];
    const double *tile = d.imu_tiles + (size_t)gi * 1024;
    const int B = 6 * grp.s, R = 6 * m.K + 6 * grp.bias;   // first knot column, first bias row
    if (t < 144) {
      const int r = t / 24, j = t - 24 * r;
      atomicAdd(&Hpp[(long long)(R + r) * ldh + B + j], tile[(24 + r) * 32 + imu_knot_major_to_col(j)]);
    } else if (t < 165) {
      const int e = t - 144;                       // lower triangle of the bias block, row-major
      const int r = e < 1 ? 0 : e < 3 ? 1 : e < 6 ? 2 : e < 10 ? 3 : e < 15 ? 4 : 5, c = e - r * (r + 1) / 2;
      atomicAdd(&Hpp[(long long)(R + r) * ldh + R + c], tile[(24 + r) * 32 + 24 + c]);
    } else {
      // (the tile is symmetric: the gradient column is read as row 30, next to the bias rows -- 7 consecutive rows of the tile instead of a
      //  cache line of every row)
      const int j = t - 165;
      atomicAdd(&g[j < 24 ? B + j : R + j - 24], tile[30 * 32 + (j < 24 ? imu_knot_major_to_col(j) : j)]);
    }
  }
}

// Scatter the group tiles into Hpp (lower triangle, fp64) and g.
// One workgroup per WINDOW walking its groups (one per group was 43 k workgroups of 195 useful threads: dispatch-bound).
// (a device function: k_misc runs it in front of the bias chain and the prior -- the two were separate launches of the same shape, one
//  256-thread workgroup per window, each a chain of dependent loads followed by atomics)
__device__ __forceinline__ void assemble_imu_window(const Dev &d, int mode, int w, double *band /* LDS [144 K] or null */) {
  if (!lin_run(d.lm[w], mode) || lin_cost_only(d.lm[w], mode, d.prm)) return;
  const WinMeta &m = d.wins[w];
  const int K = m.K, ldh = m.ldh, tg = lin_target(d.lm[w], mode);
  double *Hpp = d.HppS[tg] + m.H0, *g = d.gS[tg] + m.u0;
  if (m.vis_lds) {
    // the knot x knot part is accumulated in LDS by k_assemble_vis; what is left is the bias rows, the bias block and the gradient
    imu_bias_rows_accumulate(d, m, Hpp, g);
    return;
  }
  // Windows whose packed Hessian does not fit in LDS (K > 24).  The 24 x 24 knot blocks of consecutive segments overlap in three of their four
  // knots (and two groups of one segment coincide): added one by one with global atomics they cost 300 atomics per group -- config 5 (K = 64):
  // 27 k per window, 0.45 ms per 512 windows.  They are summed first in an LDS BAND [K][4 knots][6][6] (a knot couples with itself and the three
  // before it: 74 KB at K = 64) and every band entry goes out once; the bias rows and the gradient (195 per group) stay as they were.
  if (band) {
    const int nb = 144 * K;
    for (int i = threadIdx.x; i < nb; i += 256) band[i] = 0.0;
    __syncthreads();
    for (int i = threadIdx.x; i < 300 * m.ngrp; i += 256) {
      const int gi = i / 300, t = i - 300 * gi;
      int a = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);     // t -> (a >= b), row-major over the lower triangle of 24 x 24
      a += ((a + 1) * (a + 2) / 2 <= t) ? 1 : 0;
      a -= (a * (a + 1) / 2 > t) ? 1 : 0;
      const int b = t - a * (a + 1) / 2;
      const ImuGroup grp = d.groups[m.grp0 + gi];
      const double v = d.imu_tiles[(size_t)(m.grp0 + gi) * 1024 + a * 32 + b];
      int ga = imu_col(a, grp.s, K, grp.bias), gb = imu_col(b, grp.s, K, grp.bias);
      if (ga < gb) { const int tmp = ga; ga = gb; gb = tmp; }            // (local order [rot | pos]: a >= b does not order the unknowns)
      const int k1 = ga / 6, k2 = gb / 6;
      atomicAdd(&band[((k2 * 4 + (k1 - k2)) * 6 + (ga - 6 * k1)) * 6 + (gb - 6 * k2)], v);   // (every unordered local pair once)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256) {
      const double v = band[i];
      if (v == 0.0) continue;
      const int r2 = i % 6, r1 = (i / 6) % 6, dk = (i / 36) % 4, k2 = i / 144;
      const int ga = 6 * (k2 + dk) + r1, gb = 6 * k2 + r2;
      atomicAdd(&Hpp[(long long)ga * ldh + gb], v);
    }
    imu_bias_rows_accumulate(d, m, Hpp, g);                               // bias rows, bias block, gradient: as in the LDS-resident case above
    return;
  }
  for (int i = threadIdx.x; i < 31 * 30 * m.ngrp; i += 256) {
    const int gi = i / 930, e = i - 930 * gi;
    const ImuGroup grp = d.groups[m.grp0 + gi];
    const double *tile = d.imu_tiles + (size_t)(m.grp0 + gi) * 1024;
    const int b = e / 30, a = e % 30;  // a < 30 : unknown row; b <= 30
    const double v = tile[a * 32 + b];
    const int ga = imu_col(a, grp.s, K, grp.bias);
    if (b == 30) { atomicAdd(&g[ga], v); continue; }
    const int gb = imu_col(b, grp.s, K, grp.bias);
    if (ga >= gb) atomicAdd(&Hpp[(long long)ga * ldh + gb], v);
  }
}

}  // namespace ctv
