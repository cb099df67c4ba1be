// kernels_assemble.hpp -- Assembly of the pose block: k_assemble_vis_mfma (fp64 matrix cores, LDS Hessian; STORE = order-fixed tail with k_reduce_finalize /
// k_bias_rows), k_misc (bias chain + prior), k_post_linearize.
// Part of kernels.hpp (included from there, in order; not a stand-alone header).
#pragma once

namespace ctv {

// ---- store-semantics tail of the assembly (product path, windows whose packed Hessian is LDS resident).  Every entry of Hpp / g is
// formed completely by ONE thread and written with a plain store -- the knot x knot block and the line-delay row from the packed
// (LDS or summed-partials) Hessian, the bias rows by a gather over the IMU group tiles of that bias state (fixed order), the bias
// chain and the prior (J0^T J0 looked up through the inverse column map): no pre-zeroing pass, no floating-point atomics, and the
// value does not depend on any execution order.  Entries no factor reaches are zeroed once at upload and never written.
__device__ __forceinline__ double prior_H(const Dev &d, const WinMeta &m, int ga, int gb) {
  if (m.pn <= 0) return 0.0;
  const int pi = d.pinv[m.p0 + ga], pj = d.pinv[m.p0 + gb];
  return (pi >= 0 && pj >= 0) ? d.pH[m.pH0 + (size_t)pi * m.pn + pj] : 0.0;
}
__device__ __forceinline__ double prior_g(const Dev &d, const WinMeta &m, int u) {
  if (m.pn <= 0) return 0.0;
  const int pi = d.pinv[m.p0 + u];
  return pi >= 0 ? d.pgrad[m.pv0 + pi] : 0.0;
}
// packed index i of the knot block / line-delay row -> (row, column) unknowns
__device__ __forceinline__ void packed_decode(int i, int tri, int K6, int P, int &ga, int &gb) {
  if (i < tri) {
    ga = (int)((sqrtf(8.0f * (float)i + 1.0f) - 1.0f) * 0.5f);
    ga += ((ga + 1) * (ga + 2) / 2 <= i) ? 1 : 0;      // the float estimate is off by at most one either way
    ga -= (ga * (ga + 1) / 2 > i) ? 1 : 0;
    gb = i - ga * (ga + 1) / 2;
  } else {
    ga = P - 1;
    gb = (i - tri) < K6 ? (i - tri) : P - 1;
  }
}
// Bias rows (and the bias columns of the line-delay row) of Hpp and the bias entries of g of window w: item e of [0, nitems)
// handled by thread e of a grid-stride loop.  `bias` = the linearisation state (candidate or current).
__device__ __forceinline__ void bias_rows_store(const Dev &d, const WinMeta &m, int tg, const double *bias, int first, int stride) {
  const int K = m.K, F = m.F, P = m.P, K6 = 6 * K, ldh = m.ldh, nbr = 6 * F;
  double *Hg = d.HppS[tg] + m.H0, *g = d.gS[tg] + m.u0;
  const int32_t *boff = d.bgl_off + m.bias0 + (int)(&m - d.wins);   // F + 1 offsets of this window's per-bias group lists
  // items: rows r = K6 .. P - 2 with all columns c <= r (triangle over the bias rows, rectangle over the knot columns), then the
  // line-delay row's bias columns, then the bias entries of g
  const int n_rect = nbr * K6, n_tri = nbr * (nbr + 1) / 2, n_ld = nbr, n_g = nbr;
  for (int e = first; e < n_rect + n_tri + n_ld + n_g; e += stride) {
    if (e < n_rect + n_tri) {
      int rb, c;   // rb: bias row index (0 .. 6F), c: column unknown
      if (e < n_rect) { rb = e / K6; c = e - rb * K6; }
      else {
        const int t = e - n_rect;
        int i2 = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
        i2 += ((i2 + 1) * (i2 + 2) / 2 <= t) ? 1 : 0;
        i2 -= (i2 * (i2 + 1) / 2 > t) ? 1 : 0;
        rb = i2; c = K6 + t - i2 * (i2 + 1) / 2;
      }
      const int f = rb / 6, a = rb - 6 * f, r = K6 + rb;
      double v = 0.0;
      const int g0 = boff[f], g1 = boff[f + 1];
      if (c < K6) {
        const int k = c / 6, cc = c - 6 * k;
        for (int q = g0; q < g1; ++q) {
          const int gi = d.bgl[q];
          const int sg = d.groups[gi].s;
          if (k >= sg && k <= sg + 3) v += d.imu_tiles[(size_t)gi * 1024 + (24 + a) * 32 + (cc < 3 ? 3 * (k - sg) + cc : 12 + 3 * (k - sg) + cc - 3)];
        }
      } else {
        const int cb = c - K6, f2 = cb / 6, a2 = cb - 6 * f2;
        if (f2 == f)
          for (int q = g0; q < g1; ++q) v += d.imu_tiles[(size_t)d.bgl[q] * 1024 + (24 + a) * 32 + 24 + a2];
        if (a2 == a)
          for (int b = 0; b < m.NB; ++b) {
            const int bi = d.bc_i[m.bc0 + b], bj = d.bc_j[m.bc0 + b];
            const double wv = d.bc_w[(size_t)(m.bc0 + b) * 6 + a];
            if (f2 == f) { if (bi == f) v += wv * wv; if (bj == f) v += wv * wv; }
            else if ((bi == f2 && bj == f) || (bi == f && bj == f2)) v -= wv * wv;
          }
      }
      Hg[(long long)r * ldh + c] = v + prior_H(d, m, r, c);
    } else if (e < n_rect + n_tri + n_ld) {
      const int c = K6 + e - n_rect - n_tri;
      Hg[(long long)(P - 1) * ldh + c] = prior_H(d, m, P - 1, c);
    } else {
      const int rb = e - n_rect - n_tri - n_ld, f = rb / 6, a = rb - 6 * f, r = K6 + rb;
      double v = 0.0;
      for (int q = boff[f]; q < boff[f + 1]; ++q) v += d.imu_tiles[(size_t)d.bgl[q] * 1024 + (24 + a) * 32 + 30];
      for (int b = 0; b < m.NB; ++b) {
        const int bi = d.bc_i[m.bc0 + b], bj = d.bc_j[m.bc0 + b];
        if (bi != f && bj != f) continue;
        const double wv = d.bc_w[(size_t)(m.bc0 + b) * 6 + a];
        const double rr = wv * (bias[6 * (m.bias0 + bj) + a] - bias[6 * (m.bias0 + bi) + a]);
        if (bi == f) v -= wv * rr;
        if (bj == f) v += wv * rr;
      }
      g[r] = v + prior_g(d, m, r);
    }
  }
}

// Visual assembly on the fp64 matrix cores: gridDim.y workgroups (parts) per window.  The host sorted the visual blocks by frame pair and cut
// them into items of <= CH = 8 blocks; blocks of an item that evaluate on the same knot quadruples (si, sj) form a run, whose product is added
// into an LDS-resident copy of the window's visual Hessian (packed lower triangle over the 6K knot unknowns + the line-delay row).  The two ends
// of a block may share knots (reference image_feature_factor.h:165-180,215,233): every ordered column pair whose unknowns satisfy g(a) >= g(b)
// is added, so shared knots sum correctly.  Landmark terms (W row, Hll, g_rho) are formed by k_vis_eval.  Windows whose packed Hessian does
// not fit in LDS (vis_lds = 0) add straight into Hpp.
//   * the run's [J~_pose]^T [J~_pose] (48 x 48 = 3 x 3 tiles of 16; the lower 6 tiles) is formed with v_mfma_f64_16x16x4_f64: K = 4 is two
//     blocks x two residual rows, the operands are plain LDS reads of the staged item ([116][CH + 2], row = 2 * column + residual row),
//     the A and B operand of a tile pair are the same registers; the line-delay column and the residual ride along as plain FMAs;
//   * the staging area of a wave is private, so there is no workgroup barrier inside the item loop, and the next item's records (15
//     values per lane) are requested before the current item is processed: their latency hides under the products.
// D register r of lane l = D[(l / 16) + 4 r][l % 16] (tools/mfma_f64_layout.hip); eight fp64 staging areas fit beside the packed Hessian.
// LDS staging of one item: [VIS_SROWS][CH + 1] doubles per wave + 2 CH ints of keys.  The host sizes the dynamic LDS request -- and decides
// whether a window keeps its packed Hessian in LDS -- from these same constants (ctvio.hip: SolverImpl::vis_stage_bytes).
constexpr int VIS_SROWS = 116;
constexpr int vis_stage_stride(int ch) { return ch + 1; }
constexpr size_t vis_stage_bytes(int nw, int ch) { return (size_t)nw * VIS_SROWS * vis_stage_stride(ch) * sizeof(double) + (size_t)nw * 2 * ch * sizeof(int); }
__device__ __forceinline__ f64x4 mfma16(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
// Knot x knot part of an IMU group tile (24 x 24, imu_col order) in the packed Hessian: both ends of an entry lie in the group's knots
// s .. s + 3, so entry e = 24 a + b goes to unknowns (B + oa, B + ob) with B = 6 s and oa, ob constants of e.  Its packed index is
// B (B + 1) / 2 + B (oa + 1) + oa (oa + 1) / 2 + ob: imu_tile_const(e) = (oa + 1) << 16 | oa (oa + 1) / 2 + ob, or -1 for the
// upper triangle (oa < ob).  A lane holds the constants of its nine entries e = lane + 64 q; per group only B changes.
__device__ __forceinline__ int imu_tile_const(int e) {
  const int oa = imu_col(e / 24, 0, 0, 0), ob = imu_col(e % 24, 0, 0, 0);
  return oa >= ob ? ((oa + 1) << 16) | (oa * (oa + 1) / 2 + ob) : -1;
}
__device__ __forceinline__ void imu_tile_add(double *Hs, int s, const int (&tc)[9], const double (&tv)[9]) {
  const int B = 6 * s, tB = B * (B + 1) / 2;
#pragma unroll
  for (int q = 0; q < 9; ++q)
    if (tc[q] >= 0) atomicAdd(&Hs[tB + (int)__umul24((unsigned)B, (unsigned)tc[q] >> 16) + (tc[q] & 0xffff)], tv[q]);
}
// NW = waves per workgroup: 8, or 1 in the deterministic mode (all LDS additions of a partial Hessian then come from one wave, in program
// order).  STORE (LDS-resident windows of the product path): store-semantics tail -- with one part the workgroup finishes the window
// itself (prior added on the way out, bias rows gathered); with several parts every part writes its packed partial Hessian to
// Dev::Hpart and k_reduce_finalize sums them in part order.
template <int CH, bool LDSH, int NW = 8, bool STORE = false> __global__ __launch_bounds__(64 * NW) void k_assemble_vis_mfma(Dev d, int mode) {
  typedef f64x4 acc_t;
  // Row stride of a staged item: CH + 1 = 9 doubles.  The MFMA operand reads are ds_read_b64 of lanes (l15, k-row): row 2 (16 I + l15) + rr, so
  // consecutive l15 are 2 x 9 x 2 = 36 four-byte banks apart -- 16 distinct bank pairs, the rr = 1 half on the odd pairs: conflict-free.  With the
  // stride 10 of rounds 1-4 (40 banks apart: period 8) lanes l15 and l15 + 8 met on one bank and every operand read took twice its cycles.
  constexpr int CHP = vis_stage_stride(CH), RPP = 64 / CH, NT = 64 * NW;
  static_assert(!STORE || LDSH, "the store-semantics tail needs the LDS-resident Hessian");
  // staged rows per item: 0..95 pose columns (row = 2 * column + residual row), 98/99 line delay, 100/101 residual, 102..107 A~,
  // 108..111 cp0, 112..115 cp1.  38 of them come from the block records in HBM (rows 48..71 = the j end's rotation columns, 98..107,
  // 112..115) and 4 from the anchor records (cp0); the anchor end's rotation rows 0..23 are A~ times the anchor's GR (9 record entries
  // per lane, held in registers), the 48 position rows (24..47, 72..95) are rebuilt in LDS from rows 102..115; the inverse-depth
  // column is not needed here.
  static_assert(CH == 8, "the staging pattern is written for items of 8 blocks");
  constexpr int SROWS = VIS_SROWS, NEXP = 48 / RPP;
  const long long t_begin = d.dbg ? clock64() : 0;
  const int w = blockIdx.x, part = blockIdx.y, nparts = gridDim.y;
  if (!lin_run(d.lm[w], mode) || lin_cost_only(d.lm[w], mode, d.prm)) return;
  const WinMeta &m = d.wins[w];
  const int tgset = lin_target(d.lm[w], mode);
  const int P = m.P, K = m.K, nvitem = m.nvitem, vitem0 = m.vitem0, ngrp = m.ngrp, grp0 = m.grp0, u0 = m.u0, ldh = m.ldh;
  if ((m.vis_lds != 0) != LDSH) return;   // the host launches both variants; each window is handled by one of them
  if (!LDSH && m.V == 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smv[];
  // fp64 accumulators: ds_add_f64 sustains ~8 cycles per wave instruction on gfx950, ds_add_f32 ~190 (measured,
  // tools/lds_atomic_bench.hip) -- and the fp64 sums do not depend on the order of the additions to ~1e-16
  double *Hs = reinterpret_cast<double *>(smv);
  const int K6 = 6 * K, tri = K6 * (K6 + 1) / 2;
  const int nHh = LDSH ? tri + K6 + 1 : 0;     // packed Hessian entries: knot x knot lower triangle, line-delay row
  const int nH = nHh + K6 + 1;                 // + gradient of the pose columns (knots, line delay)
  double *gs = Hs + nHh;
  double *stage = reinterpret_cast<double *>(Hs + ((nH + 3) & ~3));     // [NW][SROWS][CHP]
  int *keys = reinterpret_cast<int *>(stage + NW * SROWS * CHP);        // [NW][2][CH]
  // (the wave index read into a scalar register: the item walk -- ranges, descriptors, staging base, loop counters -- is then scalar code)
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int per_round = NW * nparts;
  // IMU group tiles (knot x knot part, 24 x 24 per group, overlapping between consecutive segments): the loads of this wave's
  // first NGI groups are issued before the LDS Hessian is zeroed and added right after -- at the end of the kernel they
  // were three exposed memory round trips (24 k of 243 k cycles, measured)
  constexpr int NGI = 3;
  double tv[NGI][9], tgv[NGI];   // tgv: the group's gradient entries of the knot rows (tile column 30), store-semantics tail only
  int gs_[NGI];
  if (LDSH) {
#pragma unroll
    for (int u = 0; u < NGI; ++u) {
      const int gi = min(part * NW + wave + u * per_round, max(ngrp - 1, 0));
      const ImuGroup grp = d.groups[grp0 + gi];
      gs_[u] = grp.s;
      const double *tile = d.imu_tiles + (size_t)(grp0 + gi) * 1024;
#pragma unroll
      for (int q = 0; q < 9; ++q) { const int e = lane + 64 * q; tv[u][q] = ngrp > 0 ? tile[(e / 24) * 32 + e % 24] : 0.0; }
      tgv[u] = (STORE && ngrp > 0) ? tile[min(lane, 23) * 32 + 30] : 0.0;
    }
  }
  for (int i = 2 * tid; i < ((nH + 3) & ~3); i += 2 * NT) *reinterpret_cast<double2 *>(Hs + i) = double2{0.0, 0.0};
  __syncthreads();
  if (LDSH) {
    int tc[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) tc[q] = imu_tile_const(lane + 64 * q);
    const int tcg = imu_col(min(lane, 23), 0, 0, 0);
#pragma unroll
    for (int u = 0; u < NGI; ++u) {
      if (part * NW + wave + u * per_round >= ngrp) continue;
      const int sg = __builtin_amdgcn_readfirstlane(gs_[u]);   // (one group per wave: uniform; read here, so that the requests above stay in flight together)
      imu_tile_add(Hs, sg, tc, tv[u]);
      if (STORE && lane < 24) atomicAdd(&Hs[nHh + 6 * sg + tcg], tgv[u]);   // (gs = Hs + nHh)
    }
  }
  double *Js = stage + wave * SROWS * CHP;
  int *ks = keys + wave * 2 * CH;
  const size_t V = (size_t)d.Vtot;
  // every wave owns a contiguous range of items: a run that continues into the wave's next item keeps its accumulators
  // and is scattered once (the scatter costs as much as the products of an item: ~5 k cycles, measured)
  const int it0 = (int)((long long)nvitem * (part * NW + wave) / per_round);
  const int rounds = (int)((long long)nvitem * (part * NW + wave + 1) / per_round) - it0;
  double *Hg = d.HppS[tgset] + m.H0;
  const int q4 = lane >> 4, l15 = lane & 15, bsel = q4 >> 1, rr = q4 & 1;   // MFMA k index = 2 * (block of the pair) + residual row
  const int sc = lane % CH, srr = lane / CH;                               // staging: column (block) and row parity of this lane
  long long *dbg = (d.dbg && w == (d.nwin > 1000 ? 1000 : 0) && part == 0) ? d.dbg + 48 : nullptr;
  int dbi = 0;
  if (dbg && tid == 0) dbg[dbi++] = t_begin;
  CTV_STAMP(dbg, dbi, 15, tid == 0);
  // MFMA operand row offsets of this lane: tile row I -> knot column 16 I + l15, at k = q4 (block bsel of the pair, residual
  // row rr).  The line-delay column (staged rows 98, 99) and the residual (rows 100, 101) ride on the same operand
  // values with plain FMAs: every lane multiplies its three J entries by J_ld[k] and r[k] of its own k; the four k
  // groups (lanes l15 + 16 q4) are summed with two shuffles per value at the end of the run.
  // The tiles run over the columns in knot-major order (vis_knot_major_to_col): tile column 16 I + l15 reads the staged row of the vis_col
  // column behind it -- the only place the order shows before the scatter; every product is the same sum in the same K order.
  int orow[3];
#pragma unroll
  for (int I = 0; I < 3; ++I) orow[I] = (2 * vis_knot_major_to_col(16 * I + l15) + rr) * CHP;
  const int ldrow = (98 + rr) * CHP, rrow = (100 + rr) * CHP;
  double tj[5], tg9[9], tc0 = 0.0;
  int n = 0, v0 = 0, key_i = 0, key_j = 0;
  // the (start, count) of this wave's items: lane r holds item r, read once -- a per-item load of the descriptor would put a
  // full memory round trip in front of every item's J~ request
  int my_start, my_count;
  {
    const int it = it0 + lane;
    const VisItem I = d.vitems[vitem0 + min(it, max(nvitem - 1, 0))];   // clamped: always a valid descriptor
    my_start = I.start;
    my_count = (lane < rounds && it < nvitem) ? I.count : 0;
  }
  auto item_desc = [&](int r, int &istart, int &icount) {
    if (r < 64) { istart = __builtin_amdgcn_readlane(my_start, r); icount = __builtin_amdgcn_readlane(my_count, r); }   // (r is wave-uniform)
    else {
      const int it = it0 + r;
      const VisItem I = d.vitems[vitem0 + min(it, nvitem - 1)];
      istart = I.start; icount = (r < rounds && it < nvitem) ? I.count : 0;
    }
    if (r >= rounds) icount = 0;
  };
  // The blocks of an item are slots of the landmark-major evaluation order, listed in Dev::vblk: the slot of this lane's block
  // (c = sc) and of the block whose keys it reads (lane) are requested one item ahead, so that the J~ loads of an item do not
  // wait for its slot list.
  int idn = 0, idkn = 0, ian = 0, iakn = 0;
  auto load_ids = [&](int r) {
    int istart, icount;
    item_desc(r, istart, icount);
    idn = d.vblk[istart + (sc < icount ? sc : 0)];
    ian = d.vblk_anc[istart + (sc < icount ? sc : 0)];
    idkn = d.vblk[istart + (lane < icount ? lane : 0)];
    iakn = d.vblk_anc[istart + (lane < icount ? lane : 0)];
  };
  auto fetch = [&](int r) {   // request item r of this wave: unconditional loads on clamped addresses, masked when staged
    int istart, icount;
    item_desc(r, istart, icount);
    n = icount;
    v0 = istart;
    // The block records are block-major ([slot][VT_ROWS]); lane (sc, srr) takes entries srr + 8 i of its block: 0..23 the j end's
    // rotation columns, 26..33 line delay / residual / A~[0..3], 34..39 A~[4, 5] and cp1 (the inverse-depth entries 24, 25 are
    // skipped) -- the RPP lanes of a block read RPP consecutive entries.  From the anchor record: the three factors GR[c][0..2] of the
    // lane's three anchor-end rotation entries e = srr + 8 i (column c = e / 2) and one of the four cp0.
    const unsigned jb = (unsigned)idn * (unsigned)VT_ROWS + (unsigned)srr;
#pragma unroll
    for (int i = 0; i < 3; ++i) tj[i] = d.Jt[jb + (unsigned)(8 * i)];
    tj[3] = d.Jt[jb + 26u];
    tj[4] = d.Jt[(unsigned)idn * (unsigned)VT_ROWS + (unsigned)min(34 + srr, VT_ROWS - 1)];
    const double *rec = d.arec + (size_t)ian * AREC;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int mm = 0; mm < 3; ++mm) tg9[3 * i + mm] = rec[AR_GR + 3 * ((srr + 8 * i) >> 1) + mm];
    tc0 = rec[AR_CP0 + (srr & 3)];
    key_i = d.a_s[iakn];
    key_j = d.vsj[idkn];
    load_ids(r + 1);
  };
  if (nvitem > 0) load_ids(0);
  if (nvitem > 0) fetch(0);
  // accumulators of the open run (asi, asj): 3 x 3 lower tiles of the 48 x 48 pose block, line-delay column, residual
  acc_t acc[6];
  double pl[3], pr[3], pll, prl;
  int asi = -1, asj = -1;
  auto reset_acc = [&]() {
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[q] = acc_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int I = 0; I < 3; ++I) { pl[I] = 0.0; pr[I] = 0.0; }
    pll = 0.0; prl = 0.0;
  };
  // ---- scatter: local column c (knot-major) -> unknown 6 si + c (c < 24) or 6 sj + c - 24; each unordered local pair once, placed at
  //      (max, min); pairs of different local columns that map to the same unknown (ends sharing a knot) count twice on the diagonal.
  //      A run whose j end lies wholly after its i end (sj >= si + 4, wave-uniform) needs none of the per-element decisions: within an end
  //      and from the j end's rows to the i end's columns the local order is the order of the unknowns, and no two columns meet.
  auto scatter = [&](int si, int sj) {
#pragma unroll
    for (int I = 0; I < 3; ++I) { pl[I] = rowgroup_sum(pl[I]); pr[I] = rowgroup_sum(pr[I]); }
    pll = rowgroup_sum(pll); prl = rowgroup_sum(prl);
    // unknown index and triangular row offset g (g + 1) / 2 of this lane's 3 tile columns and 12 tile rows, once per run: tile 0 lies in
    // the i end, tile 2 in the j end, tile 1 changes ends at its local column 8 (row groups rg < 2 | rg >= 2)
    const int bi = 6 * si, bj = 6 * sj - 24;
    int gcol[3], grow[3][4], trow[3][4];
    gcol[0] = bi + l15; gcol[1] = 16 + l15 + (l15 < 8 ? bi : bj); gcol[2] = bj + 32 + l15;
#pragma unroll
    for (int I = 0; I < 3; ++I) {
      const int g0 = 16 * I + q4 + (I == 0 ? bi : bj), g1 = 16 * I + q4 + (I == 2 ? bj : bi);   // rows rg = 2, 3 | rg = 0, 1
      grow[I][0] = g1; grow[I][1] = g1 + 4; grow[I][2] = g0 + 8; grow[I][3] = g0 + 12;
      trow[I][0] = g1 * (g1 + 1) / 2; trow[I][1] = trow[I][0] + 4 * g1 + 10;                    // t(g + 4) = t(g) + 4 g + 10
      trow[I][2] = I == 1 ? (g0 + 8) * (g0 + 9) / 2 : trow[I][1] + 4 * g1 + 26;
      trow[I][3] = trow[I][2] + 4 * g0 + 42;
    }
    if (sj - si >= 4) {
      int q = 0;
#pragma unroll
      for (int I = 0; I < 3; ++I)
#pragma unroll
        for (int J = 0; J <= I; ++J, ++q) {
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            if (I == J && q4 + 4 * rg < l15) continue;
            if (LDSH) atomicAdd(&Hs[trow[I][rg] + gcol[J]], acc[q][rg]);
            else atomicAdd(&Hg[(long long)grow[I][rg] * ldh + gcol[J]], acc[q][rg]);
          }
        }
    } else {
      int tcol[3];
#pragma unroll
      for (int J = 0; J < 3; ++J) tcol[J] = gcol[J] * (gcol[J] + 1) / 2;
      int q = 0;
#pragma unroll
      for (int I = 0; I < 3; ++I)
#pragma unroll
        for (int J = 0; J <= I; ++J, ++q) {
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const int ca = 16 * I + (q4 + 4 * rg), cb = 16 * J + l15;
            if (I == J && ca < cb) continue;
            const int gA = grow[I][rg], gB = gcol[J];
            double hv = acc[q][rg];
            if (gA == gB && ca != cb) hv *= 2.0;
            const bool ge = gA >= gB;
            if (LDSH) atomicAdd(&Hs[(ge ? trow[I][rg] : tcol[J]) + (ge ? gB : gA)], hv);
            else atomicAdd(&Hg[(long long)(ge ? gA : gB) * ldh + (ge ? gB : gA)], hv);
          }
        }
    }
    // line-delay row of the Hessian and the pose gradient (every k group holds the totals; group q4 = 0 adds them)
    if (q4 == 0) {
#pragma unroll
      for (int J = 0; J < 3; ++J) {
        if (LDSH) atomicAdd(&Hs[tri + gcol[J]], pl[J]);
        else atomicAdd(&Hg[(long long)(P - 1) * ldh + gcol[J]], pl[J]);
        atomicAdd(&gs[gcol[J]], pr[J]);
      }
      if (l15 == 0) {   // (ld, ld) and r . J_ld
        if (LDSH) atomicAdd(&Hs[tri + K6], pll);
        else atomicAdd(&Hg[(long long)(P - 1) * ldh + (P - 1)], pll);
        atomicAdd(&gs[K6], prl);
      }
    }
  };
  for (int r = 0; r < rounds && nvitem > 0; ++r) {
    // ---- stage the fetched item (LDS operations of one wave are ordered: no barrier), then request the next one
    const int ncur = n;
    {
      const bool in = sc < ncur;
#pragma unroll
      for (int i = 0; i < 3; ++i) Js[(48 + srr + 8 * i) * CHP + sc] = in ? tj[i] : 0.0;
      Js[(98 + srr) * CHP + sc] = in ? tj[3] : 0.0;                     // rows 98..105: line delay, residual, A~[0..3]
      if (srr < 2) Js[(106 + srr) * CHP + sc] = in ? tj[4] : 0.0;       // A~[4, 5]
      else if (srr < 6) Js[(110 + srr) * CHP + sc] = in ? tj[4] : 0.0;  // cp1 (entries 36..39 -> rows 112..115)
      if (srr < 4) Js[(108 + srr) * CHP + sc] = in ? tc0 : 0.0;         // cp0 (anchor record)
    }
    if (lane < CH) { ks[lane] = key_i; ks[CH + lane] = key_j; }
    __builtin_amdgcn_wave_barrier();
    // anchor end's rotation rows: entry e = srr + 8 i (= 2 * column + residual row) = A~[rr][0..2] . GR[column][0..2]
    // position rows: column 12 + 3 k + b (i end) = cp0[k] P~[b], column 36 + 3 k + b (j end) = -cp1[k] P~[b]
    // All LDS reads of both expansions (rows 102..115) come before the first write (rows 0..95): the compiler keeps LDS reads behind
    // earlier LDS writes, and read-multiply-write per row put eight LDS round trips in a row into every item.
    {
      const int rr2 = srr & 1;
      const double a0 = Js[(102 + rr2) * CHP + sc], a1 = Js[(104 + rr2) * CHP + sc], a2 = Js[(106 + rr2) * CHP + sc];   // (zero for sc >= ncur)
      constexpr int HALF = 24 / RPP;
      double pv[HALF], cv[2][HALF];
#pragma unroll
      for (int h = 0; h < HALF; ++h) {
        const int rem = h * RPP + srr, pc = rem >> 1, kk = pc / 3, b = pc - 3 * kk;    // rem = 2 * (3 k + b) + residual row
        pv[h] = Js[(102 + 2 * b + (rem & 1)) * CHP + sc];
        cv[0][h] = Js[(108 + kk) * CHP + sc];
        cv[1][h] = Js[(112 + kk) * CHP + sc];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) Js[(srr + 8 * i) * CHP + sc] = a0 * tg9[3 * i] + a1 * tg9[3 * i + 1] + a2 * tg9[3 * i + 2];
#pragma unroll
      for (int e = 0; e < NEXP; ++e) {
        const int side = e / HALF, h = e % HALF;
        Js[(24 + 48 * side + h * RPP + srr) * CHP + sc] = side ? -(cv[1][h] * pv[h]) : cv[0][h] * pv[h];
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (r < 2) CTV_STAMP(dbg, dbi, 15, tid == 0);
    fetch(r + 1);
    int start = 0;
    while (start < ncur) {
      const int si = ks[start], sj = ks[CH + start];
      const bool diff = (lane > start && lane < ncur) && (ks[lane] != si || ks[CH + lane] != sj);
      const unsigned long long mask = __ballot(diff);
      const int end = mask ? (__ffsll((long long)mask) - 1) : ncur;
      if (asi != si || asj != sj) {     // a run that continues from the previous item keeps accumulating
        if (asi >= 0) scatter(asi, asj);
        reset_acc();
        asi = si; asj = sj;
      }
      // 4 K-steps (8 blocks) per trip: the operand reads first, then the products -- one LDS latency per trip
      for (int v8 = start; v8 < end; v8 += 8) {
        double a[4][3], ldv[4], rv[4];
        // (the usual item is one run that ends with the item: the columns past it were staged as zeros, nothing to mask)
        const bool nomask = end == ncur && v8 + 8 <= CH;     // uniform
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int blk = v8 + 2 * s + bsel;
          const int bc = min(blk, CH);       // a valid LDS address even when past the run (value discarded)
#pragma unroll
          for (int I = 0; I < 3; ++I) a[s][I] = Js[orow[I] + bc];
          ldv[s] = Js[ldrow + bc];
          rv[s] = Js[rrow + bc];
        }
        if (!nomask) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const bool in = v8 + 2 * s + bsel < end;
#pragma unroll
            for (int I = 0; I < 3; ++I) a[s][I] = in ? a[s][I] : 0.0;
            ldv[s] = in ? ldv[s] : 0.0;
            rv[s] = in ? rv[s] : 0.0;
          }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          if (v8 + 2 * s >= end) break;     // uniform
          int q = 0;
#pragma unroll
          for (int I = 0; I < 3; ++I)
#pragma unroll
            for (int J = 0; J <= I; ++J, ++q) acc[q] = mfma16(a[s][I], a[s][J], acc[q]);
#pragma unroll
          for (int I = 0; I < 3; ++I) { pl[I] += a[s][I] * ldv[s]; pr[I] += a[s][I] * rv[s]; }
          pll += ldv[s] * ldv[s];
          prl += rv[s] * ldv[s];
        }
      }
      if (r < 2) CTV_STAMP(dbg, dbi, 15, tid == 0);
      start = end;
    }
    if (r < 2) CTV_STAMP(dbg, dbi, 15, tid == 0);
  }
  if (asi >= 0) scatter(asi, asj);
  __syncthreads();
  CTV_STAMP(dbg, dbi, 15, tid == 0);
  // IMU group tiles: the knot x knot part (24 x 24 per group, overlapping between consecutive segments); without the LDS
  // Hessian k_assemble_imu adds them
  if (LDSH && part * NW + wave + NGI * per_round < ngrp) {   // groups beyond the prefetched ones
    // (the entry constants are formed again here, from a lane index the compiler cannot trace back: nine registers that would otherwise
    // stay live across the item loop)
    const int ln = lane + opaque_zero();
    int tc[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) tc[q] = imu_tile_const(ln + 64 * q);
    const int tcg = imu_col(min(ln, 23), 0, 0, 0);
    for (int gi = part * NW + wave + NGI * per_round; gi < ngrp; gi += per_round) {
      const int s = __builtin_amdgcn_readfirstlane(d.groups[grp0 + gi].s);
      const double *tile = d.imu_tiles + (size_t)(grp0 + gi) * 1024;
      double tv[9];   // 24 x 24 = 9 x 64 entries: all loads in flight together
#pragma unroll
      for (int u = 0; u < 9; ++u) { const int e = lane + 64 * u; tv[u] = tile[(e / 24) * 32 + e % 24]; }
      imu_tile_add(Hs, s, tc, tv);
      if (STORE && lane < 24) atomicAdd(&gs[6 * s + tcg], tile[lane * 32 + 30]);
    }
  }
  __syncthreads();
  CTV_STAMP(dbg, dbi, 15, tid == 0);
  if constexpr (STORE) {
    if (nparts > 1) {   // this part's packed Hessian + gradient: summed with the others, in part order, by k_reduce_finalize
      double *dst = d.Hpart + ((size_t)w * nparts + part) * d.npart_stride;
      for (int i = tid; i < nH; i += NT) dst[i] = Hs[i];
      return;
    }
    double *gq = d.gS[tgset] + u0;
    // the packed triangle by rows (wave -> rows, lane -> columns), then the line-delay row
    for (int ga = wave; ga < K6; ga += NW)
      for (int gb = lane; gb <= ga; gb += 64) Hg[(long long)ga * ldh + gb] = Hs[ga * (ga + 1) / 2 + gb] + prior_H(d, m, ga, gb);
    for (int i = tid; i < K6 + 1; i += NT) { const int gb = i < K6 ? i : P - 1; Hg[(long long)(P - 1) * ldh + gb] = Hs[tri + i] + prior_H(d, m, P - 1, gb); }
    for (int i = tid; i < K6 + 1; i += NT) { const int uu = i < K6 ? i : P - 1; gq[uu] = gs[i] + prior_g(d, m, uu); }
    return;   // (the bias rows: k_bias_rows -- a gather with dependent loads wants more waves per CU than this kernel's LDS allows)
  }
  if (LDSH) {   // the packed triangle by rows (wave -> rows, lane -> columns), then the line-delay row
    auto flush = [&](int ga, int gb, double hv) {
      if (nparts > 1) { if (hv != 0.0) atomicAdd(&Hg[(long long)ga * ldh + gb], hv); }
      else Hg[(long long)ga * ldh + gb] = hv;  // first writer after k_zero_normal; later kernels add atomically
    };
    for (int ga = wave; ga < K6; ga += NW)
      for (int gb = lane; gb <= ga; gb += 64) flush(ga, gb, Hs[ga * (ga + 1) / 2 + gb]);
    for (int i = tid; i < K6 + 1; i += NT) flush(P - 1, i < K6 ? i : P - 1, Hs[tri + i]);
  }
  CTV_STAMP(dbg, dbi, 15, tid == 0);
  for (int i = tid; i < K6 + 1; i += NT) {
    const double gv = gs[i];
    if (gv != 0.0) atomicAdd(&d.gS[tgset][u0 + (i < K6 ? i : P - 1)], gv);
  }
  CTV_STAMP(dbg, dbi, 15, tid == 0);
}

// Bias rows of the single-part store-semantics assembly: grid (blocks, windows).
__global__ __launch_bounds__(256) void k_bias_rows(Dev d, int mode) {
  const int w = blockIdx.y;
  if (!lin_run(d.lm[w], mode) || lin_cost_only(d.lm[w], mode, d.prm)) return;
  const WinMeta &m = d.wins[w];
  if (!m.vis_lds) return;
  bias_rows_store(d, m, lin_target(d.lm[w], mode), mode == LIN_SPEC ? d.cbias : d.bias, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// Several parts per window (batches smaller than the chip; the deterministic mode): sum of the parts' packed Hessians in part
// order, prior added, plain stores; the bias rows by gather.  Grid (blocks, windows).
__global__ __launch_bounds__(256) void k_reduce_finalize(Dev d, int mode, int nparts) {
  const int w = blockIdx.y;
  if (!lin_run(d.lm[w], mode) || lin_cost_only(d.lm[w], mode, d.prm)) return;
  const WinMeta &m = d.wins[w];
  if (!m.vis_lds) return;
  const int tg = lin_target(d.lm[w], mode);
  const int P = m.P, K6 = 6 * m.K, tri = K6 * (K6 + 1) / 2, nHh = tri + K6 + 1, nH = nHh + K6 + 1, ldh = m.ldh;
  double *Hg = d.HppS[tg] + m.H0, *g = d.gS[tg] + m.u0;
  const double *src = d.Hpart + (size_t)w * nparts * d.npart_stride;
  const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (int i = first; i < nH; i += stride) {
    double v = 0.0;
    int p = 0;
    for (; p + 8 <= nparts; p += 8) {   // eight loads in flight, added in part order
      double t8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) t8[q] = src[(size_t)(p + q) * d.npart_stride + i];
#pragma unroll
      for (int q = 0; q < 8; ++q) v += t8[q];
    }
    for (; p < nparts; ++p) v += src[(size_t)p * d.npart_stride + i];
    if (i < nHh) {
      int ga, gb;
      packed_decode(i, tri, K6, P, ga, gb);
      Hg[(long long)ga * ldh + gb] = v + prior_H(d, m, ga, gb);
    } else {
      const int uu = (i - nHh) < K6 ? (i - nHh) : P - 1;
      g[uu] = v + prior_g(d, m, uu);
    }
  }
  bias_rows_store(d, m, tg, mode == LIN_SPEC ? d.cbias : d.bias, first, stride);
}

// ---- order-fixed assembly of the windows whose packed Hessian is not LDS resident (vis_lds = 0; ctvio_options.deterministic = 2).  Every
// entry of the knot x knot block, the line-delay row and the pose gradient is owned by ONE workgroup (a 16 x 16 tile of the augmented pose
// block: unknowns 0 .. 6K - 1 the knots, 6K the line delay, 6K + 1 the residual, whose row is the gradient), formed completely and written
// with a plain store.  Its visual share is the sum over the blocks of the tile's walk, in the order of the upload plan (Dev::vrow: landmark
// rows in sorted order, a landmark's blocks in slot order), two blocks per v_mfma_f64_16x16x4f64 (K = 2 blocks x 2 residual rows, the
// operand layout of k_assemble_vis_mfma), the walk's chunks of 64 blocks dealt round-robin to the waves and their sums added in wave order;
// then the IMU group tiles that touch it, in group order; then the prior; then the store.  The bias rows
// come from k_bias_rows_wide (bias_rows_store), the prior gradient and the cost share from k_misc (store = 1).  No floating-point atomics.
//
// k_vis_expand: the compressed block records of k_vis_eval (Dev::Jt, the anchor records) expanded once per linearisation, in WALK order
// (entry vis0 + i = the i-th block of the window's walk, Dev::vrow), into the 48 pose columns (vis_col order), the line-delay column and
// the residual per residual row, and the two ends' first knots: [vis0 + i][2 x VX_COLS + 2].  The tiles visit a block ~15 times; the
// expansion is one pass, and the tiles' walks read consecutive records with no lookup chain in front of them.
constexpr int VX_COLS = 50, VX_LD = 2 * VX_COLS + 2;
__global__ __launch_bounds__(256) void k_vis_expand(Dev d, int mode) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (walk position, column): both residual rows
  if (e >= (long long)d.Vtot * (VX_COLS + 1)) return;
  const int pos = (int)(e / (VX_COLS + 1)), c = (int)(e - (long long)pos * (VX_COLS + 1));
  const int w = d.vb_win[pos / 64];
  const WinMeta &m = d.wins[w];
  if (pos - m.vis0 >= m.V) return;   // (the unused tail of the window's range: never walked)
  if (!lin_run(d.lm[w], mode) || lin_cost_only(d.lm[w], mode, d.prm) || m.vis_lds) return;
  const int slot = m.vis0 + d.vrow[pos];
  double *out = d.vexp + (size_t)pos * VX_LD;
  if (c == VX_COLS) { out[2 * VX_COLS] = (double)d.a_s[d.v_anc[slot]]; out[2 * VX_COLS + 1] = (double)d.vsj[slot]; return; }
  const double *J = d.Jt + (size_t)slot * VT_ROWS;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    double v;
    if (c < 12) {          // anchor end, rotation: A~[rr] . GR[c]
      const double *gr = d.arec + (size_t)d.v_anc[slot] * AREC + AR_GR + 3 * c;
      v = J[VB_AT + rr] * gr[0] + J[VB_AT + 2 + rr] * gr[1] + J[VB_AT + 4 + rr] * gr[2];
    } else if (c < 24) {   // anchor end, position: cp0[k] A~[rr][b]
      const int k = (c - 12) / 3, b = (c - 12) % 3;
      v = d.arec[(size_t)d.v_anc[slot] * AREC + AR_CP0 + k] * J[VB_AT + 2 * b + rr];
    } else if (c < 36) {   // j end, rotation
      v = J[VB_JROT + 2 * (c - 24) + rr];
    } else if (c < 48) {   // j end, position: -cp1[k] A~[rr][b]
      const int k = (c - 36) / 3, b = (c - 36) % 3;
      v = -(J[VB_CP1 + k] * J[VB_AT + 2 * b + rr]);
    } else {
      v = J[(c == 48 ? VB_LD : VB_RES) + rr];
    }
    out[VX_COLS * rr + c] = v;
  }
}
// Value of augmented unknown u in residual row rr of an expanded block whose ends start at knots si, sj (ends that share a knot add up).
__device__ __forceinline__ double vx_value(const double *X, int si, int sj, int u, int K6) {
  if (u >= K6) return u == K6 ? X[48] : (u == K6 + 1 ? X[49] : 0.0);
  const int k = u / 6, c = u - 6 * k, ki = k - si, kj = k - sj;
  double v = 0.0;
  if (ki >= 0 && ki < 4) v += X[c < 3 ? 3 * ki + c : 9 + 3 * ki + c];
  if (kj >= 0 && kj < 4) v += X[c < 3 ? 24 + 3 * kj + c : 33 + 3 * kj + c];
  return v;
}
// a block (ends at knots si, sj) reaches augmented columns [t0, t0 + 16)
__device__ __forceinline__ bool vx_reaches(int si, int sj, int t0, int K6) {
  return t0 + 15 >= K6 || (6 * si <= t0 + 15 && 6 * si + 23 >= t0) || (6 * sj <= t0 + 15 && 6 * sj + 23 >= t0);
}
// the sorted rows of W whose landmark can reach augmented tile T (the line-delay / residual tile: every observed landmark)
__device__ __forceinline__ void wide_rows(const Dev &d, const WinMeta &m, int T, int &b, int &e) {
  if (16 * T + 15 < 6 * m.K) { b = d.tl_beg[m.tr0 + T]; e = d.tl_end[m.tr0 + T]; }
  else { b = 0; e = m.Lobs; }
}
// Grid (tiles, windows): one workgroup of WIDE_NW waves per tile, the tiles of the last row (line delay, gradient: every block reaches them)
// first.  Wave v walks the chunks v, v + WIDE_NW, ... of 64 blocks of the tile's walk; wave 0 adds the other waves' sums in wave order.
constexpr int WIDE_NW = 4;
__global__ __launch_bounds__(64 * WIDE_NW) void k_assemble_wide(Dev d, int mode) {
  const int w = blockIdx.y;
  if (!lin_run(d.lm[w], mode) || lin_cost_only(d.lm[w], mode, d.prm)) return;
  const WinMeta &m = d.wins[w];
  if (m.vis_lds) return;
  const int K6 = 6 * m.K, na = K6 + 2, nt = (na + 15) / 16, P = m.P, ldh = m.ldh;
  if ((int)blockIdx.x >= nt * (nt + 1) / 2) return;     // (uniform over the workgroup)
  const int tile = nt * (nt + 1) / 2 - 1 - (int)blockIdx.x, wave = threadIdx.x >> 6;
  __shared__ double part[WIDE_NW - 1][4][64];
  int R = (int)((sqrtf(8.0f * (float)tile + 1.0f) - 1.0f) * 0.5f);
  R += ((R + 1) * (R + 2) / 2 <= tile) ? 1 : 0;
  R -= (R * (R + 1) / 2 > tile) ? 1 : 0;
  const int C = tile - R * (R + 1) / 2, r0 = 16 * R, c0 = 16 * C;
  const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4, bsel = kq >> 1, rr = kq & 1;
  const int ua = r0 + l15, ub = c0 + l15;     // the unknowns of this lane's A (tile row) and B (tile column) operand
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  // ---- visual blocks: the rows of W that can reach both the tile's rows and its columns, their blocks in plan order
  int bR, eR, bC, eC;
  wide_rows(d, m, R, bR, eR);
  wide_rows(d, m, C, bC, eC);
  const int lo = max(bR, bC), hi = min(eR, eC);
  if (hi > lo) {
    const int32_t *off = d.vrow_off + m.lm0 + w;      // (window w's L + 1 offsets start at lm0 + w)
    const int i0 = m.vis0 + off[lo], i1 = m.vis0 + off[hi];
    // 64 blocks of the walk per trip: lane q reads the ends of block base + q (the next trip's are requested before this trip's products);
    // the blocks that reach both ranges at the CURRENT line delay are taken in walk order, up to 2 NPR per round (NPR products with all
    // their operand loads in flight)
    constexpr int NPR = 8;
    auto ends = [&](int base, int &si, int &sj) {
      const size_t p = (size_t)min(base + lane, max(i1 - 1, 0)) * VX_LD + 2 * VX_COLS;
      si = (int)d.vexp[p]; sj = (int)d.vexp[p + 1];
    };
    int nsi = 0, nsj = 0;
    if (i0 + 64 * wave < i1) ends(i0 + 64 * wave, nsi, nsj);
    for (int base = i0 + 64 * wave; base < i1; base += 64 * WIDE_NW) {
      const int si = nsi, sj = nsj;
      if (base + 64 * WIDE_NW < i1) ends(base + 64 * WIDE_NW, nsi, nsj);
      const bool use = base + lane < i1 && vx_reaches(si, sj, r0, K6) && vx_reaches(si, sj, c0, K6);
      unsigned long long mask = __ballot(use);
      while (mask) {
        double av[NPR], bv[NPR];
#pragma unroll
        for (int p = 0; p < NPR; ++p) {
          int b0 = -1, b1 = -1;
          if (mask) { b0 = __ffsll((long long)mask) - 1; mask &= mask - 1; }
          if (mask) { b1 = __ffsll((long long)mask) - 1; mask &= mask - 1; }
          const int s = bsel ? b1 : b0;
          const int ssi = __shfl(si, max(s, 0)), ssj = __shfl(sj, max(s, 0));
          const double *X = d.vexp + (size_t)(base + max(s, 0)) * VX_LD + VX_COLS * rr;
          av[p] = s >= 0 ? vx_value(X, ssi, ssj, ua, K6) : 0.0;
          bv[p] = s >= 0 ? vx_value(X, ssi, ssj, ub, K6) : 0.0;
        }
#pragma unroll
        for (int p = 0; p < NPR; ++p) acc = mfma16(av[p], bv[p], acc);
      }
    }
  }
  // D register j of lane l = D[(l / 16) + 4 j][l % 16]: entries (r0 + kq + 4 j, ub)
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) part[wave - 1][j][lane] = acc[j];
  }
  __syncthreads();
  if (wave > 0) return;
  double h[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[j] = acc[j];
#pragma unroll
    for (int v = 0; v < WIDE_NW - 1; ++v) h[j] += part[v][j][lane];
  }
  // ---- IMU group tiles (knots s .. s + 3, in group order; the groups are sorted by segment) that touch the tile's rows and columns
  const bool grad_rows = r0 + 15 >= K6 + 1;
  for (int base = 0; base < m.ngrp; base += 64) {
    const int gi = base + lane;
    int s = 0;
    bool use = false;
    if (gi < m.ngrp) {
      s = d.groups[m.grp0 + gi].s;
      const bool row_hit = (6 * s <= r0 + 15 && 6 * s + 23 >= r0) || grad_rows, col_hit = 6 * s <= c0 + 15 && 6 * s + 23 >= c0;
      use = row_hit && col_hit;
    }
    unsigned long long mask = __ballot(use);
    while (mask) {
      const int q = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int sg = __shfl(s, q);
      const double *tl = d.imu_tiles + (size_t)(m.grp0 + base + q) * 1024;
      const int kb = ub / 6 - sg, cb = ub - 6 * (ub / 6);
      const int ib = (ub < K6 && kb >= 0 && kb < 4) ? (cb < 3 ? 3 * kb + cb : 9 + 3 * kb + cb) : -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ua2 = r0 + kq + 4 * j;
        if (ib < 0 || ua2 > K6 + 1 || ua2 == K6) continue;
        if (ua2 == K6 + 1) { h[j] += tl[ib * 32 + 30]; continue; }
        const int ka = ua2 / 6 - sg, ca = ua2 - 6 * (ua2 / 6);
        if (ka >= 0 && ka < 4) h[j] += tl[(ca < 3 ? 3 * ka + ca : 9 + 3 * ka + ca) * 32 + ib];
      }
    }
  }
  // ---- prior, then the store: augmented unknown 6K = the line delay (P - 1), row 6K + 1 = the gradient
  const int tg = lin_target(d.lm[w], mode);
  double *Hg = d.HppS[tg] + m.H0, *g = d.gS[tg] + m.u0;
  const int gb = ub < K6 ? ub : P - 1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ua2 = r0 + kq + 4 * j;
    if (ua2 >= na || ub > ua2 || ub > K6) continue;
    if (ua2 == K6 + 1) { g[gb] = h[j] + prior_g(d, m, gb); continue; }
    const int ga = ua2 < K6 ? ua2 : P - 1;
    Hg[(long long)ga * ldh + gb] = h[j] + prior_H(d, m, ga, gb);
  }
}
// Bias rows of the wide windows (the same gather as k_bias_rows): grid (blocks, windows).
__global__ __launch_bounds__(256) void k_bias_rows_wide(Dev d, int mode) {
  const int w = blockIdx.y;
  if (!lin_run(d.lm[w], mode) || lin_cost_only(d.lm[w], mode, d.prm)) return;
  const WinMeta &m = d.wins[w];
  if (m.vis_lds) return;
  bias_rows_store(d, m, lin_target(d.lm[w], mode), mode == LIN_SPEC ? d.cbias : d.bias, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// ------------------------------------------------------------------------------------------------ bias chain + prior
__device__ __forceinline__ const double *prior_block_ptr(const WinMeta &m, int kind, int idx, const double *quat, const double *pos,
                                                         const double *bias, const double *ldp, int w) {
  switch (kind) {
    case 0: return quat + 4 * (m.knot0 + idx);
    case 1: return pos + 3 * (m.knot0 + idx);
    case 2: return bias + 6 * (m.bias0 + idx);
    case 3: return bias + 6 * (m.bias0 + idx) + 3;
    default: return ldp + w;
  }
}

// BiasFactor (trajectory_value_factor.h:45-99) and MarginalizationFactor (marginalization_factor.cpp:326-373), fp64.
// With the prior written r = r0 + J0 dx:  J^T r = J0^T r0 + (J0^T J0) dx,  |r|^2 = r0^T r0 + 2 b0.dx + dx^T (J0^T J0) dx.
// Adds to Hpp / g of the set the mode selects (not on a cost-only pass) and stores the window's cost share (Dev::misc_cost).
// store != 0 (store-semantics assembly tail): nothing is added here -- the prior's gradient J0^T r0 + (J0^T J0) dx goes to Dev::pgrad,
// and the assembly looks the prior and the chain up when it writes each entry.
// with_imu != 0: the window's IMU group tiles are scattered first (assemble_imu_window: the accumulate path's k_assemble_imu, fused).
// NT threads per workgroup: 256 (k_misc), or 64 when the store-semantics part (prior gradient + cost share, with_imu = 0) rides in k_pre_linearize.
// The cost share comes out bit-for-bit the same for both NT (the deterministic mode promises equal bits whichever launch shape a batch
// takes -- profiling and CTVIO_SPLIT_LINEARIZE=1 select k_misc): term e of each list (bias-chain entries, then prior rows) belongs to
// virtual lane e % MISC_LANES, a lane adds its terms in list order, and the MISC_LANES partial sums go through one fixed tree.  Thread
// tid of an NT-wide workgroup runs the virtual lanes tid, tid + NT, ...
constexpr int MISC_LANES = 256;
// The largest prior dimension whose dx fits k_pre_linearize's LDS in front of the reduction cells.  A valid window has pn <= P (duplicate
// blocks are refused) and P <= ~590 (the single-workgroup Cholesky); the host launches k_misc instead for a batch beyond this.
constexpr int PRE_LIN_MAX_PN = 600;
template <int NT> __device__ __forceinline__ void misc_body(const Dev &d, int mode, int store, int with_imu, int w, double *smd /* LDS [pn (+ band)] */, double *red /* LDS [MISC_LANES] */) {
  static_assert(MISC_LANES % NT == 0, "every thread runs the same number of virtual lanes");
  constexpr int R = MISC_LANES / NT;
  // with_imu == 2: the launch carries 144 maxK doubles of LDS behind the prior's dx for the band of the IMU knot blocks (windows with K > 24)
  if (with_imu) { assemble_imu_window(d, mode, w, with_imu == 2 ? smd + ((max(d.maxPn, 1) + 1) & ~1) : nullptr); __syncthreads(); }
  const Lm &lm = d.lm[w];
  if (!lin_run(lm, mode)) return;
  const bool LIN = !lin_cost_only(lm, mode, d.prm) && !store;
  const WinMeta &m = d.wins[w];
  const bool at_cand = mode == LIN_SPEC;
  const double *quat = at_cand ? d.cquat : d.quat, *pos = at_cand ? d.cpos : d.pos, *bias = at_cand ? d.cbias : d.bias, *ldp = at_cand ? d.cld : d.ld;
  const int tg = lin_target(lm, mode);
  double *Hpp = d.HppS[tg] + m.H0, *g = d.gS[tg] + m.u0;
  double *dx = smd;                 // [pn]
  const int tid = threadIdx.x;
  double cost[R];   // [q]: virtual lane q NT + tid
#pragma unroll
  for (int q = 0; q < R; ++q) cost[q] = 0.0;
  const int nbc = m.NB * 6;
  for (int e0 = 0; e0 < nbc; e0 += MISC_LANES) {
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int e = e0 + q * NT + tid;
      if (e >= nbc) continue;
      const int b = e / 6, k = e % 6;
      const int bi = d.bc_i[m.bc0 + b], bj = d.bc_j[m.bc0 + b];
      const double wv = d.bc_w[(size_t)(m.bc0 + b) * 6 + k];
      const double r = wv * (bias[6 * (m.bias0 + bj) + k] - bias[6 * (m.bias0 + bi) + k]);
      cost[q] += 0.5 * r * r;
      if (LIN) {
        const int ii = 6 * m.K + 6 * bi + k, jj = 6 * m.K + 6 * bj + k;
        atomicAdd(&g[ii], -wv * r);
        atomicAdd(&g[jj], wv * r);
        atomicAdd(&Hpp[(long long)ii * m.ldh + ii], wv * wv);
        atomicAdd(&Hpp[(long long)jj * m.ldh + jj], wv * wv);
        const int hi = max(ii, jj), lo = min(ii, jj);
        atomicAdd(&Hpp[(long long)hi * m.ldh + lo], -wv * wv);
      }
    }
  }
  const int n = m.pn;
  if (n > 0) {
    for (int i = tid; i < n; i += NT) dx[i] = 0.0;
    __syncthreads();
    for (int b = tid; b < m.pnb; b += NT) {
      const int kind = d.p_kind[m.pblk0 + b], idx = d.p_index[m.pblk0 + b], off = d.p_off[m.pblk0 + b];
      const double *x = prior_block_ptr(m, kind, idx, quat, pos, bias, ldp, w);
      const double *x0 = d.p_x0 + 4 * (size_t)(m.pblk0 + b);
      if (kind == 0) {  // dx = 2 vec(q0^-1 q), sign-fixed (marginalization_factor.cpp:344-350)
        const Q4 dq = qmul_raw(qmk(-x0[0], -x0[1], -x0[2], x0[3]), qmk(x[0], x[1], x[2], x[3]));
        const double sg = (dq.w >= 0) ? 2.0 : -2.0;
        dx[off] = sg * dq.x; dx[off + 1] = sg * dq.y; dx[off + 2] = sg * dq.z;
      } else {
        const int sz = (kind == 4) ? 1 : 3;
        for (int k = 0; k < sz; ++k) dx[off + k] = x[k] - x0[k];
      }
    }
    __syncthreads();
    const double *pH = d.pH + m.pH0, *b0 = d.pb0 + m.pv0;
    const int *pcol = d.pcol + m.pv0;
    for (int i0 = 0; i0 < n; i0 += MISC_LANES) {
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int i = i0 + q * NT + tid;
        if (i >= n) continue;
        double hd = 0.0;
        for (int j = 0; j < n; ++j) hd += pH[(size_t)j * n + i] * dx[j];   // (J0^T J0 is symmetric: column i, coalesced over the threads)
        cost[q] += dx[i] * (b0[i] + 0.5 * hd);
        if (store) d.pgrad[m.pv0 + i] = b0[i] + hd;
        if (LIN && pcol[i] >= 0) atomicAdd(&g[pcol[i]], b0[i] + hd);
      }
    }
    if (tid == 0) cost[0] += 0.5 * d.pc0[w];
    if (LIN) {
      for (int e = tid; e < n * n; e += NT) {
        const int i = e / n, j = e % n;
        const int ci = pcol[i], cj = pcol[j];
        if (ci >= 0 && cj >= 0 && ci >= cj) atomicAdd(&Hpp[(long long)ci * m.ldh + cj], pH[e]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < R; ++q) red[q * NT + tid] = cost[q];
  __syncthreads();
  for (int st = MISC_LANES / 2; st > 0; st >>= 1) {
    for (int c = tid; c < st; c += NT) red[c] += red[c + st];
    __syncthreads();
  }
  if (tid == 0) {
    d.misc_cost[w] = red[0];
    if (store && !lin_cost_only(lm, mode, d.prm)) {   // (the generic path resets these in k_zero_normal)
      if (mode == LIN_SPEC) d.lm[w].cand_gmax_bits = 0ull; else d.lm[w].gmax_bits = 0ull;
    }
  }
}
__global__ __launch_bounds__(256) void k_misc(Dev d, int mode, int store, int with_imu) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  __shared__ double red[MISC_LANES];
  misc_body<256>(d, mode, store, with_imu, blockIdx.x, smd, red);
}
// Small batches (the merged linearisation, <= 128 windows): everything that must precede k_linearize_f64 or is independent of it in ONE launch of
// 64-thread workgroups -- [0, nA) the anchors' records (k_vis_anchor), [nA, nA + nwin) the IMU groups the specialised body leaves out
// (k_imu_linearize_rest; nothing to do as a rule), and, on the store-semantics path, [nA + nwin, nA + 2 nwin) the prior gradient + cost share
// (k_misc with store = 1).  For one window these were three launches of 5 - 7 us each in a pass of 180 us (the reference's operating mode:
// one UpdateTrajectory per image, odometry_manager.cpp:268-277); their latencies now overlap.  The general IMU body sets the register
// allocation (one wave per SIMD), which a batch smaller than the chip does not feel.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_pre_linearize(Dev d, int mode, int general_only, int zero_mode, int n_anchor_blocks, int with_misc) {
  __shared__ __attribute__((aligned(32))) double srec[64 * AREC_LD];
  static_assert(64 * AREC_LD >= 64 * 33, "the general IMU body's row buffer uses the anchor records' staging area");
  static_assert(PRE_LIN_MAX_PN + MISC_LANES <= 64 * AREC_LD, "the misc share's dx and reduction cells share the staging area");
  const int b = blockIdx.x;
  if (b < n_anchor_blocks) { vis_anchor_body(d, mode, srec, b); return; }
  if (b < n_anchor_blocks + d.nwin) { imu_rest_body(d, mode, general_only, zero_mode, reinterpret_cast<unsigned char *>(srec), b - n_anchor_blocks); return; }
  // (dx: d.maxPn <= PRE_LIN_MAX_PN doubles -- the host passes with_misc = 0 otherwise -- in front of the reduction cells at the end)
  if (with_misc) misc_body<64>(d, mode, 1, 0, b - n_anchor_blocks - d.nwin, srec, srec + 64 * AREC_LD - MISC_LANES);
}

// Jacobi scaling (computed once, at iteration 0: Ceres jacobi_scaling), gradient max-norm of
// x - Plus(x, -g) (Ceres gradient_max_norm) and |x|^2 of the reduced program.
// |x - Plus(x, -g)| of unknown j (Ceres gradient_max_norm: ambient difference for a rotation block, the box of the line delay)
// (in two parts, so that a kernel that walks the unknowns in a loop can take the rotation blocks -- the quaternion product and its series -- outside it)
__device__ __forceinline__ double grad_norm_rot(const Dev &d, const WinMeta &m, int k, const double *g, bool at_cand) {
  // rotation block of knot k (unknown 6 k): ambient difference q - q*exp(-g)
  const double *q = (at_cand ? d.cquat : d.quat) + 4 * (m.knot0 + k);
  const int j = 6 * k;
  const Q4 q0 = qmk(q[0], q[1], q[2], q[3]);
  const Q4 q1 = qmul(q0, so3_exp(mk(-g[j], -g[j + 1], -g[j + 2])));
  return fmax(fmax(fabs(q0.x - q1.x), fabs(q0.y - q1.y)), fmax(fabs(q0.z - q1.z), fabs(q0.w - q1.w)));
}
__device__ __forceinline__ bool grad_norm_is_rot(const WinMeta &m, int j) { return j < 6 * m.K && j % 6 == 0; }
__device__ __forceinline__ double grad_norm_other(const Dev &d, const WinMeta &m, int w, int j, const double *g, bool at_cand) {   // (every unknown but a rotation block's first)
  if (j < 6 * m.K) return j % 6 >= 3 ? fabs(g[j]) : 0.0;
  if (j == m.P - 1) {
    const double ld = (at_cand ? d.cld : d.ld)[w];
    double nl = ld - g[j];
    if (!m.fix_ld) nl = fmin(fmax(nl, m.ld_lo), m.ld_hi);
    return fabs(ld - nl);
  }
  return fabs(g[j]);
}
__device__ __forceinline__ double grad_norm_entry(const Dev &d, const WinMeta &m, int w, int j, const double *g, bool at_cand) {
  return grad_norm_is_rot(m, j) ? grad_norm_rot(d, m, j / 6, g, at_cand) : grad_norm_other(d, m, w, j, g, at_cand);
}

// After the first linearisation of a solve (LIN_AT_X): Jacobi scaling (computed once, at iteration 0: Ceres jacobi_scaling) and the
// gradient max-norm of the initial state.  (Every later pass: k_pass_end.)
__global__ void k_post_linearize(Dev d, int mode) {
  const int w = blockIdx.y;
  Lm &lm = d.lm[w];
  if (!lin_run(lm, mode) || lin_cost_only(lm, mode, d.prm)) return;
  const WinMeta &m = d.wins[w];
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m.N) return;
  const bool at_cand = mode == LIN_SPEC;
  const int tg = lin_target(lm, mode);
  const bool act = d.active[m.u0 + j] != 0;
  if (!at_cand && !lm.scaled) {
    const double h = (j < m.P) ? d.HppS[tg][m.H0 + (long long)j * m.ldh + j] : d.HllS[tg][m.lm0 + j - m.P];
    d.cscale[m.u0 + j] = act ? 1.0 / (1.0 + sqrt(fmax(h, 0.0))) : 1.0;
  }
  if (!act) return;
  const double gm = grad_norm_entry(d, m, w, j, d.gS[tg] + m.u0, at_cand);
  if (gm > 0.0) atomicMax(at_cand ? &lm.cand_gmax_bits : &lm.gmax_bits, (unsigned long long)__double_as_longlong(gm));
}

}  // namespace ctv
