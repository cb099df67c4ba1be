// Test shim (CPU): the layout helper of the per-call entries (ctrl-vio_amd/csrc/host_pack.hpp: CallLayout) compiled with g++ against the HIP
// headers (no device code, nothing is launched).  The cases restate the segment lists of the entries of ctvio.hip at the smallest interesting
// sizes and the degenerate ones; tests/test_host_call_layout.py reads the offsets through the C functions and checks them, and the same
// file built with -DCALL_LAYOUT_MAIN -fsanitize=address,undefined is a stand-alone program that lays every case out over std::vector-backed
// bases, fills every segment through its typed pointer and reads it back.
#define __HIP_PLATFORM_AMD__ 1
#include "../ctrl-vio_amd/csrc/host_pack.hpp"

#include <cstdio>

namespace {
using ctv::CallLayout;
struct Seg { const char *name; size_t elem, count; bool dbl; };
struct Case {
  const char *name;
  std::vector<Seg> io, landing, scr;   // io: after the head, mirrored; landing: host only; scr: device only
  size_t nw, state;                    // the head: nw LM records, the poll words, `state` doubles
};
constexpr size_t D = sizeof(double), I = sizeof(int32_t), META = 200, TILE = 24, CWIN = 32;   // (stand-ins for MargMeta / CovTile / CovWin)

// one in-LDS marginalisation window: A / V / X / Y / rot / b (ctvio.hip: marg_device)
void marg_window(std::vector<Seg> &scr, size_t N, size_t m, size_t n) {
  const size_t np = std::max(m, n) + (std::max(m, n) & 1), rot = 24 * std::max<size_t>(np - 1, 1) * (np / 2) * 2;
  for (size_t c : {N * N, m * m, m * (n + 1), m * (n + 1), rot, n}) scr.push_back({"marg", D, c, true});
}
// the scratch of one blocked window: Bm Vm Bn Vn G Y X bp Q (ctvio.hip: mb_scratch)
std::vector<Seg> mb_window(size_t m, size_t n) {
  const size_t dm = m ? (m + 63) / 64 * 64 : 0, dn = (n + 63) / 64 * 64, mn1 = m * (n + 1);
  std::vector<Seg> s;
  for (size_t c : {dm * dm, dm * dm, dn * dn, dn * dn, mn1, mn1, mn1, n, std::max(dm, dn) / 64 * 64 * 64}) s.push_back({"mb", D, c, true});
  return s;
}
size_t total(const std::vector<Seg> &v) { CallLayout l; for (const Seg &s : v) l.add(s.name, s.elem, s.count, s.dbl); return l.bytes(); }
std::vector<Seg> marg_io(size_t nw, size_t nidx, size_t outd, size_t mass) {
  return {{"meta", META, nw, false}, {"idx", I, nidx, false}, {"out", D, outd, true}, {"mass", D, mass, true}};
}
std::vector<Seg> query_io(size_t n, bool win, bool pose, bool rest) {
  return {{"t_rel", 8, n, false}, {"win", I, win ? n : 0, false}, {"err", I, 4, false}, {"query_out", D, pose ? 7 * n : 0, true},
          {"query_out", D, rest ? 3 * n : 0, true}, {"query_out", D, rest ? 3 * n : 0, true}, {"query_out", D, rest ? 3 * n : 0, true}};
}
std::vector<Seg> cov_io(size_t nsel, size_t tiles, size_t wins, size_t ncov, size_t nvar) {
  return {{"sel", I, nsel, false}, {"tiles", TILE, tiles, false}, {"wins", CWIN, wins, false}, {"cov", D, ncov, true}, {"var_rho", D, nvar, true}};
}

// `tiny`: K 12, F 5, L 12, P 103, N 115 (state 127 doubles); `config1`: P 211, L 50, N 261
std::vector<Case> cases() {
  std::vector<Case> c;
  c.push_back({"head_only", {}, {}, {}, 1, 127});   // solve, cost, get_batch_state
  c.push_back({"head_241", {}, {}, {}, 241, 241 * 445});
  c.push_back({"linearize_tiny", {}, {{"Hpp", D, 103 * 103, false}, {"W", D, 16 * 104, false}, {"Hll", D, 12, false}, {"g", D, 115, false}}, {}, 1, 127});
  c.push_back({"linearize_cost_only", {}, {{"Hpp", D, 0, false}, {"W", D, 0, false}, {"Hll", D, 0, false}, {"g", D, 0, false}}, {}, 1, 127});
  c.push_back({"lm_step", {}, {{"delta", D, 115, false}}, {}, 7, 900});
  c.push_back({"residual_summary", {{"sums", D, 14 + 37, true}}, {}, {}, 1, 127});
  c.push_back({"gauge_two_windows", {{"ids_knot", I, 4, false}, {"q0_t0", D, 14, false}}, {}, {}, 3, 500});
  c.push_back({"query_none", query_io(0, false, false, false), {}, {}, 1, 127});
  c.push_back({"query_97_pose", query_io(97, false, true, false), {}, {}, 1, 127});
  c.push_back({"query_batch_5", query_io(5, true, true, true), {}, {}, 3, 500});
  c.push_back({"cov_tiny_20", cov_io(20, 2 + 1, 1, 400, 12), {}, {{"mask", 1, 115, false}, {"excl", 1, 115, false}, {"Y", D, 2 * 16 * 103, true}}, 1, 127});
  c.push_back({"cov_no_selection_var_rho", cov_io(0, 1, 0, 0, 12), {}, {{"mask", 1, 115, false}, {"excl", 1, 115, false}, {"Y", D, 0, true}}, 1, 127});
  c.push_back({"cov_nothing", cov_io(0, 0, 0, 0, 0), {}, {{"mask", 1, 115, false}, {"excl", 1, 115, false}, {"Y", D, 0, true}}, 1, 127});
  {   // two in-LDS windows, no blocked one; the second marginalises nothing (m = 0)
    Case k{"marg_no_blocked", marg_io(2, 115 + 40, 60 * 61 + 40 * 41, 0), {}, {}, 2, 254};
    marg_window(k.scr, 115, 55, 60); marg_window(k.scr, 115, 0, 40);
    k.scr.push_back({"mb", 1, 0, true}); k.scr.push_back({"rank", I, 0, false});
    c.push_back(k);
  }
  {   // only blocked windows (m 268 / n 553 and m 0 / n 70): the scratch of the larger one
    const size_t mb = std::max(total(mb_window(268, 553)), total(mb_window(0, 70)));
    c.push_back({"marg_only_blocked", marg_io(2, 821 + 70, 553 * 554 + 70 * 71, 2 * 576 / 32), {}, {{"mb", 1, mb, true}, {"rank", I, 553, false}}, 2, 3000});
  }
  {   // one in-LDS window and one blocked
    Case k{"marg_mixed", marg_io(2, 115 + 300, 60 * 61 + 200 * 201, 2 * 256 / 32), {}, {}, 2, 1000};
    marg_window(k.scr, 115, 55, 60);
    k.scr.push_back({"mb", 1, total(mb_window(100, 200)), true}); k.scr.push_back({"rank", I, 200, false});
    c.push_back(k);
  }
  c.push_back({"mb_window_268_553", {}, {}, mb_window(268, 553), 1, 127});
  c.push_back({"mb_window_m0", {}, {}, mb_window(0, 70), 1, 127});
  // the device-only scratch of the query entries, from the library's own CovScratch (not restated): 115 unknowns, records of 1184 bytes
  for (size_t n : {(size_t)0, (size_t)5})
    for (bool cov : {false, true}) {
      const ctv::CovScratch s(cov, 115, 1184, n);
      Case k{n ? (cov ? "query_scr_5_cov" : "query_scr_5") : (cov ? "query_scr_0_cov" : "query_scr_0"), {}, {}, {}, 1, 127};
      for (const ctv::ArenaSeg &g : s.lay.segs()) k.scr.push_back({g.name, 1, g.bytes, g.dbl});
      c.push_back(k);
    }
  return c;
}
const std::vector<Case> g_cases = cases();

CallLayout head_of(const Case &k) {
  CallLayout h;
  h.add("lm", sizeof(ctv::Lm), k.nw, false); h.add("poll", I, 4, false); h.add("state", D, k.state, false);
  return h;
}
// which 0: call_io_ (a copy of the head, the mirrored segments, the landing ones); 1: call_scr_
CallLayout build(const Case &k, int which) {
  if (which) { CallLayout l; for (const Seg &s : k.scr) l.add(s.name, s.elem, s.count, s.dbl); return l; }
  const CallLayout head = head_of(k);
  CallLayout l = head;
  for (const Seg &s : k.io) l.add(s.name, s.elem, s.count, s.dbl);
  if (!k.landing.empty()) l.landing();
  for (const Seg &s : k.landing) l.add(s.name, s.elem, s.count, s.dbl);
  return l;
}
// 0, or the first rule broken: 1 a pointer before the reservation; 2 no pointer after it; 3 growing after it; 4 the layout changed by the refused add
int refusals(const Case &k, int which) {
  CallLayout l = build(k, which);
  char base[1];
  const int n = (int)l.segs().size();
  for (int i = 0; i < n; ++i) if (l.at<char>(base, i) != nullptr) return 1;
  const size_t bytes = l.bytes();
  l.reserved();
  for (int i = 0; i < n; ++i) if (l.at<char>(base, i) != base + l.off(i)) return 2;
  if (l.at<char>(base, n) != nullptr || l.at<char>(base, -1) != nullptr) return 2;
  if (l.add("late", 8, 1, true) != -1) return 3;
  if (l.bytes() != bytes || (int)l.segs().size() != n) return 4;
  return 0;
}
// every segment filled through its typed pointer over real buffers of exactly the reserved sizes, then read back (an overlap, or an extent
// past the total, changes a neighbour or leaves the buffer)
int fill_and_read(const Case &k, int which) {
  CallLayout l = build(k, which);
  std::vector<char> dev(l.dev_bytes()), host(l.bytes());
  l.reserved();
  const int n = (int)l.segs().size();
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < n; ++i) {
      const ctv::ArenaSeg &s = l.segs()[(size_t)i];
      const bool on_dev = s.off + s.bytes <= l.dev_bytes();
      for (char *base : {host.data(), on_dev ? dev.data() : nullptr}) {
        if (!base || !s.bytes) continue;
        unsigned char *p = l.at<unsigned char>(base, i);
        for (size_t b = 0; b < s.bytes; ++b) { if (pass == 0) p[b] = (unsigned char)(i + 1); else if (p[b] != (unsigned char)(i + 1)) return i + 1; }
      }
    }
  return 0;
}
// QueryOrder over (only, n, win, nwin) cut at per_tile.  0, or the first rule broken: 1 slot is not the stable order by window; 2 a tile
// holds two windows; 3 a count outside [1, per_tile]; 4 the tiles do not partition [0, n) in order; 5 an error where none is due
int order_rules(int only, int n, const int32_t *win, int nwin, int per_tile) {
  const ctv::QueryOrder ord(only, n, win, nwin);
  if (!ord.error().empty()) return 5;
  if ((int)ord.slot.size() != n) return 1;
  std::vector<char> seen((size_t)n, 0);
  for (int r = 0; r < n; ++r) {
    const int i = ord.slot[(size_t)r];
    if (i < 0 || i >= n || seen[(size_t)i]++) return 1;
    if (ord.win_of(r) != (only >= 0 ? only : win[i])) return 1;
    if (r && (ord.win_of(r - 1) > ord.win_of(r) || (ord.win_of(r - 1) == ord.win_of(r) && ord.slot[(size_t)r - 1] > i))) return 1;
  }
  int next = 0, bad = 0;
  ord.runs(per_tile, [&](int w, int first, int cnt) {
    if (first != next && !bad) bad = 4;
    if ((cnt < 1 || cnt > per_tile || first + cnt > n) && !bad) bad = 3;
    for (int r = first; r < first + cnt && !bad; ++r) if (ord.win_of(r) != w) bad = 2;
    next = first + cnt;
  });
  return bad ? bad : (next == n ? 0 : 4);
}
const int32_t ORDER_WIN[11] = {2, 0, 2, 1, 2, 2, 2, 2, 2, 2, 2};
// the cases of the issue that added QueryOrder: no query, one, a single window without a window list, the mixed list at every per_tile in use
int order_cases() {
  const int32_t one[1] = {1};
  if (const int r = order_rules(-1, 0, nullptr, 3, 2)) return 10 + r;
  if (const int r = order_rules(-1, 1, one, 3, 8)) return 20 + r;
  if (const int r = order_rules(1, 5, nullptr, 3, 2)) return 30 + r;
  for (int per : {1, 2, 8})
    if (const int r = order_rules(-1, 11, ORDER_WIN, 3, per)) return 100 * per + r;
  const int32_t out[3] = {0, 3, -1};
  if (ctv::QueryOrder(-1, 3, out, 3).error() != "query 1: window id out of range") return 40;
  return 0;
}
// fill_not_ok / cov_block / merge_status / gate_value against the literal patterns at dim 2, 3, 6, 15.  0, or 100 dim + the rule broken
int fill_cases() {
  for (int dim : {2, 3, 6, 15}) {
    std::vector<double> o((size_t)dim * dim + 1), src((size_t)dim * dim, 7.0);
    for (int st : {1, 2, 3}) {
      std::fill(o.begin(), o.end(), -1.0);
      ctv::cov_block(o.data(), src.data(), dim, st);
      for (int i = 0; i < dim; ++i)
        for (int j = 0; j < dim; ++j) {
          const double v = o[(size_t)i * dim + j];
          if (st == 2 ? (i == j ? !(std::isinf(v) && v > 0) : v != 0.0) : !std::isnan(v)) return 100 * dim + st;
        }
      if (o.back() != -1.0) return 100 * dim + 4;   // nothing past the block
    }
    ctv::cov_block(o.data(), src.data(), dim, 0);
    for (int e = 0; e < dim * dim; ++e) if (o[(size_t)e] != 7.0) return 100 * dim + 5;
  }
  if (ctv::merge_status(0, true) != 1 || ctv::merge_status(0, false) != 0 || ctv::merge_status(2, true) != 2 || ctv::merge_status(3, true) != 3) return 6;
  if (ctv::gate_value(5.0, 0) != 5.0 || ctv::gate_value(5.0, 2) != 0.0 || !std::isnan(ctv::gate_value(5.0, 1)) || !std::isnan(ctv::gate_value(5.0, 3))) return 7;
  return 0;
}
}  // namespace

extern "C" {
int cl_order_cases() { return order_cases(); }
int cl_fill_cases() { return fill_cases(); }
// QueryOrder raw: slot[n]; the runs at per_tile as (window, first, count) triples in tile[3 cap]; returns the number of runs, -1 with an error
int cl_query_order(int only, int n, const int32_t *win, int nwin, int per_tile, int32_t *slot, int cap, int32_t *tile) {
  const ctv::QueryOrder ord(only, n, win, nwin);
  if (!ord.error().empty()) return -1;
  std::copy(ord.slot.begin(), ord.slot.end(), slot);
  int nt = 0;
  ord.runs(per_tile, [&](int w, int first, int cnt) { if (nt < cap) { tile[3 * nt] = w; tile[3 * nt + 1] = first; tile[3 * nt + 2] = cnt; } ++nt; });
  return nt;
}
void cl_fill_not_ok(double *o, int dim, int st) { ctv::fill_not_ok(o, dim, st); }
int cl_ncases() { return (int)g_cases.size(); }
const char *cl_case_name(int c) { return g_cases[(size_t)c].name; }
// the segments of case c in arena `which` (at most cap): names, offsets, bytes, flags; tot[0] the total, tot[1] the device's, tot[2] the head's segments
int cl_layout(int c, int which, int cap, const char **name, uint64_t *off, uint64_t *bytes, int32_t *dbl, uint64_t *tot) {
  const CallLayout l = build(g_cases[(size_t)c], which);
  const int n = std::min(cap, (int)l.segs().size());
  for (int i = 0; i < n; ++i) { const ctv::ArenaSeg &s = l.segs()[(size_t)i]; name[i] = s.name; off[i] = s.off; bytes[i] = s.bytes; dbl[i] = s.dbl ? 1 : 0; }
  tot[0] = l.bytes(); tot[1] = l.dev_bytes(); tot[2] = which ? 0 : 3;
  return (int)l.segs().size();
}
int cl_refusals(int c, int which) { return refusals(g_cases[(size_t)c], which); }
int cl_fill_and_read(int c, int which) { return fill_and_read(g_cases[(size_t)c], which); }
// the LDS of the tile Cholesky kernels for ntr tile rows (device_types.hpp: CholTilesLds, flow = 0; CholFlowLds, flow = 1): every segment's
// name, offset and the extent the kernel uses, in bytes; *total = the bytes a launch asks for
int cl_chol_lds(int flow, int ntr, const char **name, uint64_t *off, uint64_t *bytes, uint64_t *total) {
  const uint64_t ts = ctv::CHOL_TS, n = (uint64_t)ntr;
  int ns = 0;
  auto seg = [&](const char *nm, int off_d, uint64_t doubles) { name[ns] = nm; off[ns] = (uint64_t)off_d * D; bytes[ns] = doubles * D; ++ns; };
  if (flow) {
    const ctv::CholFlowLds l(ntr);
    seg("Id", l.Id, ts); seg("Li", l.Li, n * ts); seg("Ls", l.Ls, n * ts); seg("Pn", l.Pn, ctv::CholFlowLds::NPB * n * ts);
    seg("tv", l.tv, 16 * n); seg("xs", l.xs, 16 * n); seg("flags", l.flags, ctv::CholFlowLds::NFLAG / 2);
    *total = l.bytes;
  } else {
    const ctv::CholTilesLds l(ntr);
    seg("Id", l.Id, ts); seg("Li", l.Li, n * ts); seg("Pn", l.Pn, n * ts); seg("tv", l.tv, 16 * n); seg("xs", l.xs, 16 * n);
    seg("flags", l.flags, 1); seg("park", l.park, 12 * 64);
    *total = l.bytes;
  }
  return ns;
}
}

#ifdef CALL_LAYOUT_MAIN
int main() {
  for (int c = 0; c < cl_ncases(); ++c)
    for (int which = 0; which < 2; ++which) {
      const int r = cl_refusals(c, which), f = cl_fill_and_read(c, which);
      if (r || f) { std::printf("%s arena %d: refusal rule %d, segment %d\n", cl_case_name(c), which, r, f); return 1; }
    }
  if (const int r = order_cases()) { std::printf("query order: case / rule %d\n", r); return 1; }
  if (const int r = fill_cases()) { std::printf("status fill: dim / rule %d\n", r); return 1; }
  std::printf("CALL_LAYOUT_OK %d cases\n", cl_ncases());
  return 0;
}
#endif
