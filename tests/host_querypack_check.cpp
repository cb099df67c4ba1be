// Test program (CPU): the helpers the query entries share on the host (ctrl-vio_amd/csrc/host_pack.hpp: ImuSamples, check_frame, check_count,
// gate_scatter) compiled with g++ against the HIP headers (no device code, nothing is launched).
//   ImuSamples   2 queries of 1 and 3 samples: the accepted streams give first = {0, 1, 4}, three io segments of 4, 12 and 12 elements
//                behind a segment of the call's own, and stage() copies the streams there; one rejected call per error string, with the
//                prefix "query" or "prediction", and two faults in one call report the first one in the order of detection.  The cap of
//                2^30 samples needs 8 GiB of them and is not run.
//   gate_scatter every status 0 .. 4 x bad against the table written out below (not derived from the function), for the 2 x 2 and the
//                6 x 6 block; null outputs read no computed value.
// tests/test_querypack_host.py runs it plainly and under -fsanitize=address,undefined.
#define __HIP_PLATFORM_AMD__ 1
#include "../ctrl-vio_amd/csrc/host_pack.hpp"

#include <cstdio>

using namespace ctv;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

struct Streams {
  int32_t win[2] = {1, 0}, frame[2] = {0, 2}, n_imu[2] = {1, 3};
  int64_t t[4] = {100, 100, 105, 112};   // (query 1 may start where query 0 ends: only a query's own times increase)
  double gyro[12], acc[12];
  WinMeta meta[2];
  ctvio_imu_noise nz{4e-3, 8e-2, 2e-6, 4e-5};
  Streams() {
    for (int i = 0; i < 12; ++i) { gyro[i] = 0.01 * i; acc[i] = 9.0 - 0.1 * i; }
    std::memset(meta, 0, sizeof(meta));
    meta[0].F = 3; meta[1].F = 1;
  }
  bool run(ImuSamples &s, const char *what, int only = -1, bool with_frame = true) {
    return s.noise(nz) && s.streams(what, only, 2, win, with_frame ? frame : nullptr, meta, n_imu, t, gyro, acc);
  }
};

static void rejected(Streams &in, const char *what, const char *want) {
  ImuSamples s;
  const bool ok = in.run(s, what);
  if (ok || s.error != want) { std::printf("want \"%s\", got %s \"%s\"\n", want, ok ? "accepted" : "rejected", s.error.c_str()); ++fails; }
}

static void imu_samples() {
  {   // accepted: the prefix sums, the segments, the staged copy
    Streams in;
    ImuSamples s;
    CHECK(in.run(s, "query") && s.error.empty());
    CHECK(s.first == (std::vector<int64_t>{0, 1, 4}) && s.ns == 4);
    CallLayout io;
    const int s_head = io.add("own", sizeof(double), 5, true);
    s.add(io);
    const int s_tail = io.add("tail", 1, 1, false);
    CHECK(s.s_t == s_head + 1 && s.s_gyro == s_head + 2 && s.s_acc == s_head + 3 && s_tail == s_head + 4);
    CHECK(io.segs()[(size_t)s.s_t].bytes == 32 && io.segs()[(size_t)s.s_gyro].bytes == 96 && io.segs()[(size_t)s.s_acc].bytes == 96);
    io.reserved();
    std::vector<char> host(io.bytes(), 0);
    s.stage(io, host.data());
    CHECK(std::memcmp(io.at<int64_t>(host.data(), s.s_t), in.t, sizeof(in.t)) == 0);
    CHECK(std::memcmp(io.at<double>(host.data(), s.s_gyro), in.gyro, sizeof(in.gyro)) == 0);
    CHECK(std::memcmp(io.at<double>(host.data(), s.s_acc), in.acc, sizeof(in.acc)) == 0);
    CHECK(*io.at<char>(host.data(), s_tail) == 0);
    ImuSamples one, newest;   // every query of window 0 (win is not read); frame null: the newest state is always there
    CHECK(in.run(one, "prediction", 0) && one.first == s.first);
    in.meta[0].F = 1;
    CHECK(in.run(newest, "query", -1, false));
  }
  const double inf = std::numeric_limits<double>::infinity();
  { Streams in; in.nz.acc_w = -1e-9; rejected(in, "query", "a noise sigma is negative or not finite"); }
  { Streams in; in.nz.gyr_n = inf; rejected(in, "prediction", "a noise sigma is negative or not finite"); }
  { Streams in; in.frame[1] = 3; rejected(in, "query", "query 1: bias state out of range"); }
  { Streams in; in.frame[0] = -1; rejected(in, "prediction", "prediction 0: bias state out of range"); }
  { Streams in; in.n_imu[0] = 0; rejected(in, "query", "query 0: 1 to 4096 samples"); }
  { Streams in; in.n_imu[1] = 4097; rejected(in, "prediction", "prediction 1: 1 to 4096 samples"); }
  { Streams in; in.t[3] = in.t[2]; rejected(in, "query", "query 1: sample times not strictly increasing"); }
  { Streams in; in.acc[11] = std::nan(""); rejected(in, "query", "query 1: a measurement is not finite"); }
  { Streams in; in.gyro[0] = inf; rejected(in, "prediction", "prediction 0: a measurement is not finite"); }
  // the order of detection: the sigmas before any stream, query 0 before query 1, a query's bias state before its samples
  { Streams in; in.nz.gyr_w = -1.0; in.frame[0] = 9; rejected(in, "query", "a noise sigma is negative or not finite"); }
  { Streams in; in.gyro[1] = inf; in.frame[1] = 9; rejected(in, "query", "query 0: a measurement is not finite"); }
  { Streams in; in.frame[1] = 9; in.n_imu[1] = 0; rejected(in, "query", "query 1: bias state out of range"); }
  { Streams in; in.t[2] = 90; in.acc[3] = inf; rejected(in, "query", "query 1: a measurement is not finite"); }   // (sample 1 is looked at before the times of sample 2)
  std::string err;
  const int32_t fr[2] = {0, 4};
  CHECK(check_frame(nullptr, 1, 1, "query", err) && check_frame(fr, 0, 1, "query", err) && err.empty());
  CHECK(!check_frame(fr, 1, 4, "query", err) && err == "query 1: bias state out of range");
  CHECK(!check_count(-1) && check_count(0) && check_count((int64_t)1 << 30) && !check_count(((int64_t)1 << 30) + 1));
}

// The table of the two gates' scatter loops.  Status the kernels left x bad (the window's factorisation failed) -> the status reported;
// by the status reported: redundancy, block, gate.  C: the computed value, Z: zero, I: +inf on the diagonal and zero elsewhere, N: NaN.
struct Row { int st; bool bad; int want; char red, cov, chi2; };
static const Row TABLE[] = {
    {0, false, 0, 'C', 'C', 'C'}, {0, true, 1, 'N', 'N', 'N'},   // ok; a failed window: singular
    {1, false, 1, 'N', 'N', 'N'}, {1, true, 1, 'N', 'N', 'N'},   // (singular is the host's; it stands if it ever arrives)
    {2, false, 2, 'Z', 'I', 'Z'}, {2, true, 2, 'Z', 'I', 'Z'},   // no information stands
    {3, false, 3, 'N', 'N', 'N'}, {3, true, 3, 'N', 'N', 'N'},   // not computable stands
    {4, false, 4, 'C', 'I', 'Z'}, {4, true, 1, 'N', 'N', 'N'},   // weak: the redundancy is reported, block and gate as without information
};

static bool is(char kind, double got, double computed, bool diagonal) {
  switch (kind) {
    case 'C': return got == computed;
    case 'Z': return got == 0.0;
    case 'I': return diagonal ? got == std::numeric_limits<double>::infinity() : got == 0.0;
    default: return std::isnan(got);
  }
}

static void gate_table() {
  const GateCodes codes{0, 4, 1, 2};
  for (const int dim : {2, 6}) {
    std::vector<double> computed((size_t)dim * dim), out((size_t)dim * dim);
    for (size_t e = 0; e < computed.size(); ++e) computed[e] = 1.5 + (double)e;
    for (const Row &r : TABLE) {
      const double cred = 0.75, cchi = 3.25;
      double red = -7.0, chi2 = -7.0;
      std::fill(out.begin(), out.end(), -7.0);
      const int st = gate_scatter(codes, r.st, r.bad, dim, &cred, computed.data(), &cchi, &red, out.data(), &chi2);
      bool ok = st == r.want && is(r.red, red, cred, false) && is(r.chi2, chi2, cchi, false);
      for (int e = 0; e < dim * dim; ++e) ok = ok && is(r.cov, out[(size_t)e], computed[(size_t)e], e % (dim + 1) == 0);
      if (!ok) { std::printf("gate_scatter: status %d bad %d dim %d: got status %d red %g chi2 %g cov[0] %g cov[1] %g\n", r.st, (int)r.bad, dim, st, red, chi2, out[0], out[1]); ++fails; }
      CHECK(gate_scatter(codes, r.st, r.bad, dim, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == r.want);   // values only: nothing is read
    }
  }
}

int main() {
  imu_samples();
  gate_table();
  if (fails) return 1;
  std::printf("QUERYPACK_OK\n");
  return 0;
}
