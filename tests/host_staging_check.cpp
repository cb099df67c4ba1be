// Test shim (CPU): the host-only steps of a batch upload (ctrl-vio_amd/csrc/host_pack.hpp: plan, offsets, input-arena layout, fill) compiled
// with g++ against the HIP headers (no device code, nothing is launched), in the order SolverImpl::pack_and_upload runs them.  The batch is
// packed over 0x00 and over 0xFF into a plain buffer; tests/test_host_staging.py checks that every segment's filled extent agrees.
#define __HIP_PLATFORM_AMD__ 1
#include "../ctrl-vio_amd/csrc/host_pack.hpp"

extern "C" {
int hs_nseg() { return ctv::INPUT_NSEG; }
// n windows as the caller hands them over.  deterministic2: ctvio_options.deterministic == 2 (a batch with a window beyond the LDS-resident
// Hessian then uploads the row walk); dense: CTVIO_DENSE; vis_stage: kernels_assemble.hpp's vis_stage_bytes(8, 8).  out (hs_nseg() entries each):
// the segments' names, offsets, filled bytes and FNV-1a hashes of the filled extents; *walk: the row walk was packed.
// returns 0; 1 when a window is rejected; 2 when a staged byte is not written by the packer (err_out gets the message).
int hs_pack(int n, const ctvio_window *wins, int deterministic2, int dense, uint64_t vis_stage, int threads, const char **name, uint64_t *off,
            uint64_t *bytes, uint64_t *hash, int32_t *walk, char *err_out, int err_cap) {
  auto fail = [&](int rc, const std::string &m) { std::snprintf(err_out, (size_t)err_cap, "%s", m.c_str()); return rc; };
  std::vector<const ctvio_window *> ptr((size_t)n);
  std::vector<ctv::PackTmp> tmp((size_t)n);
  int maxP = 0;
  for (int i = 0; i < n; ++i) { ptr[i] = wins + i; maxP = std::max(maxP, 6 * wins[i].K + 6 * wins[i].F + 1); }
  const bool dense_env = maxP <= 223 || dense;   // (the register-resident tile Cholesky keeps the whole triangle)
  for (int i = 0; i < n; ++i) {
    if (!ctv::validate_window(ptr[i], tmp[i].err)) return fail(1, tmp[i].err);
    ctv::plan_window(ptr[i], 8, tmp[i]);
    if (tmp[i].err.empty()) ctv::plan_sparsity(ptr[i], dense_env, dense != 0, tmp[i]);
    if (!tmp[i].err.empty()) return fail(1, tmp[i].err);
  }
  std::vector<ctv::WinMeta> meta;
  std::vector<int64_t> t0;
  const ctv::BatchFacts b = ctv::batch_offsets(ptr, tmp, false, (size_t)vis_stage, deterministic2 != 0, meta, t0);
  const ctv::InputLayout lay = ctv::layout_input(b);
  std::vector<char> buf(lay.bytes);
  ctv::WorkerPool pool;
  const std::string err = ctv::check_staging(lay, buf.data(), [&] { ctv::pack_input(ptr, tmp, meta, b, lay, buf.data(), 8, pool, threads); });
  *walk = b.walk ? 1 : 0;
  for (int i = 0; i < ctv::INPUT_NSEG; ++i) {
    const ctv::ArenaSeg &sg = lay.segs[i];
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < sg.bytes; ++k) h = (h ^ (unsigned char)buf[sg.off + k]) * 1099511628211ull;
    name[i] = sg.name; off[i] = sg.off; bytes[i] = sg.bytes; hash[i] = h;
  }
  return err.empty() ? 0 : fail(2, err);
}
}
