// Test shim (CPU): the walk of the order-fixed wide-window assembly (ctrl-vio_amd/csrc/host_pack.hpp: plan_row_walk, after plan_window and
// plan_sparsity) compiled with g++ against the HIP headers (no device code, nothing is launched), with the slot layout and the row order it
// is built from -- tests/test_row_walk_plan.py compares it with its Python mirror (packer.row_walk).
#define __HIP_PLATFORM_AMD__ 1
#include "../ctrl-vio_amd/csrc/host_pack.hpp"

// out: Vp, lord[Vp_cap], lm_pos[L], vrow[V], off[L + 1].  returns 0, 1 when the window is rejected (err_out gets the message), 2 when
// Vp > Vp_cap.
extern "C" int hw_row_walk(const ctvio_window *w, int Vp_cap, int32_t *Vp, int32_t *lord, int32_t *lm_pos, int32_t *vrow, int32_t *off,
                           char *err_out, int err_cap) {
  std::string err;
  if (!ctv::validate_window(w, err)) { std::snprintf(err_out, (size_t)err_cap, "%s", err.c_str()); return 1; }
  ctv::PackTmp t;
  ctv::plan_window(w, 8, t);
  if (!t.err.empty()) { std::snprintf(err_out, (size_t)err_cap, "%s", t.err.c_str()); return 1; }
  ctv::plan_sparsity(w, false, false, t);
  *Vp = t.Vp;
  if (t.Vp > Vp_cap) return 2;
  for (int s = 0; s < t.Vp; ++s) lord[s] = t.lord[s];
  for (int l = 0; l < w->L; ++l) lm_pos[l] = t.lm_pos[l];
  ctv::plan_row_walk(w, t, vrow, off);
  return 0;
}
