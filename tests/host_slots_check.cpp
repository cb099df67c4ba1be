// Test shim (CPU): the LDS slots of the panel Cholesky's slot-indexed variant (ctrl-vio_amd/csrc/host_pack.hpp: chol_panel_slots),
// compiled with g++ against the HIP headers (no device code), so that tests/test_chol_compact_model.py can hold it equal to the
// Python mirror (packer.chol_panel_slots).
#define __HIP_PLATFORM_AMD__ 1
#include "../ctrl-vio_amd/csrc/host_pack.hpp"

extern "C" {
int hs_chol_slots(const int32_t *env_first, int P) { return ctv::chol_panel_slots(env_first, P); }
}
