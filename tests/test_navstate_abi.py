"""CPU: the navigation-state entries are part of the C ABI (exported, listed in capi.SYMBOLS, with prototypes), and the adaptor's
GetIMUStateCovariance compiles with the host compiler alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <vector>
#include "ctvio_estimator.hpp"
bool nav_state_at(ctvio::TrajectoryEstimator &est, int64_t t_ns, const double *bias_gyr, std::vector<ctvio::IMUState> &states,
                  std::vector<double> &bias6, std::vector<double> &cov225) {
  return est.GetIMUStateCovariance({t_ns}, nullptr, states, bias6, cov225) && est.GetIMUStateCovariance({t_ns}, bias_gyr, states, bias6, cov225);
}
int32_t (*const batch_entry)(ctvio_solver *, int64_t, const int32_t *, const int64_t *, const int32_t *, double *, double *, int32_t *) =
    &ctvio_nav_state_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, int32_t, const int64_t *, const int32_t *, double *, double *, int32_t *) = &ctvio_nav_state;
"""


def test_nav_state_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    for name in ("ctvio_nav_state_batch", "ctvio_nav_state"):
        assert name in cv.capi.SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert callable(cv.Solver.nav_state) and callable(cv.Solver.nav_state_batch)


def test_null_solver_is_refused_without_a_device(cv):
    """The null-handle check answers before anything touches a device."""
    cv.capi.build_library()
    lib = cv.capi.load_library()
    assert lib.ctvio_nav_state_batch(None, 0, None, None, None, None, None, None) == 1
    assert lib.ctvio_nav_state(None, 0, 0, None, None, None, None, None) == 1


def test_adaptor_nav_state_compiles_standalone(tmp_path):
    src = tmp_path / "navstate_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "nav_state_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
