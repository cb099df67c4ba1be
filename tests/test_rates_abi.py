"""CPU: the body-rates entries are part of the C ABI (exported, listed in capi.SYMBOLS, with prototypes), and the adaptor's
GetBodyRatesCovariance and its demo compile with the host compiler alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <vector>
#include "ctvio_estimator.hpp"
bool rates_at(ctvio::TrajectoryEstimator &est, int64_t t_ns, const double *bias_gyr, const double *meas6, const double *noise6,
              std::vector<double> &rates, std::vector<double> &cov225, std::vector<double> &chi2) {
  return est.GetBodyRatesCovariance({t_ns}, nullptr, rates, cov225) && est.GetBodyRatesCovariance({t_ns}, bias_gyr, rates, cov225, meas6, noise6, &chi2);
}
int32_t (*const batch_entry)(ctvio_solver *, int64_t, const int32_t *, const int64_t *, const int32_t *, const double *, const double *, double *,
                             double *, double *, int32_t *) = &ctvio_body_rates_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, int32_t, const int64_t *, const int32_t *, const double *, const double *, double *,
                              double *, double *, int32_t *) = &ctvio_body_rates;
"""


def test_body_rates_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    for name in ("ctvio_body_rates_batch", "ctvio_body_rates"):
        assert name in cv.capi.SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.ctvio_body_rates_batch.argtypes) == 11 and len(lib.ctvio_body_rates.argtypes) == 11
    assert callable(cv.Solver.body_rates) and callable(cv.Solver.body_rates_batch)


def test_null_solver_is_refused_without_a_device(cv):
    """The null-handle check answers before anything touches a device."""
    cv.capi.build_library()
    lib = cv.capi.load_library()
    assert lib.ctvio_body_rates_batch(None, 0, None, None, None, None, None, None, None, None, None) == 1
    assert lib.ctvio_body_rates(None, 0, 0, None, None, None, None, None, None, None, None) == 1


def test_adaptor_body_rates_compiles_standalone(tmp_path):
    src = tmp_path / "rates_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "body_rates_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
