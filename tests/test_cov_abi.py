"""CPU: the covariance entries are part of the C ABI (exported, listed in capi.SYMBOLS, with prototypes), and the adaptor's
GetCovarianceInTangentSpace compiles with the host compiler alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <vector>
#include "ctvio_estimator.hpp"
bool covariance_of_last_knot(ctvio::Trajectory &traj, ctvio::TrajectoryEstimator &est, double *bg, double *ba, std::vector<double> &cov) {
  const size_t k = traj.numKnots() - 2;
  const std::vector<const double *> blocks = {traj.getKnotSO3(k).data(), traj.getKnotPos(k).data(), bg, ba, &traj.line_delay};
  return est.GetCovarianceInTangentSpace(blocks, cov);
}
int32_t (*const batch_entry)(ctvio_solver *, const int32_t *, const int32_t *, double *, double *, int32_t *) = &ctvio_covariance_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, int32_t, const int32_t *, double *, double *, int32_t *) = &ctvio_covariance;
"""


def test_covariance_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    for name in ("ctvio_covariance_batch", "ctvio_covariance"):
        assert name in cv.capi.SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert callable(cv.Solver.covariance) and callable(cv.Solver.covariance_batch)


def test_adaptor_covariance_compiles_standalone(tmp_path):
    src = tmp_path / "cov_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "covariance_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
