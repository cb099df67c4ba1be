"""CPU: the pose-covariance entries are part of the C ABI (exported, listed in capi.SYMBOLS, with prototypes), and the adaptor's
GetPoseCovariance compiles with the host compiler alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <vector>
#include "ctvio_estimator.hpp"
bool pose_covariance_at(ctvio::Trajectory &traj, ctvio::TrajectoryEstimator &est, int64_t t_ns, std::vector<double> &body, std::vector<double> &cam) {
  return est.GetPoseCovariance({t_ns}, body) && est.GetPoseCovariance({t_ns}, cam, traj.q_CI, traj.p_CI);
}
int32_t (*const batch_entry)(ctvio_solver *, int64_t, const int32_t *, const int64_t *, const double *, const double *, double *, int32_t *) =
    &ctvio_pose_covariance_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, int32_t, const int64_t *, const double *, const double *, double *, int32_t *) =
    &ctvio_pose_covariance;
"""


def test_pose_covariance_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    for name in ("ctvio_pose_covariance_batch", "ctvio_pose_covariance"):
        assert name in cv.capi.SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert callable(cv.Solver.pose_covariance) and callable(cv.Solver.pose_covariance_batch)


def test_null_solver_is_refused_without_a_device(cv):
    """The null-handle check answers before anything touches a device."""
    cv.capi.build_library()
    lib = cv.capi.load_library()
    assert lib.ctvio_pose_covariance_batch(None, 0, None, None, None, None, None, None) == 1
    assert lib.ctvio_pose_covariance(None, 0, 0, None, None, None, None, None) == 1


def test_adaptor_pose_covariance_compiles_standalone(tmp_path):
    src = tmp_path / "posecov_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "pose_covariance_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
