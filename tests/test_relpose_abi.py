"""CPU: the relative-pose entries are part of the C ABI (declared, exported, listed in capi.SYMBOLS, with prototypes), the refusals that need
no device, and the adaptor's GetRelativePoseCovariance compiles with the host compiler alone."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <utility>
#include <vector>
#include "ctvio_estimator.hpp"
bool between(ctvio::TrajectoryEstimator &est, const ctvio::Trajectory &traj, int64_t t_a, int64_t t_b, std::vector<double> &rel, std::vector<double> &cov36) {
  return est.GetRelativePoseCovariance({{t_a, t_b}}, rel, cov36) && est.GetRelativePoseCovariance({{t_a, t_b}}, rel, cov36, traj.q_CI, traj.p_CI);
}
int32_t (*const batch_entry)(ctvio_solver *, int64_t, const int32_t *, const int64_t *, const int64_t *, const double *, const double *, double *,
                             double *, int32_t *) = &ctvio_relative_pose_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, int32_t, const int64_t *, const int64_t *, const double *, const double *, double *, double *,
                              int32_t *) = &ctvio_relative_pose;
"""


def test_relative_pose_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "ctvio.h")).read()
    for name in ("ctvio_relative_pose_batch", "ctvio_relative_pose"):
        assert name in cv.capi.SYMBOLS
        assert f"int32_t {name}(ctvio_solver *s" in hdr, name
        assert hasattr(lib, name), name
    assert lib.ctvio_relative_pose_batch.argtypes == [C.c_void_p, C.c_int64] + [C.c_void_p] * 8
    assert lib.ctvio_relative_pose.argtypes == [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 7
    assert callable(cv.Solver.relative_pose) and callable(cv.Solver.relative_pose_batch)


def test_null_solver_is_refused_without_a_device(cv):
    """The null-handle check answers before anything touches a device."""
    cv.capi.build_library()
    lib = cv.capi.load_library()
    assert lib.ctvio_relative_pose_batch(None, 0, None, None, None, None, None, None, None, None) == 1
    assert lib.ctvio_relative_pose(None, 0, 0, None, None, None, None, None, None, None) == 1
    assert lib.ctvio_relative_pose(None, -1, 1, None, None, None, None, None, None, None) == 1


def test_adaptor_relative_pose_compiles_standalone(tmp_path):
    src = tmp_path / "relpose_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "relative_pose_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
