"""CPU: the landmark-point entries are part of the C ABI (declared in include/ctvio.h, exported, listed in capi.SYMBOLS, with prototypes of
matching argument counts), and the adaptor's GetLandmarkPoints compiles with the host compiler alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <vector>
#include "ctvio_estimator.hpp"
bool cloud_of(ctvio::TrajectoryEstimator &est, std::vector<double> &points, std::vector<double> &cov, std::vector<int32_t> &status) {
  return est.GetLandmarkPoints(points) && est.GetLandmarkPoints(points, &cov) && est.GetLandmarkPoints(points, &cov, &status);
}
int32_t (*const batch_entry)(ctvio_solver *, double *, double *, int32_t *) = &ctvio_landmark_points_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, double *, double *, int32_t *) = &ctvio_landmark_points;
"""

NAMES = ("ctvio_landmark_points_batch", "ctvio_landmark_points")


def test_landmark_points_symbols_declared_and_exported(cv):
    hdr = open(os.path.join(ROOT, "include", "ctvio.h")).read()
    cv.capi.build_library()
    lib = cv.capi.load_library()
    for name in NAMES:
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/ctvio.h"
        assert name in cv.capi.SYMBOLS
        assert hasattr(lib, name), name
        argtypes = getattr(lib, name).argtypes
        assert argtypes is not None and len(argtypes) == len(m.group(1).split(",")), name
    assert callable(cv.Solver.landmark_points) and callable(cv.Solver.landmark_points_batch)


def test_null_solver_is_refused_without_a_device(cv):
    """The null-handle check answers before anything touches a device."""
    cv.capi.build_library()
    lib = cv.capi.load_library()
    assert lib.ctvio_landmark_points_batch(None, None, None, None) == 1
    assert lib.ctvio_landmark_points(None, 0, None, None, None) == 1


def test_adaptor_landmark_points_compiles_standalone(tmp_path):
    src = tmp_path / "lmpoint_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "landmark_points_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
