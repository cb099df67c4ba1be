"""CPU: the landmark-projection entries are part of the C ABI (declared, exported, listed in capi.SYMBOLS, with prototypes; ctvio_row_model is
24 bytes on both sides), the refusals that need no device, and the adaptor's ProjectLandmarks compiles with the host compiler alone."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <vector>
#include "ctvio_estimator.hpp"
static_assert(sizeof(ctvio_row_model) == 24, "ctvio_row_model");
bool predict(ctvio::TrajectoryEstimator &est, const double *inv_depth, int64_t t, std::vector<double> &proj3, std::vector<double> &cov4,
             const std::vector<double> &obs2, std::vector<double> &chi2, std::vector<int32_t> &rows) {
  const ctvio_row_model rm = {460.0, 240.0, 480, 3};
  return est.ProjectLandmarks({{inv_depth, t, 240}}, proj3) && est.ProjectLandmarks({{inv_depth, t, 240}}, proj3, &cov4, &obs2, &chi2, &rm, &rows);
}
int32_t (*const batch_entry)(ctvio_solver *, int64_t, const int32_t *, const int32_t *, const int64_t *, const int32_t *, const ctvio_row_model *,
                             const double *, double *, double *, double *, int32_t *, int32_t *) = &ctvio_project_landmarks_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, int32_t, const int32_t *, const int64_t *, const int32_t *, const ctvio_row_model *,
                              const double *, double *, double *, double *, int32_t *, int32_t *) = &ctvio_project_landmarks;
"""


def test_projection_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "ctvio.h")).read()
    for name in ("ctvio_project_landmarks_batch", "ctvio_project_landmarks"):
        assert name in cv.capi.SYMBOLS
        assert f"int32_t {name}(ctvio_solver *s" in hdr, name
        assert hasattr(lib, name), name
    rm = C.POINTER(cv.capi.RowModel)
    assert lib.ctvio_project_landmarks_batch.argtypes == [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [rm] + [C.c_void_p] * 6
    assert lib.ctvio_project_landmarks.argtypes == [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [rm] + [C.c_void_p] * 6
    assert C.sizeof(cv.capi.RowModel) == 24
    assert "typedef struct ctvio_row_model { double fy, cy; int32_t rows, iterations; } ctvio_row_model;" in hdr
    assert callable(cv.Solver.project_landmarks) and callable(cv.Solver.project_landmarks_batch)


def test_null_solver_is_refused_without_a_device(cv):
    """The null-handle check answers before anything touches a device."""
    cv.capi.build_library()
    lib = cv.capi.load_library()
    assert lib.ctvio_project_landmarks_batch(None, 0, None, None, None, None, None, None, None, None, None, None, None) == 1
    assert lib.ctvio_project_landmarks(None, 0, 0, None, None, None, None, None, None, None, None, None, None) == 1
    assert lib.ctvio_project_landmarks(None, -1, 1, None, None, None, None, None, None, None, None, None, None) == 1


def test_adaptor_project_landmarks_compiles_standalone(tmp_path):
    src = tmp_path / "projection_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "project_landmarks_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
