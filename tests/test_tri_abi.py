"""CPU: the triangulation and anchor-shift entries are part of the C ABI (exported, listed in capi.SYMBOLS, with prototypes), and a translation
unit that takes their addresses -- and the adaptor's TriangulateDepths -- compiles with the host compiler alone."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ctvio_default_triangulate_options", "ctvio_triangulate_batch", "ctvio_triangulate", "ctvio_shift_anchor_batch")

TU = """
#include <vector>
#include "ctvio_estimator.hpp"
void (*const defaults)(ctvio_triangulate_options *) = &ctvio_default_triangulate_options;
int32_t (*const batch_entry)(ctvio_solver *, const ctvio_triangulate_options *, double *, int32_t *) = &ctvio_triangulate_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, const ctvio_triangulate_options *, double *, int32_t *) = &ctvio_triangulate;
int32_t (*const shift_entry)(ctvio_solver *, const ctvio_triangulate_options *, int64_t, const int32_t *, const int32_t *, const int64_t *,
                             const int32_t *, double *, int32_t *) = &ctvio_shift_anchor_batch;
int new_depths(ctvio::TrajectoryEstimator &est, std::vector<int32_t> &flags) { return est.TriangulateDepths(true, true, &flags); }
static_assert(sizeof(ctvio_triangulate_options) == 32, "three int32, padding, two doubles");
"""


def test_triangulation_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    for name in NAMES:
        assert name in cv.capi.SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert callable(cv.Solver.triangulate_batch) and callable(cv.Solver.triangulate) and callable(cv.Solver.shift_anchor)
    assert C.sizeof(cv.capi.TriangulateOptions) == 32


def test_default_triangulate_options(cv):
    """The defaults are the reference's: row times on, only unset landmarks, applied, 0.1 (feature_manager.cpp:218) and INIT_DEPTH = 5."""
    o = cv.capi.TriangulateOptions()
    cv.capi.load_library().ctvio_default_triangulate_options(C.byref(o))
    assert (o.row_times, o.only_unset, o.apply, o.min_depth, o.init_depth) == (1, 1, 1, 0.1, 5.0)


def test_entries_compile_standalone(tmp_path):
    src = tmp_path / "tri_tu.cpp"
    src.write_text(TU)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
