"""CPU: the visual-gate entries are part of the C ABI (declared, exported, listed in capi.SYMBOLS, with prototypes; ctvio_gate_options is
8 bytes on both sides, its default 0.01), the refusals that need no device, and the adaptor's GateVisualBlocks and the demo compile with the
host compiler alone."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <map>
#include "ctvio_estimator.hpp"
static_assert(sizeof(ctvio_gate_options) == 8, "ctvio_gate_options");
bool gate(ctvio::TrajectoryEstimator &est, ctvio::TrajectoryEstimator::VisualGate &blocks,
          std::map<const double *, ctvio::TrajectoryEstimator::LandmarkGate> &lms) {
  return est.GateVisualBlocks(blocks) && est.GateVisualBlocks(blocks, &lms, 0.02, false);
}
int32_t (*const batch_entry)(ctvio_solver *, const ctvio_gate_options *, double *, double *, double *, double *, double *, double *, int32_t *,
                             double *, int32_t *) = &ctvio_visual_gate_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, const ctvio_gate_options *, double *, double *, double *, double *, double *, double *,
                              int32_t *, double *, int32_t *) = &ctvio_visual_gate;
void (*const defaults)(ctvio_gate_options *) = &ctvio_default_gate_options;
"""


def test_visual_gate_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "ctvio.h")).read()
    for name in ("ctvio_visual_gate_batch", "ctvio_visual_gate"):
        assert name in cv.capi.SYMBOLS
        assert f"int32_t {name}(ctvio_solver *s" in hdr, name
        assert hasattr(lib, name), name
    assert "ctvio_default_gate_options" in cv.capi.SYMBOLS and hasattr(lib, "ctvio_default_gate_options")
    go = C.POINTER(cv.capi.GateOptions)
    assert lib.ctvio_visual_gate_batch.argtypes == [C.c_void_p, go] + [C.c_void_p] * 9
    assert lib.ctvio_visual_gate.argtypes == [C.c_void_p, C.c_int32, go] + [C.c_void_p] * 9
    assert C.sizeof(cv.capi.GateOptions) == 8
    assert "typedef struct ctvio_gate_options { double min_redundancy; } ctvio_gate_options;" in hdr
    o = cv.capi.GateOptions(-1.0)
    lib.ctvio_default_gate_options(C.byref(o))
    assert o.min_redundancy == 0.01
    lib.ctvio_default_gate_options(None)      # (a null pointer is ignored)
    assert callable(cv.Solver.visual_gate) and callable(cv.Solver.visual_gate_batch)


def test_null_solver_is_refused_without_a_device(cv):
    """The null-handle check answers before anything touches a device, whatever else is wrong with the call."""
    cv.capi.build_library()
    lib = cv.capi.load_library()
    o = cv.capi.GateOptions(0.01)
    none9 = [None] * 9
    assert lib.ctvio_visual_gate_batch(None, C.byref(o), *none9) == 1
    assert lib.ctvio_visual_gate_batch(None, None, *none9) == 1
    assert lib.ctvio_visual_gate(None, 0, C.byref(o), *none9) == 1
    assert lib.ctvio_visual_gate(None, -1, None, *none9) == 1
    assert lib.ctvio_visual_gate(None, 0, C.byref(cv.capi.GateOptions(float("nan"))), *none9) == 1


def test_adaptor_gate_visual_blocks_compiles_standalone(tmp_path):
    src = tmp_path / "visgate_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "visual_gate_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
