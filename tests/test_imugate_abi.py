"""CPU: the IMU-gate entries are part of the C ABI (declared, exported, listed in capi.SYMBOLS, with prototypes), the refusals that need no
device, and the adaptor's GateIMUSamples and the demo compile with the host compiler alone."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <map>
#include "ctvio_estimator.hpp"
bool gate(ctvio::TrajectoryEstimator &est, ctvio::TrajectoryEstimator::IMUGate &samples,
          std::map<const double *, ctvio::TrajectoryEstimator::FrameGate> &frames) {
  return est.GateIMUSamples(samples) && est.GateIMUSamples(samples, &frames, 0.02, true);
}
int32_t (*const batch_entry)(ctvio_solver *, const ctvio_gate_options *, double *, double *, double *, double *, int32_t *, double *) =
    &ctvio_imu_gate_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, const ctvio_gate_options *, double *, double *, double *, double *, int32_t *, double *) =
    &ctvio_imu_gate;
"""


def test_imu_gate_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "ctvio.h")).read()
    for name in ("ctvio_imu_gate_batch", "ctvio_imu_gate"):
        assert name in cv.capi.SYMBOLS
        assert f"int32_t {name}(ctvio_solver *s" in hdr, name
        assert hasattr(lib, name), name
    go = C.POINTER(cv.capi.GateOptions)
    assert lib.ctvio_imu_gate_batch.argtypes == [C.c_void_p, go] + [C.c_void_p] * 6
    assert lib.ctvio_imu_gate.argtypes == [C.c_void_p, C.c_int32, go] + [C.c_void_p] * 6
    assert callable(cv.Solver.imu_gate) and callable(cv.Solver.imu_gate_batch)
    assert "CTVIO_GATE_SLICE=n" in hdr and "ctvio_imu_gate_batch in slices of at most n IMU samples" in hdr


def test_null_solver_is_refused_without_a_device(cv):
    """The null-handle check answers before anything touches a device, whatever else is wrong with the call."""
    cv.capi.build_library()
    lib = cv.capi.load_library()
    o = cv.capi.GateOptions(0.01)
    none6 = [None] * 6
    assert lib.ctvio_imu_gate_batch(None, C.byref(o), *none6) == 1
    assert lib.ctvio_imu_gate_batch(None, None, *none6) == 1
    assert lib.ctvio_imu_gate(None, 0, C.byref(o), *none6) == 1
    assert lib.ctvio_imu_gate(None, -1, None, *none6) == 1
    assert lib.ctvio_imu_gate(None, 0, C.byref(cv.capi.GateOptions(float("nan"))), *none6) == 1


def test_adaptor_gate_imu_samples_compiles_standalone(tmp_path):
    src = tmp_path / "imugate_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "imu_gate_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
