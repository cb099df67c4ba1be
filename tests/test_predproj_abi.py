"""CPU: the landmark-prediction entries are part of the C ABI (declared, exported, listed in capi.SYMBOLS, with prototypes), the refusals that
need no device, and the adaptor's PredictLandmarks and its demo compile with the host compiler alone."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <vector>
#include "ctvio_estimator.hpp"
bool predict(ctvio::TrajectoryEstimator &est, const std::vector<ctvio::IMUData> &samples, const double *inv_depth, std::vector<double> &proj3,
             std::vector<double> &cov4, const std::vector<double> &obs2, std::vector<double> &chi2, std::vector<int32_t> &rows) {
  const ctvio_row_model rm = {460.0, 240.0, 480, 3};
  ctvio_imu_noise noise;
  ctvio_default_imu_noise(&noise);
  ctvio::IMUState end;
  return est.PredictLandmarks(samples, nullptr, noise, {{inv_depth, 240}}, proj3) &&
         est.PredictLandmarks(samples, nullptr, noise, {{inv_depth, 240}}, proj3, &cov4, &obs2, &chi2, &rm, &rows, nullptr, &end);
}
int32_t (*const batch_entry)(ctvio_solver *, int64_t, const int32_t *, const int32_t *, const int32_t *, const int64_t *, const double *, const double *,
                             const ctvio_imu_noise *, int64_t, const int32_t *, const int32_t *, const int32_t *, const ctvio_row_model *, const double *,
                             double *, double *, double *, double *, int32_t *, int32_t *) = &ctvio_predict_landmarks_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, int32_t, int32_t, const int64_t *, const double *, const double *, const ctvio_imu_noise *, int32_t,
                              const int32_t *, const int32_t *, const ctvio_row_model *, const double *, double *, double *, double *, double *, int32_t *,
                              int32_t *) = &ctvio_predict_landmarks;
"""


def test_prediction_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "ctvio.h")).read()
    for name in ("ctvio_predict_landmarks_batch", "ctvio_predict_landmarks"):
        assert name in cv.capi.SYMBOLS
        assert f"int32_t {name}(ctvio_solver *s" in hdr, name
        assert hasattr(lib, name), name
    rm, nz = C.POINTER(cv.capi.RowModel), C.POINTER(cv.capi.ImuNoise)
    assert lib.ctvio_predict_landmarks_batch.argtypes == [C.c_void_p, C.c_int64] + [C.c_void_p] * 6 + [nz, C.c_int64] + [C.c_void_p] * 3 + [rm] + [C.c_void_p] * 7
    assert lib.ctvio_predict_landmarks.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [nz, C.c_int32] + [C.c_void_p] * 2 + [rm] + [C.c_void_p] * 7
    assert callable(cv.Solver.predict_landmarks) and callable(cv.Solver.predict_landmarks_batch)


def test_null_solver_is_refused_without_a_device(cv):
    """The null-handle check answers before anything touches a device."""
    cv.capi.build_library()
    lib = cv.capi.load_library()
    assert lib.ctvio_predict_landmarks_batch(None, 0, None, None, None, None, None, None, None, 0, *([None] * 11)) == 1
    assert lib.ctvio_predict_landmarks_batch(None, 1, None, None, None, None, None, None, None, 1, *([None] * 11)) == 1
    assert lib.ctvio_predict_landmarks(None, 0, -1, 1, None, None, None, None, 0, *([None] * 10)) == 1
    assert lib.ctvio_predict_landmarks(None, -1, 0, 1, None, None, None, None, 1, *([None] * 10)) == 1


def test_adaptor_predict_landmarks_compiles_standalone(tmp_path):
    src = tmp_path / "prediction_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "predict_landmarks_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
