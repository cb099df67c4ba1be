"""CPU: the IMU-prediction entries are part of the C ABI (exported, listed in capi.SYMBOLS, with prototypes), a null handle is refused before
anything touches a device, and the adaptor's PredictIMUStates compiles with the host compiler alone."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = """
#include <vector>
#include "ctvio_estimator.hpp"
bool predict(ctvio::TrajectoryEstimator &est, const std::vector<ctvio::IMUData> &samples, const double *bias_gyr, std::vector<ctvio::IMUState> &states,
             std::vector<double> &cov225) {
  ctvio_imu_noise noise;
  ctvio_default_imu_noise(&noise);
  return est.PredictIMUStates(samples, nullptr, noise, states, cov225) && est.PredictIMUStates(samples, bias_gyr, noise, states, cov225);
}
int32_t (*const batch_entry)(ctvio_solver *, int64_t, const int32_t *, const int32_t *, const int32_t *, const int64_t *, const double *, const double *,
                             const ctvio_imu_noise *, int32_t, double *, double *, int32_t *) = &ctvio_imu_predict_batch;
int32_t (*const single_entry)(ctvio_solver *, int32_t, int32_t, int32_t, const int64_t *, const double *, const double *, const ctvio_imu_noise *, int32_t,
                              double *, double *, int32_t *) = &ctvio_imu_predict;
"""


def test_imu_predict_symbols_exported(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    for name in ("ctvio_default_imu_noise", "ctvio_imu_predict_batch", "ctvio_imu_predict"):
        assert name in cv.capi.SYMBOLS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert callable(cv.Solver.imu_predict) and callable(cv.Solver.imu_predict_batch)
    nz = cv.capi.ImuNoise()
    lib.ctvio_default_imu_noise(C.byref(nz))
    assert (nz.gyr_n, nz.acc_n, nz.gyr_w, nz.acc_w) == (4.0e-3, 8.0e-2, 2.0e-6, 4.0e-5)
    assert C.sizeof(cv.capi.ImuNoise) == 32
    lib.ctvio_default_imu_noise(None)


def test_null_solver_is_refused_without_a_device(cv):
    """The null-handle check answers before anything touches a device."""
    cv.capi.build_library()
    lib = cv.capi.load_library()
    assert lib.ctvio_imu_predict_batch(None, 0, None, None, None, None, None, None, None, 0, None, None, None) == 1
    assert lib.ctvio_imu_predict(None, 0, -1, 1, None, None, None, None, 0, None, None, None) == 1


def test_adaptor_predict_compiles_standalone(tmp_path):
    src = tmp_path / "imupredict_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "imu_predict_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
