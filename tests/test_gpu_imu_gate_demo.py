"""GPU (-m gpu): tests/imu_gate_demo.cpp through the C++ adaptor (include/ctvio_estimator.hpp: GateIMUSamples).  The demo raises the gyro x
reading of one IMU sample by 0.04 rad/s (10 sigma at imu_w = 250), solves the window with it and runs the leave-one-out test: that sample
has the largest chi2 of its window, beyond the 99 % point of chi-square with 6 degrees of freedom (the demo's own exit status), and its bias
state reports it; per-factor results come in the order of the AddIMUMeasurementAnalytic calls, per-frame results keyed by the gyro-bias
pointer."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_corrupted_sample_has_the_largest_chi2(cv, tmp_path):
    import query_harness as qh
    exe = qh.build_demo("imu_gate_demo", tmp_path)
    w0 = cv.synth.make_window("config1", seed=1003)
    M, F, bad = w0.M, w0.F, 250
    assert M == 500 and abs(w0.imu_w[0] - 250.0) < 1e-9
    qh._dump(w0, str(tmp_path / "in.txt"))
    p = subprocess.run([exe, str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), "15", str(bad), "0.04"], capture_output=True, text=True, timeout=120)
    print(p.stdout[-400:])
    assert p.returncode == 0, (p.returncode, p.stdout[-400:], p.stderr[-2000:])
    arr = np.array(open(tmp_path / "out.txt").read().split(), float)
    assert arr[1] == M
    chi2 = arr[2:2 + M]; status = arr[2 + M:2 + 2 * M]; res = arr[2 + 2 * M:2 + 8 * M].reshape(M, 6)
    rest = arr[2 + 8 * M:]
    assert rest[0] == F
    fs = rest[1:1 + 4 * F].reshape(F, 4)
    rest = rest[1 + 4 * F:]
    assert rest[1] == M
    res_again = rest[2:2 + 6 * M].reshape(M, 6)
    assert (status == 0).all() and arr[0] == 1
    others = np.delete(chi2, bad)
    print(f"sample {bad}: chi2 {chi2[bad]:.4g}, the next largest {others.max():.4g}; {(chi2 > 16.81).sum()} of {M} above 16.81; mean of the others {others.mean():.3g}")
    assert int(np.argmax(chi2)) == bad and chi2[bad] > 16.81 and chi2[bad] > 2 * others.max()
    assert 0.8 < others.mean() / 6 < 1.25
    fb = int(w0.imu_bias[bad])
    assert np.array_equal(fs[:, 0], np.bincount(w0.imu_bias, minlength=F)) and fs[fb, 2] == chi2[bad] and int(np.argmax(fs[:, 2])) == fb
    assert np.array_equal(res_again, res)
