"""CPU: nav_jac_T (ctrl-vio_amd/csrc/factors.hpp), the per-query Jacobian of the navigation-state covariance, compiled with g++ for the test only
(tests/host_navjac_check.cpp) and compared with the NumPy restatement (tests/navstate_helpers.py) at rtol 1e-11, the convention of
tests/test_device_math_host.py for fp64 device math."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@pytest.fixture(scope="module")
def hn():
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import devprobe
    return devprobe.host_lib("libhostnavjac.so", "host_navjac_check.cpp")          # one build rule for every host check


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_nav_jacobian_matches_numpy(cv, hn):
    import navstate_helpers as nh
    rtol = 1e-11
    w = cv.synth.make_window("config1", seed=1003)
    idt = 1e9 / w.dt_ns
    worst = 0.0
    for s in range(0, w.K - 3, 2):
        for u in (0.0, 0.25, 0.9):
            jac = nh.nav_jacobian(w, nh.time_of(w, s, u))
            jt = np.zeros((24, 6)); cv4 = np.zeros(4)
            hn.hm_nav_jac(_p(np.ascontiguousarray(w.quat[s:s + 4])), C.c_double(jac.u), C.c_double(idt), _p(jt), _p(cv4))
            ref = jac.J[:6, 6 * s:6 * s + 24]
            worst = max(worst, float(np.abs(jt.T - ref).max() / np.abs(ref).max()), float(np.abs(cv4 - jac.cv).max() / np.abs(jac.cv).max()))
            assert np.abs(jt.T - ref).max() <= rtol * np.abs(ref).max(), (s, u)
            assert np.abs(cv4 - jac.cv).max() <= rtol * np.abs(jac.cv).max(), (s, u)
            # the velocity rows of the helper are these coefficients on the position unknowns (knot s + 3 only if u > 0)
            vel = np.zeros((3, 24))
            for k in range(len(jac.knots)):
                vel[:, 6 * k + 3:6 * k + 6] = cv4[k] * np.eye(3)
            assert np.abs(vel - jac.J[6:9, 6 * s:6 * s + 24]).max() <= rtol * np.abs(jac.cv).max(), (s, u)
            if u == 0.0:
                assert not jt[18:].any() and cv4[3] == 0.0          # the last knot's blocks and c'_3 are exact zeros at u = 0
    print(f"max relative difference {worst:.3g}")
