"""CPU: pose_jac_T (ctrl-vio_amd/csrc/factors.hpp), the per-query Jacobian of the pose covariance, compiled with g++ for the test only
(tests/host_posejac_check.cpp) and compared with the NumPy restatement (tests/posecov_helpers.py) at rtol 1e-11, the convention of
tests/test_device_math_host.py for fp64 device math."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@pytest.fixture(scope="module")
def hp():
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import devprobe
    return devprobe.host_lib("libhostposejac.so", "host_posejac_check.cpp")          # one build rule for every host check


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("cam", [False, True], ids=["body", "camera"])
def test_pose_jacobian_matches_numpy(cv, hp, cam):
    import posecov_helpers as ph
    rtol = 1e-11
    w = cv.synth.make_window("config1", seed=1003)
    q_SI = np.ascontiguousarray(w.q_CI / np.linalg.norm(w.q_CI)); p_SI = np.ascontiguousarray(w.p_CI)
    worst = 0.0
    for s in range(0, w.K - 3, 2):
        for u in (0.0, 0.25, 0.9):
            jac = ph.pose_jacobian(w, ph.time_of(w, s, u), *((q_SI, p_SI) if cam else (None, None)))
            jt = np.zeros((24, 6))
            hp.hm_pose_jac(_p(np.ascontiguousarray(w.quat[s:s + 4])), C.c_double(jac.u), int(cam), _p(q_SI), _p(p_SI), _p(jt))
            ref = jac.J[:, 6 * s:6 * s + 24]
            worst = max(worst, float(np.abs(jt.T - ref).max() / np.abs(ref).max()))
            assert np.abs(jt.T - ref).max() <= rtol * np.abs(ref).max(), (s, u)
            if u == 0.0:
                assert not jt[18:].any()          # the last knot's blocks are exact zeros at u = 0
    print(f"{'camera' if cam else 'body'}: max relative difference {worst:.3g}")
