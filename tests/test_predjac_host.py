"""CPU: pred_row_pose / pred_B / pred_Cext / pred_A (ctrl-vio_amd/csrc/factors.hpp), the maps of ctvio_predict_landmarks from an IMU-predicted
end state to the image point, compiled with g++ for the test only (tests/host_predjac_check.cpp) and compared with the NumPy restatement
(tests/predproj_helpers.py) at rtol 1e-11, the bound of tests/test_projjac_host.py."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# (|w_e| in rad/s, delta in s): delta = 0 exactly; |w_e delta| = 1e-9; an ordinary rate over a long read-out; a fast turn
CASES = [(1.0, 0.0), (1.0, 1e-9), (0.7, 0.036), (25.0, 0.036)]


@pytest.fixture(scope="module")
def hp():
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import devprobe
    lib = devprobe.host_lib("libhostpredjac.so", "host_predjac_check.cpp")          # one build rule for every host check
    lib.hm_pred_jac.argtypes = [C.c_void_p] * 4 + [C.c_double] + [C.c_void_p] * 8
    lib.hm_pred_jac.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("rate,delta", CASES)
def test_prediction_maps_match_numpy(hp, rate, delta):
    """The pose at the row time, the value, B, C_ext and A entry by entry.  At delta = 0 the velocity and gyro-bias columns of A are exact
    zeros and B's rotation block is the identity to the bit."""
    import imuprop_helpers as ih
    import predproj_helpers as pp
    from scipy.spatial.transform import Rotation as Rot
    rng = np.random.default_rng(int(1000 * rate) + 7)
    rtol = 1e-11
    for _ in range(4):
        q_e = Rot.from_rotvec(rng.normal(0, 1.0, 3)).as_quat()
        p_e, v_e = rng.normal(0, 1.0, 3), rng.normal(0, 1.5, 3)
        w_e = rng.normal(0, 1.0, 3); w_e *= rate / np.linalg.norm(w_e)
        q_CI = Rot.from_rotvec(rng.normal(0, 0.3, 3)).as_quat()
        p_CI = rng.normal(0, 0.1, 3)
        w = SimpleNamespace(q_CI=q_CI, p_CI=p_CI)
        R_e = Rot.from_quat(q_e).as_matrix()
        RI, pI = pp.row_pose((R_e, p_e, v_e), w_e, delta)
        RC = RI @ Rot.from_quat(q_CI).as_matrix()
        y = np.array([rng.normal(0, 0.5), rng.normal(0, 0.5), rng.uniform(2.0, 8.0)])          # in front of the camera
        X = RC @ y + pI + RI @ p_CI
        pose7, proj3, B, Cx, A = np.zeros(7), np.zeros(3), np.zeros((6, 15)), np.zeros((6, 6)), np.zeros((2, 15))
        hp.hm_pred_jac(_p(np.ascontiguousarray(q_e)), _p(p_e), _p(v_e), _p(w_e), delta, _p(X), _p(np.ascontiguousarray(q_CI)), _p(p_CI),
                       _p(pose7), _p(proj3), _p(B), _p(Cx), _p(A))
        An, _, _ = pp.A_matrix(w, y, RI, w_e, delta)
        Bn, Cn = pp.B_matrix(w_e, delta), pp.C_ext(w, RI)
        assert np.abs(pose7[:3] - pI).max() <= rtol * max(1.0, np.abs(pI).max())
        assert (Rot.from_quat(pose7[3:]).inv() * Rot.from_matrix(RI)).magnitude() <= rtol
        assert np.abs(proj3 - np.array([y[0] / y[2], y[1] / y[2], y[2]])).max() <= rtol * max(1.0, np.abs(y).max())
        for name, got, want in (("B", B, Bn), ("C_ext", Cx, Cn), ("A", A, An)):
            assert np.abs(got - want).max() <= rtol * max(1.0, np.abs(want).max()), (name, rate, delta, np.abs(got - want).max())
        if delta == 0.0:
            assert not A[:, 6:].any() and np.array_equal(B[:3, :3], np.eye(3)) and not B[:, 6:].any()
        else:
            assert A[:, 6:12].any()
        assert not A[:, 12:].any()
        if rate * delta == 1e-9:                       # the series branch: Jr = I - [phi]x / 2 to rounding
            assert np.abs(B[:3, 9:12] + delta * (np.eye(3) - 0.5 * ih.hat(w_e * delta))).max() <= 1e-16 * delta
