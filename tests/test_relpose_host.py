"""CPU: rel_pose_jac_T (ctrl-vio_amd/csrc/factors.hpp), the per-query Jacobian of the relative-pose covariance, compiled with g++ for the test
only (tests/host_relpose_check.cpp) and compared with the NumPy restatement (tests/relpose_helpers.py) at rtol 1e-11, the bound of
tests/test_navjac_host.py and the convention of tests/test_device_math_host.py for fp64 device math."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

EXT = (np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9]), np.array([0.05, -0.02, 0.1]))
PAIRS = [((2, 0.3), (4, 0.75)), ((1, 0.9), (9, 0.37)), ((5, 0.37), (5, 0.87)), ((9, 0.5), (2, 0.25)), ((4, 0.0), (3, 0.6)), ((0, 0.0), (3, 0.0)),
         ((6, 0.4), (6, 0.4))]


@pytest.fixture(scope="module")
def hr():
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import devprobe
    lib = devprobe.host_lib("libhostrelpose.so", "host_relpose_check.cpp")          # one build rule for every host check
    lib.hm_rel_pose_jac.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_double, C.c_int] + [C.c_void_p] * 5
    lib.hm_rel_pose_jac.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("ext", [False, True], ids=["body", "extrinsic"])
def test_rel_jacobian_matches_numpy(cv, hr, ext):
    """Both 24 x 6 blocks against the NumPy J_rel: where the knot groups overlap the reference holds the sum of the two blocks; the value
    against rel_numpy."""
    import relpose_helpers as rh
    rtol = 1e-11
    w = cv.synth.make_window("config1", seed=1003)
    q_SI, p_SI = EXT if ext else (None, None)
    qe, pe = (np.ascontiguousarray(EXT[0]), np.ascontiguousarray(EXT[1])) if ext else (np.array([0.0, 0, 0, 1]), np.zeros(3))
    worst = 0.0
    for (sa, ua), (sb, ub) in PAIRS:
        ta, tb = rh.time_of(w, sa, ua), rh.time_of(w, sb, ub)
        jac = rh.rel_jacobian(w, ta, tb, q_SI, p_SI)
        jt_a, jt_b, rel7 = np.zeros((24, 6)), np.zeros((24, 6)), np.zeros(7)
        hr.hm_rel_pose_jac(_p(np.ascontiguousarray(w.quat[sa:sa + 4])), _p(np.ascontiguousarray(w.pos[sa:sa + 4])), jac.a.u,
                           _p(np.ascontiguousarray(w.quat[sb:sb + 4])), _p(np.ascontiguousarray(w.pos[sb:sb + 4])), jac.b.u, int(ext), _p(qe), _p(pe),
                           _p(jt_a), _p(jt_b), _p(rel7))
        J = np.zeros((6, w.P))
        J[:, 6 * sa:6 * sa + 24] += jt_a.T          # a-term + b-term, the kernel's order
        J[:, 6 * sb:6 * sb + 24] += jt_b.T
        scale = max(np.abs(jt_a).max(), np.abs(jt_b).max())
        d = float(np.abs(J - jac.J).max() / scale)
        worst = max(worst, d)
        assert d <= rtol, ((sa, ua), (sb, ub), d)
        R, p = rh.rel_numpy(w, ta, tb, q_SI, p_SI)
        assert abs(np.linalg.norm(rel7[3:]) - 1.0) <= 1e-15
        assert (rh.Rot.from_quat(rel7[3:]).inv() * R).magnitude() <= 1e-12 and np.abs(rel7[:3] - p).max() <= 1e-12 * max(1.0, np.abs(p).max())
        if ua == 0.0:
            assert not jt_a[18:].any()              # the last knot's block stays an exact zero at u = 0
        if ub == 0.0:
            assert not jt_b[18:].any()
    print(f"{'extrinsic' if ext else 'body'}: max relative difference {worst:.3g}")
