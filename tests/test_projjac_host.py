"""CPU: proj_point / proj_lin / proj_jac_T / proj_cols (ctrl-vio_amd/csrc/factors.hpp), the per-query Jacobian of the landmark projection,
compiled with g++ for the test only (tests/host_projjac_check.cpp) and compared with the NumPy restatement (tests/projection_helpers.py) at
rtol 1e-11, the bound of tests/test_posejac_host.py and the convention of tests/test_device_math_host.py for fp64 device math."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# (anchor (segment, u, row), query (segment, u, row)): u = 0 on either time and on both, the same segment, the same time
CASES = [((2, 0.3, 120), (4, 0.75, 300)), ((4, 0.0, 0), (3, 0.6, 17)), ((1, 0.9, 845), (5, 0.0, 0)), ((0, 0.0, 0), (3, 0.0, 0)),
         ((5, 0.37, 10), (5, 0.87, 470)), ((6, 0.4, 33), (6, 0.4, 33)), ((9, 0.5, 1), (2, 0.25, 0))]


@pytest.fixture(scope="module")
def hp():
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import devprobe
    lib = devprobe.host_lib("libhostprojjac.so", "host_projjac_check.cpp")          # one build rule for every host check
    lib.hm_proj_jac.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_double, C.c_double] + [C.c_void_p] * 7
    lib.hm_proj_jac.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_projection_jacobian_matches_numpy(cv, hp):
    """Both 24 x 2 blocks against the NumPy Jp: where the knot groups overlap the reference holds the sum of the two blocks; the inverse-depth
    and line-delay columns; the value.  At u = 0 the block of knot s + 3 is an exact zero."""
    import posecov_helpers as ph
    import projection_helpers as pr
    rtol = 1e-11
    w0 = cv.synth.make_window("config1", seed=1003)
    w0.ld = 2.0e-5                                # the row time is not the frame time
    ld_ns = int(np.int64(w0.ld * 1e9))
    l = int(w0.v_lm[0])
    worst = 0.0
    for (sa, ua, ra), (sq, uq, rq) in CASES:
        w = w0.copy()
        tau_a, tau_q = ph.time_of(w, sa, ua), ph.time_of(w, sq, uq)
        mine = w.v_lm == l
        w.v_ti[mine] = tau_a - ra * ld_ns          # the landmark re-anchored at (segment sa, u ua) on row ra
        w.v_rowi[mine] = ra
        t_q = tau_q - rq * ld_ns
        pj = pr.projection_jacobian(w, l, t_q, rq)
        assert pj is not None and (pj.s_a, pj.s_q) == (sa, sq) and pj.tau_q == tau_q
        u_a = ph.segment(w, tau_a)[1]
        assert (u_a == 0.0) == (ua == 0.0) and (pj.u_q == 0.0) == (uq == 0.0)
        jt_a, jt_q, out7 = np.zeros((24, 2)), np.zeros((24, 2)), np.zeros(7)
        obs3 = np.array([w.v_pi[mine][0, 0], w.v_pi[mine][0, 1], w.rho[l]])
        hp.hm_proj_jac(_p(np.ascontiguousarray(w.quat[sa:sa + 4])), _p(np.ascontiguousarray(w.pos[sa:sa + 4])), u_a,
                       _p(np.ascontiguousarray(w.quat[sq:sq + 4])), _p(np.ascontiguousarray(w.pos[sq:sq + 4])), pj.u_q, 1e9 / w.dt_ns,
                       _p(np.ascontiguousarray(w.q_CI, float)), _p(np.ascontiguousarray(w.p_CI, float)), _p(obs3), _p(np.array([float(ra), float(rq)])),
                       _p(jt_a), _p(jt_q), _p(out7))
        J = np.zeros((2, w.P))
        J[:, 6 * sa:6 * sa + 24] += jt_a.T          # anchor term + query term, the kernel's order
        J[:, 6 * sq:6 * sq + 24] += jt_q.T
        J[:, w.P - 1] = out7[5:7]
        scale = max(np.abs(jt_a).max(), np.abs(jt_q).max())
        d = float(np.abs(J[:, :6 * w.K] - pj.Jp[:, :6 * w.K]).max() / scale)
        d = max(d, float(np.abs(out7[3:5] - pj.j).max() / max(1.0, np.abs(pj.j).max())))
        d = max(d, float(np.abs(out7[5:7] - pj.Jp[:, w.P - 1]).max() / max(1.0, np.abs(pj.Jp[:, w.P - 1]).max())))
        d = max(d, float(np.abs(out7[:3] - pj.proj).max() / max(1.0, np.abs(pj.proj).max())))
        worst = max(worst, d)
        assert d <= rtol, ((sa, ua, ra), (sq, uq, rq), d)
        if ua == 0.0:
            assert not jt_a[18:].any()              # the last knot's block stays an exact zero at u = 0
        if uq == 0.0:
            assert not jt_q[18:].any()
        if ra == 0 and rq == 0:
            assert not out7[5:7].any()
    print(f"max relative difference {worst:.3g}")
