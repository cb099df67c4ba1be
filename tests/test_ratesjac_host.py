"""CPU: rates_jac_T (ctrl-vio_amd/csrc/factors.hpp), the per-query Jacobian of the body-rates covariance, compiled with g++ for the test only
(tests/host_rates_check.cpp) and compared with the NumPy restatement (tests/rates_helpers.py) at rtol 1e-11, the convention of
tests/test_device_math_host.py for fp64 device math."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@pytest.fixture(scope="module")
def hr():
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import devprobe
    return devprobe.host_lib("libhostrates.so", "host_rates_check.cpp")          # one build rule for every host check


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("cfg, seed", [("tiny", 7), ("config1", 1003)])
def test_rates_jacobian_matches_numpy(cv, hr, cfg, seed):
    """Every row block (omega, f, v_B) of the 24 x 9 block against the helper's J, relative to the largest entry of the row block; at u = 0 the
    last knot's rows are exact zeros."""
    import rates_helpers as rh
    rtol = 1e-11
    w = cv.synth.make_window(cfg, seed=seed)
    idt = 1e9 / w.dt_ns
    worst = 0.0
    for s in range(0, w.K - 3, 2):
        for u in (0.0, 0.25, 0.9):
            jac = rh.rates_jacobian(w, rh.time_of(w, s, u))
            jt = np.full((24, 9), np.nan)
            hr.hm_rates_jac(_p(np.ascontiguousarray(w.quat[s:s + 4])), _p(np.ascontiguousarray(w.pos[s:s + 4])), C.c_double(jac.u), C.c_double(idt),
                            _p(np.ascontiguousarray(w.gravity, dtype=np.float64)), _p(jt))
            ref = jac.J[:9, 6 * s:6 * s + 24]
            for blk in (rh.OMEGA, rh.FORCE, rh.VELB):
                scale = np.abs(ref[blk]).max()
                err = float(np.abs(jt.T[blk] - ref[blk]).max() / scale)
                worst = max(worst, err)
                assert err <= rtol, (s, u, blk, err)
            if u == 0.0:
                assert not jt[18:].any()          # the last knot's blocks are exact zeros at u = 0
    print(f"{cfg}: max relative difference {worst:.3g}")
