"""CPU: imu_step (ctrl-vio_amd/csrc/factors.hpp), the midpoint step of k_imu_propagate with the blocks of its Jacobians, compiled with g++ for
the test only (tests/host_imustep_check.cpp) and compared with the NumPy restatement (tests/imuprop_helpers.py) at rtol 1e-11, the convention
of tests/test_navjac_host.py for fp64 device math -- including w = 0 exactly and |w dt| = 1e-9, the small-angle branches."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@pytest.fixture(scope="module")
def hs():
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import devprobe
    lib = devprobe.host_lib("libhostimustep.so", "host_imustep_check.cpp")          # one build rule for every host check
    lib.hm_imu_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    lib.hm_imu_step.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cases():
    """(name, gyro rate of the midpoint after the bias, dt): ordinary rates, a fast turn past the series' range of so3_exp (|w dt| > 0.5), the
    exact zero and a tiny angle."""
    return [("1 rad/s, 5 ms", 1.0, 5e-3), ("0.3 rad/s, 7 ms", 0.3, 7e-3), ("60 rad/s, 10 ms", 60.0, 1e-2), ("w = 0", 0.0, 5e-3),
            ("|w dt| = 1e-9", 2e-7, 5e-3)]


def test_imu_step_matches_numpy(hs):
    import imuprop_helpers as ih
    from scipy.spatial.transform import Rotation as Rot
    rtol = 1e-11
    worst = 0.0
    for ci, (name, rate, dt) in enumerate(_cases()):
        for seed in range(4):
            rng = np.random.default_rng(100 * ci + seed)
            q = Rot.from_rotvec(rng.normal(0, 1.0, 3)).as_quat()
            R = Rot.from_quat(q).as_matrix()
            p, v, bg, ba = rng.normal(0, 2.0, 3), rng.normal(0, 1.0, 3), rng.normal(0, 1e-2, 3), rng.normal(0, 1e-1, 3)
            g = np.array([0.0, 0.0, 9.81])
            axis = rng.normal(0, 1.0, 3)
            w = rate * axis / np.linalg.norm(axis)
            half = rng.normal(0, 0.05, 3) if rate >= 0.1 else np.zeros(3)
            w0, w1 = (w + bg) + half, (w + bg) - half            # the midpoint minus bg is w (to rounding; exactly for w = 0: bg - bg)
            if rate == 0.0:
                w0 = w1 = bg.copy()
            a0, a1 = R.T @ g + rng.normal(0, 1.0, 3), R.T @ g + rng.normal(0, 1.0, 3)
            x = np.concatenate([q, p, v, bg, ba])
            xm = x.copy()
            meas = np.concatenate([w0, a0, w1, a1])
            blocks = np.zeros((7, 3, 3))
            hs.hm_imu_step(_p(x), _p(meas), _p(g), dt, _p(blocks))
            hs.hm_imu_step(_p(xm), _p(meas), _p(g), dt, None)
            assert np.array_equal(x, xm), name                   # the mean does not depend on the request for blocks
            st = (R, p, v, bg, ba)
            R1, p1, v1, _, _ = ih.step(st, w0, a0, w1, a1, dt, g)
            F, G = ih.jacobians(st, w0, a0, w1, a1, dt)
            assert (Rot.from_quat(x[0:4]).inv() * Rot.from_matrix(R1)).magnitude() <= 1e-14, name
            assert abs(np.linalg.norm(x[0:4]) - 1.0) <= 1e-15
            for got, ref in ((x[4:7], p1), (x[7:10], v1)):
                assert np.abs(got - ref).max() <= rtol * max(1.0, np.abs(ref).max()), name
            assert np.array_equal(x[10:], np.concatenate([bg, ba]))
            refs = [F[ih.TH, ih.TH], F[ih.TH, ih.BG], F[ih.VV, ih.TH], F[ih.VV, ih.BG], F[ih.VV, ih.BA], R, R1]
            for k, (b, ref) in enumerate(zip(blocks, refs)):
                scale = np.abs(ref).max()
                e = np.abs(b - ref).max()
                worst = max(worst, e / scale)
                assert e <= rtol * scale, (name, seed, k, e, scale)
            # the position rows are dt / 2 times the velocity rows, the gyro-noise columns -1/2 of the bg columns
            for cols in (ih.TH, ih.BG, ih.BA):
                assert np.abs(F[ih.PP, cols] - 0.5 * dt * F[ih.VV, cols]).max() <= 1e-15 * max(np.abs(F[ih.VV, cols]).max(), 1e-300)
            if rate == 0.0:                                       # Exp(0) = I and Jr(0) = I exactly
                assert np.array_equal(blocks[0], np.eye(3)) and np.array_equal(blocks[1], -dt * np.eye(3)) and np.abs(blocks[5] - blocks[6]).max() <= 1e-15
    print(f"max relative difference of a block {worst:.3g}")
