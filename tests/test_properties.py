"""Property tests.

CPU: hypothesis-driven Lie-group identities on the DEVICE math headers compiled for the host (tests/host_math_check.cpp: the very
so3.hpp the kernels include) -- exp(log(R)) = R, log(exp(phi)) = phi, Jr(phi) Jr^-1(phi) = I, continuity across the series / closed
form switch at |phi| = 0.5 -- and gauge invariance of the oracle's cost: a global yaw about gravity plus a translation of every knot
leaves the cost unchanged (landmarks are inverse depths in their anchor camera, biases live in the body frame).  This is what
TrajectoryManager::double2vector relies on when it re-anchors yaw and position after every solve (trajectory_manager.cpp:485-516).
GPU (-m gpu): the same gauge invariance through the HIP path (ctvio_cost), and the solve of a gauge-moved window lands on the gauge-moved
solution.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hm():
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import devprobe
    return devprobe.host_lib("libhostmath.so", "host_math_check.cpp")          # one build rule for every host check


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _so3(hm, phi):
    phi = np.ascontiguousarray(phi, np.float64)
    q = np.zeros(4); Jr = np.zeros((3, 3)); Ji = np.zeros((3, 3)); lg = np.zeros(3)
    hm.hm_so3(_p(phi), _p(q), _p(Jr), _p(Ji), _p(lg))
    return q, Jr, Ji, lg


_unit = st.tuples(st.floats(-1, 1), st.floats(-1, 1), st.floats(-1, 1)).filter(lambda v: 1e-3 < np.linalg.norm(v))
# rotation angles from far below the series switch to close to pi (log is not unique at pi; the windows never get there)
_angle = st.one_of(st.floats(1e-12, 1e-6), st.floats(1e-6, 0.49), st.floats(0.49, 0.51), st.floats(0.51, 3.0))


@settings(max_examples=300, deadline=None)
@given(axis=_unit, angle=_angle)
def test_lie_identities_on_the_device_math(hm, axis, angle):
    a = np.array(axis); a /= np.linalg.norm(a)
    phi = angle * a
    q, Jr, Ji, lg = _so3(hm, phi)
    assert abs(np.linalg.norm(q) - 1.0) < 4e-16 * 4                       # exp lands on the unit sphere
    np.testing.assert_allclose(lg, phi, atol=5e-15 * max(1.0, angle))      # log(exp(phi)) = phi
    np.testing.assert_allclose(Jr @ Ji, np.eye(3), atol=3e-14)             # Jr Jr^-1 = I
    # Jr against its definition exp(phi + d) ~ exp(phi) exp(Jr d): the rotation vector of exp(phi)^-1 exp(phi + d) is Jr d to O(|d|^2)
    dvec = 1e-6 * np.array([0.3, -0.5, 0.8])
    q2, *_ = _so3(hm, phi + dvec)
    qi = np.array([-q[0], -q[1], -q[2], q[3]])
    x1, y1, z1, w1 = qi; x2, y2, z2, w2 = q2
    rel = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
    np.testing.assert_allclose(2.0 * rel, Jr @ dvec, atol=3e-11)


@settings(max_examples=100, deadline=None)
@given(axis=_unit, eps=st.floats(1e-9, 1e-4))
def test_series_and_closed_form_agree_at_the_switch(hm, axis, eps):
    """|phi| = 0.5 -/+ eps take different code paths (alternating series / sin-cos closed forms): the functions are continuous there."""
    a = np.array(axis); a /= np.linalg.norm(a)
    lo = _so3(hm, (0.5 - eps) * a); hi = _so3(hm, (0.5 + eps) * a)
    for x, y, scale in zip(lo[:3], hi[:3], (1.0, 1.0, 1.0)):
        assert np.abs(np.asarray(x) - np.asarray(y)).max() <= 2.5 * eps * scale + 1e-15


def _gauge_move(w, yaw, t):
    """every knot: R <- Rz(yaw) R, p <- Rz(yaw) p + t (quaternions x, y, z, w)"""
    g = w.copy()
    c, s = np.cos(yaw / 2), np.sin(yaw / 2)
    x, y, z, ww = w.quat[:, 0], w.quat[:, 1], w.quat[:, 2], w.quat[:, 3]
    g.quat = np.stack([c * x - s * y, c * y + s * x, c * z + s * ww, c * ww - s * z], axis=1)      # (0, 0, s, c) (x) q
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])
    g.pos = w.pos @ Rz.T + np.asarray(t)
    return g.normalize()


@pytest.mark.parametrize("cfg,seed", [("tiny", 3), ("config1", 1002)])
def test_cost_is_gauge_invariant_oracle(cv, oracle, cfg, seed):
    w = cv.synth.make_window(cfg, seed=seed, with_prior=False)      # (a prior on knot positions / rotations pins the gauge: left out)
    w.ld = 1.3e-5
    c0 = oracle.OracleWindow(w.copy()).cost()
    for yaw, t in ((0.7, (1.0, -2.0, 0.5)), (-2.9, (30.0, 4.0, -7.0)), (3.1, (0.0, 0.0, 0.0))):
        c1 = oracle.OracleWindow(_gauge_move(w, yaw, t)).cost()
        assert c1 == pytest.approx(c0, rel=2e-11)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed", [("tiny", 3), ("config2", 1002), ("config3", 1001)])
def test_cost_and_solution_are_gauge_invariant_on_the_device(cv, cfg, seed):
    w = cv.synth.make_window(cfg, seed=seed, with_prior=False)
    w.ld = 1.3e-5
    moves = ((0.7, (1.0, -2.0, 0.5)), (-2.9, (30.0, 4.0, -7.0)))
    with cv.Solver() as s:
        ws = [w.copy()] + [_gauge_move(w, yaw, t) for yaw, t in moves]
        s.set_windows(ws)
        costs = [s.cost(i) for i in range(len(ws))]
        for c in costs[1:]:
            assert c == pytest.approx(costs[0], rel=2e-11)
        # without a prior the 4-DoF gauge is free and the damped steps are not equivariant to rounding: the COST along the solve is
        sms = s.solve(15)
    for sm in sms[1:]:
        assert sm["final_cost"] == pytest.approx(sms[0]["final_cost"], rel=1e-6)
