"""CPU: the NumPy reference of the body-rates covariance (tests/rates_helpers.py).  The analytic Jacobian against central differences of the
oracle's NumPy spline evaluation under the library's retraction; independently, its omega and f rows against the oracle's Jacobian of the IMU
residuals at the window's own sample times; the exact zeros of knot s + 3 at u = 0; the gate.  Tolerance: the project's finite-difference
convention, step 1e-6 on the knots, agreement 1e-7 relative to the largest entry of the row block."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

WINDOWS = [("tiny", 7), ("config1", 1003)]
H, FD_TOL = 1e-6, 1e-7
BLOCKS = ("omega", "f", "v_B", "bias")


def _blocks(rh):
    return dict(zip(BLOCKS, (rh.OMEGA, rh.FORCE, rh.VELB, slice(9, 15))))


@pytest.mark.parametrize("cfg, seed", WINDOWS)
@pytest.mark.parametrize("u", [0.0, 0.25, 0.9])
def test_analytic_jacobian_against_central_differences(cv, cfg, seed, u):
    """Check 1: every one of the 15 outputs against every unknown of the four knots, their neighbours and all bias states."""
    import np_oracle
    import rates_helpers as rh
    w = cv.synth.make_window(cfg, seed=seed)
    worst = dict.fromkeys(BLOCKS, 0.0)

    def outputs(x, t, f):
        return np.concatenate(rh.rates_numpy(x, t, f))

    for s, f in ((0, 0), (w.K // 2, None), (w.K - 4, w.F // 2)):
        t = rh.time_of(w, s, u)
        jac = rh.rates_jacobian(w, t, f)
        assert jac.s == s and jac.knots == list(range(s, s + (4 if jac.u > 0 else 3))) and jac.frame == (w.F - 1 if f is None else f)
        cols = list(range(6 * max(s - 1, 0), 6 * min(s + 5, w.K))) + list(range(6 * w.K, 6 * w.K + 6 * w.F))
        fd = np.zeros((15, len(cols)))
        for n, j in enumerate(cols):
            xi = np.zeros(w.N); xi[j] = H
            fd[:, n] = (outputs(np_oracle.retract(w, xi), t, f) - outputs(np_oracle.retract(w, -xi), t, f)) / (2 * H)
        for name, blk in _blocks(rh).items():
            err = float(np.abs(fd[blk] - jac.J[blk][:, cols]).max() / np.abs(jac.J[blk]).max())
            worst[name] = max(worst[name], err)
            assert err <= FD_TOL, (s, f, name, err)
        assert not jac.J[:, [j for j in range(w.P) if j not in cols]].any()
        if jac.u == 0.0:                                   # check 3: knot s + 3 does not enter at u = 0
            assert not jac.J[:, 6 * (s + 3):6 * (s + 4)].any()
    print(f"{cfg} u {u}: max |J - fd| / max |J| per row block " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("cfg, seed", WINDOWS)
def test_imu_rows_against_the_oracle_residual_jacobian(cv, cfg, seed):
    """Check 2: at the time of an IMU sample with bias state b, imu_w (J[0:6] + J[9:15]) is the Jacobian of that sample's residual
    imu_w ((omega + bg_b, f + ba_b) - meas): compared with np_oracle.fd_jacobian of `residuals` over every trajectory unknown but the line
    delay, on up to 40 samples spread over the window."""
    import np_oracle
    import rates_helpers as rh
    w = cv.synth.make_window(cfg, seed=seed)
    cols = list(range(w.P - 1))
    Jo = np_oracle.fd_jacobian(w, cols, eps_rot=H)[:6 * w.M].reshape(w.M, 6, len(cols))
    res = np_oracle.residuals(w)["imu"]
    worst = {"omega": 0.0, "f": 0.0}
    seen_u0 = False
    for m in range(0, w.M, max(1, w.M // 40)):
        t, b = int(w.imu_t[m]), int(w.imu_bias[m])
        jac = rh.rates_jacobian(w, t, b)
        assert jac is not None
        seen_u0 = seen_u0 or jac.u == 0.0
        J6 = (jac.J[0:6] + jac.J[9:15])[:, cols] * np.asarray(w.imu_w, float)[:, None]
        rates, bias = rh.rates_numpy(w, t, b)
        meas = np.concatenate([w.imu_gyro[m], w.imu_acc[m]])
        assert np.abs((rates[:6] + bias - meas) * w.imu_w - res[m]).max() <= 1e-12 * max(1.0, np.abs(res[m]).max()), m
        for name, blk in (("omega", slice(0, 3)), ("f", slice(3, 6))):
            err = float(np.abs(Jo[m][blk] - J6[blk]).max() / np.abs(J6[blk]).max())
            worst[name] = max(worst[name], err)
            assert err <= FD_TOL, (m, name, err)
    print(f"{cfg}: max |imu_w J - oracle| / max |imu_w J| omega {worst['omega']:.3g}, f {worst['f']:.3g}; a sample at u = 0: {seen_u0}")


def test_gate_restates_the_definition(cv):
    """The helper's gate against the 6 x 6 system written out: S = C[0:6, 0:6] + C[0:6, 9:15] + C[9:15, 0:6] + C[9:15, 9:15] + diag(sigma^2)."""
    import rates_helpers as rh
    rng = np.random.default_rng(5)
    B = rng.standard_normal((15, 15))
    C = B @ B.T
    rates, bias, meas, sig = rng.standard_normal(9), 0.1 * rng.standard_normal(6), rng.standard_normal(6), rng.uniform(0.1, 1.0, 6)
    chi, S = rh.gate(rates, bias, C, meas, sig)
    S2 = C[:6, :6] + C[:6, 9:] + C[9:, :6] + C[9:, 9:] + np.diag(sig ** 2)
    e = meas - rates[:6] - bias
    assert np.allclose(S, S2, rtol=1e-14, atol=0) and abs(chi - e @ np.linalg.inv(S2) @ e) <= 1e-10 * chi
    assert (rh.caps()[9:, 9:] == 1e-4).all() and (rh.caps()[:9] == 1e-3).all() and (rh.caps()[:, :9] == 1e-3).all()
