"""CPU: the NumPy restatement of the IMU prediction (tests/imuprop_helpers.py) is consistent with itself and with the reference's first-order
form: F and G are the derivatives of the step map, F reduces to IntegrationBase::midPointIntegration's blocks up to second order in |w| dt,
the recurrence keeps P symmetric positive semi-definite, and without noise and initial uncertainty P stays zero."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def draw(seed, dt=5e-3, rate=1.0):
    """A random attitude and state, two samples with |w| ~ rate rad/s."""
    import imuprop_helpers as ih
    rng = np.random.default_rng(seed)
    R = ih.so3_exp(rng.normal(0, 1.0, 3))
    x = (R, rng.normal(0, 0.3, 3), rng.normal(0, 0.5, 3), rng.normal(0, 1e-2, 3), rng.normal(0, 1e-1, 3))
    g = np.array([0.0, 0.0, 9.81])
    w = rng.normal(0, 1.0, 3)
    w *= rate / np.linalg.norm(w)
    w0, w1 = w + rng.normal(0, 0.05, 3) + x[3], w - rng.normal(0, 0.05, 3) + x[3]
    a0, a1 = R.T @ g + rng.normal(0, 1.0, 3), R.T @ g + rng.normal(0, 1.0, 3)
    return x, w0, a0, w1, a1, dt, g


def test_F_and_G_are_the_derivatives_of_the_step():
    """Central differences (h = 1e-6) of the helper's own step map, in the state's tangent and in the additive noises of both samples and of
    the bias walks, at |w| ~ 1 rad/s, dt = 5 ms: <= 1e-9 max|F| (8e-11 measured)."""
    import imuprop_helpers as ih
    h = 1e-6
    worst = 0.0
    for seed in range(5):
        x, w0, a0, w1, a1, dt, g = draw(seed)
        F, G = ih.jacobians(x, w0, a0, w1, a1, dt)
        x1 = ih.step(x, w0, a0, w1, a1, dt, g)
        Fn = np.zeros((15, 15))
        for k in range(15):
            d = np.zeros(15); d[k] = h
            Fn[:, k] = (ih.boxminus(ih.step(ih.boxplus(x, d), w0, a0, w1, a1, dt, g), x1) -
                        ih.boxminus(ih.step(ih.boxplus(x, -d), w0, a0, w1, a1, dt, g), x1)) / (2 * h)
        Gn = np.zeros((15, 18))
        for k in range(12):                    # n_g0, n_a0, n_g1, n_a1: added to the measurements
            def at(s):
                m = [np.array(w0), np.array(a0), np.array(w1), np.array(a1)]
                m[k // 3][k % 3] += s
                return ih.step(x, m[0], m[1], m[2], m[3], dt, g)
            Gn[:, k] = (ih.boxminus(at(h), x1) - ih.boxminus(at(-h), x1)) / (2 * h)
        for k in range(6):                     # the bias walks: sigma dt on the bias itself, after the step
            Gn[9 + k, 12 + k] = dt
        eF, eG = np.abs(F - Fn).max(), np.abs(G - Gn).max()
        worst = max(worst, eF, eG)
        assert eF <= 1e-9 * np.abs(F).max() and eG <= 1e-9 * np.abs(F).max(), (seed, eF, eG)
    print(f"F, G against central differences: {worst:.3g}")


def test_F_reduces_to_the_first_order_form():
    """The reference's blocks (I - [w] dt for E^T, J = I) differ from the exact ones at second order: every entry within (|w| dt)^2 times the
    size of what multiplies it, the difference of the rotation block falling by 4 when dt halves -- and not zero."""
    import imuprop_helpers as ih
    for seed in range(3):
        x, w0, a0, w1, a1, dt, g = draw(seed)
        d = []
        for s in (1.0, 0.5):
            F = ih.jacobians(x, w0, a0, w1, a1, s * dt)[0]
            F1 = ih.first_order_F(x, w0, a0, w1, a1, s * dt)
            w = np.linalg.norm(0.5 * (w0 + w1) - x[3])
            phi = w * s * dt
            amax = max(np.linalg.norm(a0 - x[4]), np.linalg.norm(a1 - x[4]))
            assert np.abs(F - F1).max() <= phi * phi * max(1.0, 1.0 / w) * max(1.0, amax * s * dt), (seed, s)
            d.append(np.abs(F - F1)[ih.TH, ih.TH].max())
        assert d[0] > 1e-6 and 3.5 < d[0] / d[1] < 4.5, d


def test_P_stays_symmetric_positive_semidefinite():
    import imuprop_helpers as ih
    rng = np.random.default_rng(11)
    x, _, _, _, _, dt, g = draw(3)
    m = 41
    t = (np.arange(m) * 5_000_000).astype(np.int64)
    gyro = rng.normal(0, 0.5, (m, 3))
    acc = x[0].T @ g + rng.normal(0, 1.0, (m, 3))
    A = rng.normal(0, 1e-2, (15, 15))
    _, Ps = ih.propagate(x, A @ A.T, t, gyro, acc, g)
    for P in Ps:
        assert np.abs(P - P.T).max() <= 1e-14 * np.abs(P).max()
        assert np.linalg.eigvalsh(0.5 * (P + P.T)).min() >= -1e-12 * np.abs(P).max()
    assert np.trace(Ps[-1]) > np.trace(Ps[0])


def test_no_noise_no_uncertainty():
    import imuprop_helpers as ih
    rng = np.random.default_rng(12)
    x, _, _, _, _, dt, g = draw(4)
    m = 41
    t = (np.arange(m) * 5_000_000).astype(np.int64)
    _, Ps = ih.propagate(x, np.zeros((15, 15)), t, rng.normal(0, 0.5, (m, 3)), rng.normal(0, 1.0, (m, 3)), g, noise=(0, 0, 0, 0))
    assert not Ps.any()


def test_longdouble_measures_the_rounding_of_the_recurrence():
    """The same code in np.longdouble: the float64 recurrence is within 1e-13 of it over 40 steps (5e-15 measured), the d of the GPU test's bound."""
    import imuprop_helpers as ih
    rng = np.random.default_rng(13)
    x, _, _, _, _, dt, g = draw(5)
    m = 41
    t = (np.arange(m) * 5_000_000).astype(np.int64)
    gyro, acc = rng.normal(0, 0.5, (m, 3)), x[0].T @ g + rng.normal(0, 1.0, (m, 3))
    A = rng.normal(0, 1e-2, (15, 15))
    _, P64 = ih.propagate(x, A @ A.T, t, gyro, acc, g)
    _, Pld = ih.propagate(x, A @ A.T, t, gyro, acc, g, dtype=np.longdouble)
    d = max(ih.entry_metric(a, b) for a, b in zip(P64, Pld))
    print(f"float64 against longdouble over {m - 1} steps: {d:.3g}")
    assert d <= 1e-13
