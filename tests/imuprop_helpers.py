"""NumPy restatement of ctvio_imu_predict_batch (tests/test_imuprop_reference.py, tests/test_imustep_host.py, tests/test_gpu_imu_predict.py): one
midpoint step of the IMU dead reckoning, its exact Jacobians F (15 x 15) and G (15 x 18) as DENSE matrices, and the recurrence
P_j = F P_{j-1} F^T + G Q G^T -- an independent statement of the formulas of include/ctvio.h.  Every function takes a dtype, so that the same
code runs in np.longdouble (the tests' measure of the float64 recurrence's own rounding).

State: (R 3 x 3, p, v, bg, ba); tangent (dtheta 0..2, dp 3..5, dv 6..8, dbg 9..11, dba 12..14), R <- R Exp(dtheta), the rest additive.
Noise columns of G: (n_g0, n_a0, n_g1, n_a1, n_bg, n_ba), three each."""
import numpy as np

TH, PP, VV, BG, BA = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), slice(12, 15)
DEFAULT_NOISE = (4.0e-3, 8.0e-2, 2.0e-6, 4.0e-5)          # gyr_n, acc_n, gyr_w, acc_w: the reference's parameters


def hat(w):
    w = np.asarray(w)
    z = w.dtype.type(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=w.dtype)


def _coeffs(t2, dtype):
    """(sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3) at t^2: series below t^2 = 1e-2 (16 terms: exact to the dtype), closed forms above."""
    t2 = dtype(t2)
    if t2 < dtype(1e-2):
        a = b = c = dtype(0)
        term = dtype(1)                        # (-t^2)^k / (2 k)!
        for k in range(16):
            a += term / dtype(2 * k + 1)                                   # / (2k+1)!
            b += term / dtype((2 * k + 1) * (2 * k + 2))                   # / (2k+2)!
            c += term / dtype((2 * k + 1) * (2 * k + 2) * (2 * k + 3))     # / (2k+3)!
            term = -term * t2 / dtype((2 * k + 1) * (2 * k + 2))
        return a, b, c
    t = np.sqrt(t2)
    return np.sin(t) / t, (dtype(1) - np.cos(t)) / t2, (t - np.sin(t)) / (t2 * t)


def so3_exp(phi, dtype=np.float64):
    phi = np.asarray(phi, dtype)
    a, b, _ = _coeffs(phi @ phi, dtype)
    H = hat(phi)
    return np.eye(3, dtype=dtype) + a * H + b * (H @ H)


def so3_jr(phi, dtype=np.float64):
    phi = np.asarray(phi, dtype)
    _, b, c = _coeffs(phi @ phi, dtype)
    H = hat(phi)
    return np.eye(3, dtype=dtype) - b * H + c * (H @ H)


def so3_log(R):
    """float64 is enough for its uses (differences of rotations in the tests)."""
    R = np.asarray(R, np.float64)
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(w)
    if s < 1e-8:
        return w
    t = np.arctan2(s, 0.5 * (np.trace(R) - 1.0))
    return w * (t / s)


def step(x, w0, a0, w1, a1, dt, g, dtype=np.float64):
    """One midpoint step of the mean: x = (R, p, v, bg, ba) -> x'."""
    R, p, v, bg, ba = (np.asarray(y, dtype) for y in x)
    w0, a0, w1, a1, g = (np.asarray(y, dtype) for y in (w0, a0, w1, a1, g))
    dt = dtype(dt)
    half = dtype(1) / dtype(2)
    w = half * (w0 + w1) - bg
    R1 = R @ so3_exp(w * dt, dtype)
    A = half * ((R @ (a0 - ba) - g) + (R1 @ (a1 - ba) - g))
    return R1, p + dt * v + half * dt * dt * A, v + dt * A, bg, ba


def jacobians(x, w0, a0, w1, a1, dt, dtype=np.float64):
    """The dense F (15 x 15) and G (15 x 18) of `step` at x."""
    R, _, _, bg, ba = (np.asarray(y, dtype) for y in x)
    w0, a0, w1, a1 = (np.asarray(y, dtype) for y in (w0, a0, w1, a1))
    dt = dtype(dt)
    half, quarter = dtype(1) / dtype(2), dtype(1) / dtype(4)
    I = np.eye(3, dtype=dtype)
    w = half * (w0 + w1) - bg
    E, J = so3_exp(w * dt, dtype), so3_jr(w * dt, dtype)
    R1 = R @ E
    u0, u1 = a0 - ba, a1 - ba
    Ath = -half * (R @ hat(u0) + R1 @ hat(u1) @ E.T)
    Ag = half * (R1 @ hat(u1) @ J) * dt
    Aa = -half * (R + R1)
    F = np.zeros((15, 15), dtype)
    F[TH, TH] = E.T
    F[TH, BG] = -J * dt
    F[PP, TH], F[PP, PP], F[PP, VV], F[PP, BG], F[PP, BA] = half * dt * dt * Ath, I, dt * I, half * dt * dt * Ag, half * dt * dt * Aa
    F[VV, TH], F[VV, VV], F[VV, BG], F[VV, BA] = dt * Ath, I, dt * Ag, dt * Aa
    F[BG, BG] = I
    F[BA, BA] = I
    G = np.zeros((15, 18), dtype)
    G[0:9, 0:3] = -half * F[0:9, BG]
    G[0:9, 6:9] = -half * F[0:9, BG]
    G[PP, 3:6], G[VV, 3:6] = quarter * dt * dt * R, half * dt * R
    G[PP, 9:12], G[VV, 9:12] = quarter * dt * dt * R1, half * dt * R1
    G[BG, 12:15] = dt * I
    G[BA, 15:18] = dt * I
    return F, G


def first_order_F(x, w0, a0, w1, a1, dt):
    """The reference's F (IntegrationBase::midPointIntegration) restated in this tangent's order: I - [w] dt for E^T and J = I."""
    R, _, _, bg, ba = (np.asarray(y, np.float64) for y in x)
    w = 0.5 * (np.asarray(w0) + np.asarray(w1)) - bg
    I = np.eye(3)
    E1t = I - hat(w) * dt
    R1 = R @ so3_exp(w * dt)
    u0, u1 = np.asarray(a0) - ba, np.asarray(a1) - ba
    Ath = -0.5 * (R @ hat(u0) + R1 @ hat(u1) @ E1t)
    Ag = 0.5 * (R1 @ hat(u1)) * dt
    Aa = -0.5 * (R + R1)
    F = np.eye(15)
    F[TH, TH] = E1t
    F[TH, BG] = -I * dt
    F[PP, TH], F[PP, VV], F[PP, BG], F[PP, BA] = 0.5 * dt * dt * Ath, dt * I, 0.5 * dt * dt * Ag, 0.5 * dt * dt * Aa
    F[VV, TH], F[VV, BG], F[VV, BA] = dt * Ath, dt * Ag, dt * Aa
    return F


def noise_Q(noise, dtype=np.float64):
    gn, an, gw, aw = (dtype(s) for s in noise)
    return np.diag(np.repeat(np.array([gn * gn, an * an, gn * gn, an * an, gw * gw, aw * aw], dtype), 3))


def boxminus(xa, xb):
    """The tangent of xa relative to xb (float64): (Log(Rb^T Ra), pa - pb, va - vb, bga - bgb, baa - bab)."""
    return np.concatenate([so3_log(np.asarray(xb[0], np.float64).T @ np.asarray(xa[0], np.float64))] +
                          [np.asarray(xa[i], np.float64) - np.asarray(xb[i], np.float64) for i in range(1, 5)])


def boxplus(x, d):
    R, p, v, bg, ba = (np.asarray(y, np.float64) for y in x)
    return R @ so3_exp(d[TH]), p + d[PP], v + d[VV], bg + d[BG], ba + d[BA]


def propagate(x0, P0, t_ns, gyro, acc, g, noise=DEFAULT_NOISE, dtype=np.float64, cov=True):
    """The recurrence over the samples (t_ns absolute, int64; dt = (t_j - t_{j-1}) * 1e-9 in float64, as the device forms it).  Returns (states: list of
    (R, p, v, bg, ba), covs: (m, 15, 15) or None), sample 0 included."""
    x = tuple(np.asarray(y, dtype) for y in x0)
    P = np.asarray(P0, dtype) if cov else None
    Q = noise_Q(noise, dtype)
    xs, Ps = [x], [P]
    for j in range(1, len(t_ns)):
        dt = np.float64(int(t_ns[j]) - int(t_ns[j - 1])) * np.float64(1e-9)
        if cov:
            F, G = jacobians(x, gyro[j - 1], acc[j - 1], gyro[j], acc[j], dt, dtype)
            P = F @ P @ F.T + G @ Q @ G.T
        x = step(x, gyro[j - 1], acc[j - 1], gyro[j], acc[j], dt, g, dtype)
        xs.append(x)
        Ps.append(P)
    return xs, (np.array(Ps) if cov else None)


def entry_metric(c, r):
    """max over the entries of |c_ab - r_ab| / sqrt(r_aa r_bb), over the rows and columns whose reference diagonal is positive; an entry of c
    in a row or column whose reference diagonal is zero must be an exact zero (else inf)."""
    c, r = np.asarray(c, np.longdouble), np.asarray(r, np.longdouble)
    d = np.diag(r)
    live = d > 0
    sd = np.sqrt(np.where(live, d, 1))
    e = np.abs(c - r) / np.outer(sd, sd)
    both = live[:, None] & live[None, :]
    if (c[~both] != 0).any():
        return float("inf")
    return float(e[both].max()) if both.any() else 0.0
