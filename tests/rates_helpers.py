"""NumPy fp64 reference of ctvio_body_rates_batch (tests/test_rates_reference.py, tests/test_ratesjac_host.py, tests/test_gpu_body_rates.py).

Definition (include/ctvio.h): rates = (omega, f, v_B) with omega the body angular velocity, f = R(t)^T (p''(t) + g) the specific force and
v_B = R(t)^T v_W(t) the body-frame velocity; Sigma_rates(t, f) = J Sigma J^T with Sigma the covariance of the trajectory unknowns
(tests/cov_helpers.py) and J the 15 x P Jacobian in the additive tangent (domega 0..2, df 3..5, dv_B 6..8, dbg 9..11, dba 12..14) against the
library's retraction of the knots (R_k <- R_k exp(delta_k), p_k <- p_k + dp_k), knots s .. s + 3 (knot s + 3 iff u > 0).

The restatement is not the device's: the omega rows differentiate the recursion omega_{i+1} = A_i^T omega_i + lam'_{i+1} d_i through the pair
logs d_i; the f and v_B rows use R(t) <- R(t) exp(dtheta) => R^T x <- R^T x + [R^T x]x dtheta with the pose reference's J_theta
(tests/posecov_helpers.py), where the device takes the f rows from the IMU factor's own chain (imu_eval_core: Ja).
"""
from types import SimpleNamespace

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import posecov_helpers as ph
from posecov_helpers import OK, OUTSIDE, SINGULAR, UNTOUCHED, hat, segment, time_of   # noqa: F401  (the statuses and the time rule are the pose entry's)

OMEGA, FORCE, VELB, BG, BA = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), slice(12, 15)
CAP_BIAS, CAP_REST = 1e-4, 1e-3       # what every check asserts on its own bound: entries among bias rows, every other entry


def rates_numpy(w, t_ns, frame=None):
    """(rates9, bias6) at t_ns from the oracle's NumPy spline evaluation (np_oracle._rot_eval / _pos_eval)."""
    import np_oracle
    s, u, _ = segment(w, t_ns)
    sa, ua, idt = np.array([s]), np.array([u]), 1e9 / w.dt_ns
    R, om = np_oracle._rot_eval(w.quat, sa, ua, idt, True)
    acc = np_oracle._pos_eval(w.pos, sa, ua, idt, 2)[0] + np.asarray(w.gravity, float)
    vel = np_oracle._pos_eval(w.pos, sa, ua, idt, 1)[0]
    f = w.F - 1 if frame is None else int(frame)
    return np.concatenate([om[0], R[0].inv().apply(acc), R[0].inv().apply(vel)]), np.array(w.bias[f], float)


def omega_blocks(w, s, u):
    """d(omega) / d(delta_k) of the four knots s .. s + 3, and omega."""
    idt = 1e9 / w.dt_ns
    lam = ph._MC @ np.array([1.0, u, u * u, u ** 3])
    dlam = ph._MC @ np.array([0.0, 1.0, 2.0 * u, 3.0 * u * u]) * idt
    Rk = [Rot.from_quat(w.quat[s + i]) for i in range(4)]
    d = [(Rk[i].inv() * Rk[i + 1]).as_rotvec() for i in range(3)]
    At = [Rot.from_rotvec(-lam[i + 1] * d[i]).as_matrix() for i in range(3)]      # A_i^T
    om = [np.zeros(3)]
    for i in range(3):
        om.append(At[i] @ om[i] + dlam[i + 1] * d[i])
    Jk = [np.zeros((3, 3)) for _ in range(4)]
    for j in range(3):
        D = lam[j + 1] * At[j] @ hat(om[j]) @ ph.so3_Jr(-lam[j + 1] * d[j]) + dlam[j + 1] * np.eye(3)     # d(omega_{j+1}) / d(d_j)
        for i in range(j + 1, 3):
            D = At[i] @ D
        JrI = ph.so3_Jr_inv(d[j])
        Jk[j] = Jk[j] - D @ JrI.T
        Jk[j + 1] = Jk[j + 1] + D @ JrI
    return Jk, om[3]


def rates_jacobian(w, t_ns, frame=None):
    """The 15 x P Jacobian of the body rates of window w at absolute time t_ns with bias state frame (None: the newest, F - 1).  Returns a
    namespace (J, s, u, knots, frame), or None outside the spline."""
    jac = ph.pose_jacobian(w, t_ns)
    if jac is None:
        return None
    f = w.F - 1 if frame is None else int(frame)
    assert 0 <= f < w.F
    s, u, idt = jac.s, jac.u, 1e9 / w.dt_ns
    c1 = ph._MB @ np.array([0.0, 1.0, 2.0 * u, 3.0 * u * u]) * idt
    c2 = ph._MB @ np.array([0.0, 0.0, 2.0, 6.0 * u]) * idt * idt
    P4 = w.pos[s:s + 4]
    RT = jac.R.T
    force, vb = RT @ (c2 @ P4 + np.asarray(w.gravity, float)), RT @ (c1 @ P4)
    Jw, _ = omega_blocks(w, s, u)
    J = np.zeros((15, w.P))
    for k in range(len(jac.knots)):
        rot, pos = slice(6 * (s + k), 6 * (s + k) + 3), slice(6 * (s + k) + 3, 6 * (s + k) + 6)
        Jth = jac.J[0:3, rot]
        J[OMEGA, rot] = Jw[k]
        J[FORCE, rot] = hat(force) @ Jth
        J[FORCE, pos] = c2[k] * RT
        J[VELB, rot] = hat(vb) @ Jth
        J[VELB, pos] = c1[k] * RT
    J[9:15, 6 * w.K + 6 * f:6 * w.K + 6 * f + 6] = np.eye(6)
    return SimpleNamespace(J=J, s=s, u=u, knots=jac.knots, frame=f)


def caps():
    """The 15 x 15 cap every check holds its bound under: 1e-4 among bias rows, 1e-3 for every entry with an omega, f or v_B row."""
    cap = np.full((15, 15), CAP_REST)
    cap[9:, 9:] = CAP_BIAS
    return cap


def gate(rates9, bias6, cov, meas6, sigma6):
    """(chi2, S) of one IMU sample: e = meas - (omega + bg, f + ba), S = A C A^T + diag(sigma^2), chi2 = e^T S^-1 e."""
    A = np.zeros((6, 15))
    A[:, 0:6] = np.eye(6)
    A[:, 9:15] = np.eye(6)
    S = A @ np.asarray(cov, float) @ A.T + np.diag(np.asarray(sigma6, float) ** 2)
    e = np.asarray(meas6, float) - (np.asarray(rates9, float)[:6] + np.asarray(bias6, float))
    return float(e @ np.linalg.solve(S, e)), S
