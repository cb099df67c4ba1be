"""NumPy fp64 reference of ctvio_nav_state_batch (tests/test_navstate_reference.py, tests/test_navjac_host.py, tests/test_gpu_nav_state.py).

Definition (include/ctvio.h): Sigma_nav(t, f) = J Sigma J^T with Sigma the covariance of the trajectory unknowns (tests/cov_helpers.py) and J the
15 x P Jacobian of the navigation state at t with bias state f, tangent (dtheta 0..2, dp 3..5, dv 6..8, dbg 9..11, dba 12..14): the pose rows of
tests/posecov_helpers.py (body), the velocity rows c'_k(u) / dt I on the position unknowns of knots s .. s + 3 (knot s + 3 iff u > 0: c'_3 =
u^2 / 2), the bias rows one-hot on unknowns 6 K + 6 f .. 6 K + 6 f + 5.
"""
from types import SimpleNamespace

import numpy as np

import posecov_helpers as ph
from posecov_helpers import OK, OUTSIDE, SINGULAR, UNTOUCHED, segment, time_of   # noqa: F401  (the statuses and the time rule are the pose entry's)

POSE, VEL, BG, BA = slice(0, 6), slice(6, 9), slice(9, 12), slice(12, 15)
CAP_POSE_BIAS, CAP_VEL = 1e-4, 1e-3       # what every check asserts on its own bound: entries among pose / bias rows, entries with a velocity row


def vel_coeffs(w, u):
    """c'_k(u) / dt in 1 / s: the derivative of the blending coefficients of the position spline."""
    return ph._MB @ np.array([0.0, 1.0, 2.0 * u, 3.0 * u * u]) * (1e9 / w.dt_ns)


def nav_jacobian(w, t_ns, frame=None):
    """The 15 x P Jacobian of the navigation state of window w at absolute time t_ns with bias state frame (None: the newest, F - 1).  Returns
    a namespace (J, s, u, knots, frame, cv: the four velocity coefficients), or None outside the spline."""
    jac = ph.pose_jacobian(w, t_ns)
    if jac is None:
        return None
    f = w.F - 1 if frame is None else int(frame)
    assert 0 <= f < w.F
    cv = vel_coeffs(w, jac.u)
    J = np.zeros((15, w.P))
    J[POSE] = jac.J
    for k in range(len(jac.knots)):
        J[VEL, 6 * (jac.s + k) + 3:6 * (jac.s + k) + 6] = cv[k] * np.eye(3)
    J[9:15, 6 * w.K + 6 * f:6 * w.K + 6 * f + 6] = np.eye(6)
    return SimpleNamespace(J=J, s=jac.s, u=jac.u, knots=jac.knots, frame=f, cv=cv)


def nav_numpy(w, t_ns, frame=None):
    """(R, p, v, bias6) of the state at t_ns from the oracle's NumPy spline evaluation (np_oracle._rot_eval / _pos_eval)."""
    import np_oracle
    s, u, _ = segment(w, t_ns)
    sa, ua = np.array([s]), np.array([u])
    R, p = ph.pose_numpy(w, t_ns)
    v = np_oracle._pos_eval(w.pos, sa, ua, 1e9 / w.dt_ns, 1)[0]
    f = w.F - 1 if frame is None else int(frame)
    return R, p, v, np.array(w.bias[f], float)


def nav_cov_reference(ref, jac, K, route="full"):
    """The status and zero rules on a cov_helpers.cov_reference result over ALL P unknowns (sel = range(P)): returns (15 x 15, status).
    jac None (time outside the spline): NaN, 3.  A knot the state depends on, or its bias state, with an untouched, non-constant unknown: +inf
    on the diagonal and 0 elsewhere, 2.  Otherwise J Sigma J^T with the excluded unknowns' rows and columns zero, 0."""
    if jac is None:
        return np.full((15, 15), np.nan), OUTSIDE
    free_untouched = ref.untouched & ~ref.const
    b0 = 6 * K + 6 * jac.frame
    if any(free_untouched[6 * k:6 * k + 6].any() for k in jac.knots) or free_untouched[b0:b0 + 6].any():
        return np.diag(np.full(15, np.inf)), UNTOUCHED
    Sig = np.array(ref.cov_full if route == "full" else ref.cov_schur)
    Sig[~np.isfinite(Sig)] = 0.0          # (+inf diagonals of untouched unknowns elsewhere in the window: J is zero there)
    return jac.J @ Sig @ jac.J.T, OK


def row_amplification(J, Sig):
    """g_a = (sum_k |J_ak| sqrt(Sigma_kk))^2 / Pi_aa per row of Pi = J Sigma J^T (1 where Pi_aa == 0: such a row is exactly zero): an error of
    tol sqrt(Sigma_kk Sigma_ll) per entry of Sigma becomes at most tol s_a s_b in Pi_ab, that is tol sqrt(g_a g_b) relative to sqrt(Pi_aa Pi_bb)."""
    Sig = np.array(Sig)
    Sig[~np.isfinite(Sig)] = 0.0
    sd = np.sqrt(np.clip(np.diag(Sig), 0.0, None))
    s = np.abs(J) @ sd
    Pi = np.diag(J @ Sig @ J.T)
    g = np.ones(J.shape[0])
    ok = Pi > 0
    g[ok] = s[ok] ** 2 / Pi[ok]
    return g


def entry_bounds(tol, g):
    """The 15 x 15 bound tol sqrt(g_a g_b), and the cap every check holds it under: 1e-3 where a velocity row is involved, else 1e-4."""
    b = tol * np.sqrt(np.outer(g, g))
    cap = np.full((15, 15), CAP_POSE_BIAS)
    cap[VEL, :] = CAP_VEL
    cap[:, VEL] = CAP_VEL
    return b, cap


def entry_errors(c, r):
    """|c_ab - r_ab| / sqrt(r_aa r_bb) entry by entry; rows whose reference diagonal is zero (constant unknowns alone) must be exact zeros in c and
    count as error 0 / inf."""
    c, r = np.asarray(c, float), np.asarray(r, float)
    d = np.diag(r)
    live = d > 0
    e = np.zeros(r.shape)
    sd = np.sqrt(np.where(live, d, 1.0))
    e[np.ix_(live, live)] = (np.abs(c - r) / np.outer(sd, sd))[np.ix_(live, live)]
    dead = ~(live[:, None] & live[None, :])
    e[dead & (c != 0.0)] = np.inf
    return e
