"""NumPy fp64 reference of ctvio_pose_covariance_batch (tests/test_posecov_reference.py, tests/test_posejac_host.py,
tests/test_gpu_pose_covariance.py).

Definition (include/ctvio.h): Sigma_pose(t) = J Sigma J^T with Sigma the covariance of the spline unknowns (tests/cov_helpers.py) and J the 6 x P
Jacobian of the pose at t: output tangent (theta, p) of R(t) <- R(t) exp(dtheta), p(t) <- p(t) + dp against the library's retraction of the
knots (R_k <- R_k exp(delta_k), p_k <- p_k + dp_k).  The rotation block is the cumulative-B-spline Jacobian of the reference's
So3SplineView::EvaluateRp (so3_spline_view.h:136-198), restated here with NumPy / SciPy rotations; the position block is c_k I with the blending
coefficients of the position spline.  The pose depends on knots s, s + 1, s + 2, and on s + 3 iff u > 0.
"""
from types import SimpleNamespace

import numpy as np
from scipy.spatial.transform import Rotation as Rot

_MB = np.array([[1, -3, 3, -1], [4, 0, -6, 3], [1, 3, 3, -3], [0, 0, 0, 1]], float) / 6   # blending matrix (position spline)
_MC = np.array([[6, 0, 0, 0], [5, 3, -3, 1], [1, 3, 3, -2], [0, 0, 0, 1]], float) / 6     # cumulative blending matrix (rotation spline)

OK, SINGULAR, UNTOUCHED, OUTSIDE = 0, 1, 2, 3


def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], float)


def so3_Jr(phi):
    """Right Jacobian of SO(3): exp(phi + d) = exp(phi) exp(Jr d)."""
    t = np.linalg.norm(phi)
    H = hat(phi)
    if t < 1e-5:
        return np.eye(3) - 0.5 * H + H @ H / 6
    return np.eye(3) - (1 - np.cos(t)) / t ** 2 * H + (t - np.sin(t)) / t ** 3 * H @ H


def so3_Jr_inv(phi):
    t = np.linalg.norm(phi)
    H = hat(phi)
    if t < 1e-5:
        return np.eye(3) + 0.5 * H + H @ H / 12
    return np.eye(3) + 0.5 * H + (1 / t ** 2 - (1 + np.cos(t)) / (2 * t * np.sin(t))) * H @ H


def time_of(w, s, u):
    """The integer-ns time of (segment s, fraction ~u) of window w: the device recomputes u = ((t - t0) mod dt) / dt from it."""
    return int(w.t0_ns + s * w.dt_ns + int(round(u * w.dt_ns)))


def segment(w, t_ns):
    """(s, u, inside) by the integer-ns rule of the trajectory query: inside iff t in [t0, t0 + (K - 3) dt)."""
    st = int(t_ns) - int(w.t0_ns)
    s, u = st // w.dt_ns, (st % w.dt_ns) / float(w.dt_ns)
    return int(s), float(u), (st >= 0 and s + 3 < w.K)


def pose_jacobian(w, t_ns, q_SI=None, p_SI=None):
    """The 6 x P Jacobian of the pose of window w at absolute time t_ns (body pose, or T_I(t) T_SI with the extrinsic q_SI = (x,y,z,w), p_SI).
    Returns a namespace (J, s, u, knots: the knots the pose depends on, R: R_I(t) as a matrix, p: p_I(t)), or None outside the spline."""
    s, u, inside = segment(w, t_ns)
    if not inside:
        return None
    pw = np.array([1.0, u, u * u, u ** 3])
    lam, c = _MC @ pw, _MB @ pw
    Rk = [Rot.from_quat(w.quat[s + i]) for i in range(4)]
    Apost = [None, None, None, np.eye(3)]
    JrI, JrK = [None] * 3, [None] * 3
    acc = Rot.identity()
    for i in (2, 1, 0):
        d = (Rk[i].inv() * Rk[i + 1]).as_rotvec()
        kd = lam[i + 1] * d
        acc = acc * Rot.from_rotvec(-kd)
        JrI[i], JrK[i] = so3_Jr_inv(d), so3_Jr(kd)
        Apost[i] = acc.as_matrix()
    R = (Rk[0] * acc.inv()).as_matrix()
    Jk = [Apost[0], None, None, None]
    for i in range(3):
        Jh = lam[i + 1] * Apost[i + 1] @ JrK[i]
        Jk[i] = Jk[i] - Jh @ JrI[i].T
        Jk[i + 1] = Jh @ JrI[i]
    nk = 4 if u > 0 else 3
    J = np.zeros((6, w.P))
    for k in range(nk):
        J[0:3, 6 * (s + k):6 * (s + k) + 3] = Jk[k]
        J[3:6, 6 * (s + k) + 3:6 * (s + k) + 6] = c[k] * np.eye(3)
    p = c @ w.pos[s:s + 4]
    if q_SI is not None:
        q = np.asarray(q_SI, float)
        RSI = Rot.from_quat(q / np.linalg.norm(q)).as_matrix()
        Jth = J[0:3].copy()
        J[3:6] = J[3:6] - R @ hat(np.asarray(p_SI, float)) @ Jth
        J[0:3] = RSI.T @ Jth
    return SimpleNamespace(J=J, s=s, u=u, knots=list(range(s, s + nk)), R=R, p=p)


def pose_cov_reference(ref, jac, route="full"):
    """The status and zero rules on a cov_helpers.cov_reference result over ALL P unknowns (sel = range(P)): returns (6 x 6, status).
    jac None (time outside the spline): NaN, 3.  A knot the pose depends on with an untouched, non-constant unknown: +inf on the diagonal and 0
    elsewhere, 2.  Otherwise J Sigma J^T with the excluded unknowns' rows and columns zero (constant ones contribute nothing), 0."""
    if jac is None:
        return np.full((6, 6), np.nan), OUTSIDE
    free_untouched = ref.untouched & ~ref.const
    if any(free_untouched[6 * k:6 * k + 6].any() for k in jac.knots):
        return np.diag(np.full(6, np.inf)), UNTOUCHED
    Sig = np.array(ref.cov_full if route == "full" else ref.cov_schur)
    Sig[~np.isfinite(Sig)] = 0.0          # (+inf diagonals of untouched unknowns elsewhere in the window: J is zero there)
    return jac.J @ Sig @ jac.J.T, OK


def amplification(J, Sig):
    """g = max_a (sum_k |J_ak| sqrt(Sigma_kk))^2 / Pi_aa: an error of tol sqrt(Sigma_kk Sigma_ll) per entry of Sigma becomes at most
    tol s_a s_b in Pi = J Sigma J^T with s_a = sum_k |J_ak| sqrt(Sigma_kk); relative to sqrt(Pi_aa Pi_bb) that is at most g tol."""
    Sig = np.array(Sig)
    Sig[~np.isfinite(Sig)] = 0.0
    sd = np.sqrt(np.clip(np.diag(Sig), 0.0, None))
    s = np.abs(J) @ sd
    Pi = np.diag(J @ Sig @ J.T)
    ok = Pi > 0
    return float(np.max(s[ok] ** 2 / Pi[ok])) if ok.any() else 1.0


def pose_numpy(w, t_ns, q_SI=None, p_SI=None):
    """(R, p) of the pose at t_ns from the oracle's NumPy spline evaluation (np_oracle._rot_eval / _pos_eval), with the extrinsic applied."""
    import np_oracle
    s, u, _ = segment(w, t_ns)
    sa, ua = np.array([s]), np.array([u])
    R = np_oracle._rot_eval(w.quat, sa, ua, 1e9 / w.dt_ns)
    p = np_oracle._pos_eval(w.pos, sa, ua, 1e9 / w.dt_ns, 0)[0]
    R = R[0]
    if q_SI is not None:
        p = p + R.apply(np.asarray(p_SI, float))
        R = R * Rot.from_quat(np.asarray(q_SI, float))
    return R, p
