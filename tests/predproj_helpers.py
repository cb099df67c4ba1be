"""NumPy fp64 reference of ctvio_predict_landmarks_batch (tests/test_predproj_reference.py, tests/test_predjac_host.py,
tests/test_gpu_predict_landmarks.py), built from the helpers of the entries it composes.

Definition (include/ctvio.h): a prediction (window, bias state f, samples t / gyro / acc) starts at the navigation state of
navstate_helpers at (t[0], f) and runs imuprop_helpers.propagate to the end state (R, p, v, bg, ba); w_e = gyro[-1] - bg.  At image row `row`,
delta = float(row * int(ld * 1e9)) * 1e-9, R_I = R Exp(w_e delta), p_I = p + delta v, the camera pose is T_I (q_CI, p_CI); X is the world point
of lmpoint_helpers; y = R_C^T (X - p_C), proj = (y.x / y.z, y.y / y.z, y.z).
[Jp | j]: Jp = A Phi J_nav + Pi R_C^T Jp_X (+ the read-out term in the line-delay column), j = Pi R_C^T j_rho, with
A = Pi [[y]x, -R_C^T] C_ext B (2 x 15), Phi the product of imuprop_helpers.jacobians' F, J_nav navstate_helpers.nav_jacobian.
Cov = [Jp | j] Sigma [Jp | j]^T + A N A^T over lmpoint_helpers.joint_reference, N = imuprop_helpers.propagate's last P from P0 = 0.
"""
from types import SimpleNamespace

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import cov_helpers as ch
import imuprop_helpers as ih
import lmpoint_helpers as lh
import navstate_helpers as nh
import posecov_helpers as ph

OK, SINGULAR, NO_INFO, NONE = 0, 1, 2, 3
NAN3 = np.full(3, np.nan)


def delta_of(w, row):
    """The read-out offset of a row in seconds, from the line delay truncated to integer ns as the factors take it."""
    return float(int(row) * int(np.int64(w.ld * 1e9))) * 1e-9


def start_state(w, t0_ns, frame=None):
    """(R matrix, p, v, bg, ba) of navstate_helpers at (t0_ns, frame), or None outside the spline."""
    if not ph.segment(w, t0_ns)[2]:
        return None
    R, p, v, b = nh.nav_numpy(w, t0_ns, frame)
    return R.as_matrix(), p, v, b[:3].copy(), b[3:].copy()


def transition(x0, t, gyro, acc, g, noise=ih.DEFAULT_NOISE, dtype=np.float64):
    """(end state, Phi = F_{m-1} ... F_1, N) of the dead reckoning from x0: imuprop_helpers.jacobians step by step and propagate from P0 = 0."""
    x = tuple(np.asarray(y, dtype) for y in x0)
    Phi = np.eye(15, dtype=dtype)
    for j in range(1, len(t)):
        dt = np.float64(int(t[j]) - int(t[j - 1])) * np.float64(1e-9)
        F, _ = ih.jacobians(x, gyro[j - 1], acc[j - 1], gyro[j], acc[j], dt, dtype)
        Phi = F @ Phi
        x = ih.step(x, gyro[j - 1], acc[j - 1], gyro[j], acc[j], dt, g, dtype)
    xs, Ps = ih.propagate(x0, np.zeros((15, 15)), t, gyro, acc, g, noise, dtype)
    return xs[-1], Phi, Ps[-1]


def row_pose(xe, w_e, delta):
    """(R_I(tau), p_I(tau)): the constant-rate extrapolation of the end state over the read-out."""
    R, p, v = (np.asarray(y, np.float64) for y in xe[:3])
    return R @ ih.so3_exp(np.asarray(w_e, np.float64) * delta), p + delta * v


def camera_point(w, X, xe, w_e, row):
    RI, pI = row_pose(xe, w_e, delta_of(w, row))
    RC = RI @ Rot.from_quat(np.asarray(w.q_CI, float)).as_matrix()
    return RC.T @ (X - (pI + RI @ np.asarray(w.p_CI, float)))


def predict_from(w, l, xe, w_e, row, row_model=None):
    """(proj3, final row, status) for a GIVEN end state (None: the start time was outside the spline)."""
    X, st = lh.point(w, l)
    if st != lh.OK or xe is None:
        return NAN3.copy(), -1, NONE
    row = int(row)
    its = int(row_model[3]) if row_model is not None else 0
    for it in range(its + 1):
        y = camera_point(w, X, xe, w_e, row)
        if not np.isfinite(y).all() or not y[2] > 0:
            return NAN3.copy(), -1, NONE
        if it < its:
            fy, cy, rows = float(row_model[0]), float(row_model[1]), int(row_model[2])
            row = int(min(max(np.rint(fy * y[1] / y[2] + cy), 0.0), rows - 1.0))
    return np.array([y[0] / y[2], y[1] / y[2], y[2]]), row, OK


def end_of(w, frame, t, gyro, acc):
    """(end state or None, w_e) of a prediction on the window's own state."""
    x0 = start_state(w, int(t[0]), frame)
    if x0 is None:
        return None, None
    xs, _ = ih.propagate(x0, None, t, gyro, acc, w.gravity, cov=False)
    return xs[-1], np.asarray(gyro[-1], float) - np.asarray(xs[-1][3], float)


def predict(w, l, frame, t, gyro, acc, row, row_model=None):
    """(proj3, final row, status): the value of the entry."""
    xe, w_e = end_of(w, frame, t, gyro, acc)
    return predict_from(w, l, xe, w_e, row, row_model)


def B_matrix(w_e, delta):
    """(6 x 15): the body pose at the row time against the end state's tangent (dtheta, dp, dv, dbg, dba)."""
    B = np.zeros((6, 15))
    B[0:3, ih.TH] = ih.so3_exp(np.asarray(w_e, float) * delta).T
    B[0:3, ih.BG] = -delta * ih.so3_jr(np.asarray(w_e, float) * delta)
    B[3:6, ih.PP] = np.eye(3)
    B[3:6, ih.VV] = delta * np.eye(3)
    return B


def C_ext(w, RI):
    """(6 x 6): body -> camera tangent map (posecov_helpers.pose_jacobian's extrinsic rule)."""
    C = np.zeros((6, 6))
    C[0:3, 0:3] = Rot.from_quat(np.asarray(w.q_CI, float)).as_matrix().T
    C[3:6, 0:3] = -RI @ ph.hat(np.asarray(w.p_CI, float))
    C[3:6, 3:6] = np.eye(3)
    return C


def A_matrix(w, y, RI, w_e, delta):
    """(A (2 x 15), Pi, R_C)."""
    RC = RI @ Rot.from_quat(np.asarray(w.q_CI, float)).as_matrix()
    Pi = np.array([[1.0, 0.0, -y[0] / y[2]], [0.0, 1.0, -y[1] / y[2]]]) / y[2]
    D = np.hstack([ph.hat(y), -RC.T])
    return Pi @ D @ C_ext(w, RI) @ B_matrix(w_e, delta), Pi, RC


def prediction_jacobian(w, l, frame, t, gyro, acc, row, noise=ih.DEFAULT_NOISE):
    """Analytic [Jp | j] at a GIVEN row: a namespace (proj, y, Jp (2, P), j (2,), J (2, P + L), A (2, 15), Phi, N, ANA = A N A^T, xe, w_e,
    delta, nav: navstate_helpers.nav_jacobian of the start, pa: lmpoint_helpers.point_jacobian, knots_a, knots_q, frame, const), or None where
    the value is not computable."""
    x0 = start_state(w, int(t[0]), frame)
    pa = lh.point_jacobian(w, l)
    if x0 is None or pa is None:
        return None
    xe, Phi, N = transition(x0, t, gyro, acc, w.gravity, noise)
    w_e = np.asarray(gyro[-1], float) - xe[3]
    proj, _, st = predict_from(w, l, xe, w_e, row)
    if st != OK:
        return None
    delta = delta_of(w, row)
    RI, pI = row_pose(xe, w_e, delta)
    y = camera_point(w, pa.X, xe, w_e, row)
    A, Pi, RC = A_matrix(w, y, RI, w_e, delta)
    nav = nh.nav_jacobian(w, int(t[0]), frame)
    M = Pi @ RC.T
    Jn = A @ Phi @ nav.J
    Ja = M @ pa.Jp
    Jp = Jn + Ja
    RCI = Rot.from_quat(np.asarray(w.q_CI, float)).as_matrix()
    p_CI = np.asarray(w.p_CI, float)
    Jp[:, w.P - 1] += int(row) * (Pi @ (np.cross(y, RCI.T @ w_e) - RC.T @ (xe[2] + RI @ np.cross(w_e, p_CI))))
    j = M @ pa.jrho
    J = np.zeros((2, w.P + w.L))
    J[:, :w.P] = Jp
    J[:, w.P + l] = j
    return SimpleNamespace(proj=proj, y=y, Jp=Jp, j=j, J=J, A=A, Phi=Phi, N=N, ANA=A @ N @ A.T, xe=xe, w_e=w_e, delta=delta, nav=nav, pa=pa, Ja=Ja, Jn=Jn,
                           knots_a=pa.knots, knots_q=nav.knots, frame=nav.frame, row=int(row),
                           const=np.asarray(ch.constant_mask(w)).reshape(-1)[:w.P])


def kept_jacobian(ref, pj, l):
    """[Jp | j] restricted to the unknowns of ref.Sig (the excluded trajectory unknowns contribute nothing)."""
    J = np.zeros((2, ref.kp.shape[0] + ref.kl.shape[0]))
    J[:, :ref.kp.shape[0]] = pj.Jp[:, ref.kp]
    J[:, ref.kp.shape[0] + int(np.nonzero(ref.kl == l)[0][0])] = pj.j
    return J


def no_info(ref, pj, l, K):
    """The status-2 rule: Hll_l == 0, or a non-constant unknown no factor touches under the anchor knots, the knots of the start time or the
    chosen bias state."""
    free_untouched = (np.diag(ref.Hpp) == 0.0) & ~pj.const
    b0 = 6 * K + 6 * pj.frame
    return bool(not ref.Hll[l] > 0 or any(free_untouched[6 * k:6 * k + 6].any() for k in list(pj.knots_a) + list(pj.knots_q)) or free_untouched[b0:b0 + 6].any())


def pred_cov_reference(ref, pj, l, K, route="full", noise_part=True):
    """(2 x 2, status) on a lmpoint_helpers.joint_reference.  pj None: NaN, NONE.  The status-2 rule: +inf on the diagonal and 0 elsewhere.
    route "full": J Sigma J^T over the joint covariance; "schur": (L^-1 G)^T (L^-1 G) + j j^T / Hll with G = Jp^T - w_l j^T / Hll; both + A N A^T."""
    if pj is None:
        return np.full((2, 2), np.nan), NONE
    if no_info(ref, pj, l, K):
        return np.diag(np.full(2, np.inf)), NO_INFO
    h = ref.Hll[l]
    if route == "full":
        J = kept_jacobian(ref, pj, l)
        c = J @ ref.Sig @ J.T
    else:
        G = pj.Jp[:, ref.kp].T - np.outer(ref.W[ref.kp, l], pj.j) / h
        Y = np.linalg.solve(ref.Lc, G)
        c = Y.T @ Y + np.outer(pj.j, pj.j) / h
    return (c + pj.ANA if noise_part else c), OK


def recurrence_d(pj_inputs):
    """d of tests/test_gpu_imu_predict.py's bound, measured on THIS helper's Phi and N: the worst entry metric between float64 and longdouble of
    N and of Phi S Phi^T for S = I (every column of Phi enters with weight one)."""
    x0, t, gyro, acc, g, noise = pj_inputs
    _, P64, N64 = transition(x0, t, gyro, acc, g, noise)
    _, Pl, Nl = transition(x0, t, gyro, acc, g, noise, dtype=np.longdouble)
    d = ih.entry_metric(P64 @ P64.T, Pl @ Pl.T)
    if np.diag(Nl).max() > 0:
        d = max(d, ih.entry_metric(N64, Nl))
    return d


def bound(ref, pj, l, d, m):
    """(tolerance, g, share): cov_helpers.bound(kappa_s) g for the state part, g = posecov_helpers.amplification of [Jp | j] over the joint
    covariance, plus the recurrence bound 64 max(d, 15 m 2^-53) of tests/test_gpu_imu_predict.py scaled by the share of A N A^T in the block
    (max over the diagonal of (A N A^T)_aa / Cov_aa); with m = 1 there is no recurrence and the second term is zero."""
    J = kept_jacobian(ref, pj, l)
    g = ph.amplification(J, ref.Sig)
    c = J @ ref.Sig @ J.T + pj.ANA
    share = float(np.max(np.diag(pj.ANA) / np.diag(c))) if m > 1 else 0.0
    rec = 64 * max(d, 15 * m * 2.0 ** -53) if m > 1 else 0.0
    return ch.bound(ref.kappa) * g + rec * share, g, share
