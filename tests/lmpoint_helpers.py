"""NumPy fp64 reference of ctvio_landmark_points_batch (tests/test_lmpoint_reference.py, tests/test_gpu_landmark_points.py).

Definition (include/ctvio.h): landmark l is anchored at the observation (t_i, row_i, p_i = (x, y, 1)) all its visual blocks share; with
tau = t_i + row_i * int(ld * 1e9), x_c = p_i / rho and the camera pose T_C = T_I(tau) (q_CI, p_CI): X = R_C x_c + p_C.  Cov(X) = J Sigma J^T with
J = [Jp | j_rho] (3 x (P + L)) and Sigma the joint covariance of the trajectory unknowns and the inverse depths: H, the exclusions and the
+inf rule of tests/cov_helpers.py.  Jp = [-R_C [x_c]x, I] J_pose (tests/posecov_helpers.pose_jacobian with the camera extrinsic) on the knots of
tau, row_i (R_I [omega]x (R_CI x_c + p_CI) + v) in the line-delay column; j_rho = -R_C p_i / rho^2.
"""
from types import SimpleNamespace

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import cov_helpers as ch
import posecov_helpers as ph

OK, SINGULAR, NO_INFO, NONE = 0, 1, 2, 3


def anchor_of(w, l):
    """(t_i, row_i, p_i (3,)) of landmark l, or None: no visual block, or blocks that name more than one anchor observation."""
    idx = np.nonzero(np.asarray(w.v_lm) == l)[0]
    if idx.shape[0] == 0:
        return None
    obs = {(int(w.v_ti[v]), int(w.v_rowi[v]), float(w.v_pi[v, 0]), float(w.v_pi[v, 1])) for v in idx}
    if len(obs) != 1:
        return None
    t, row, x, y = obs.pop()
    return t, row, np.array([x, y, 1.0])


def anchor_time(w, t_i, row_i):
    """The time exactly as the factors take it: the line delay truncated to integer ns (np_oracle.residuals, trunc_ld)."""
    return int(t_i) + int(row_i) * int(np.int64(w.ld * 1e9))


def point_at(w, tau, p_i, rho):
    """X for an anchor time tau from the oracle's NumPy spline evaluation (posecov_helpers.pose_numpy with the camera extrinsic)."""
    R, p = ph.pose_numpy(w, tau, w.q_CI, w.p_CI)
    return R.apply(p_i / rho) + p


def point(w, l):
    """(X (3,), status): NaN and NONE by the rules of the entry (rho <= 0 or non-finite, no single anchor, tau outside the spline)."""
    a = anchor_of(w, l)
    rho = float(w.rho[l])
    if a is None or not (rho > 0 and np.isfinite(rho)):
        return np.full(3, np.nan), NONE
    tau = anchor_time(w, a[0], a[1])
    if not ph.segment(w, tau)[2]:
        return np.full(3, np.nan), NONE
    return point_at(w, tau, a[2], rho), OK


def point_jacobian(w, l):
    """Analytic [Jp | j_rho] of landmark l: a namespace (X, Jp (3, P), jrho (3,), J (3, P + L), tau, row, s, knots), or None where the point is
    not computable."""
    import np_oracle
    X, st = point(w, l)
    if st != OK:
        return None
    t_i, row, p_i = anchor_of(w, l)
    rho = float(w.rho[l])
    tau = anchor_time(w, t_i, row)
    jac = ph.pose_jacobian(w, tau, w.q_CI, w.p_CI)
    RCI = Rot.from_quat(np.asarray(w.q_CI, float)).as_matrix()
    RC = jac.R @ RCI
    x_c = p_i / rho
    Jp = -RC @ ph.hat(x_c) @ jac.J[0:3] + jac.J[3:6]
    idt = 1e9 / w.dt_ns
    sa, ua = np.array([jac.s]), np.array([jac.u])
    _, om = np_oracle._rot_eval(w.quat, sa, ua, idt, True)
    v = np_oracle._pos_eval(w.pos, sa, ua, idt, 1)[0]
    p_I = RCI @ x_c + np.asarray(w.p_CI, float)
    Jp[:, w.P - 1] = row * (jac.R @ np.cross(om[0], p_I) + v)
    jrho = -RC @ p_i / rho ** 2
    J = np.zeros((3, w.P + w.L))
    J[:, :w.P] = Jp
    J[:, w.P + l] = jrho
    return SimpleNamespace(X=X, Jp=Jp, jrho=jrho, J=J, tau=tau, row=row, s=jac.s, knots=jac.knots)


def joint_reference(Hpp, W, Hll, active):
    """Hpp (P, P), W (P, L), Hll (L,) as ctvio_linearize returns them; active: [P], non-zero where the unknown is NOT constant.  The joint
    covariance over (kept trajectory unknowns kp, landmarks kl with Hll > 0) by the Jacobi-scaled inverse of the un-eliminated system -- this
    route never uses the Schur identity -- and the Cholesky factor of the reduced system for the second route.  Returns a namespace (Sig, kp,
    kl, kappa, Lc, Hpp, W, Hll, P, L)."""
    Hpp = np.asarray(Hpp, float); Hll = np.asarray(Hll, float).reshape(-1)
    P, L = Hpp.shape[0], Hll.shape[0]
    W = np.asarray(W, float).reshape(P, L) if L else np.zeros((P, 0))
    const = ~(np.asarray(active).reshape(-1)[:P] != 0)
    untouched = np.diag(Hpp) == 0.0
    kp = np.nonzero(~const & ~untouched)[0]
    kl = np.nonzero(Hll > 0)[0]
    n = kp.shape[0] + kl.shape[0]
    H = np.zeros((n, n))
    H[:kp.shape[0], :kp.shape[0]] = Hpp[np.ix_(kp, kp)]
    H[:kp.shape[0], kp.shape[0]:] = W[np.ix_(kp, kl)]
    H[kp.shape[0]:, :kp.shape[0]] = W[np.ix_(kp, kl)].T
    H[kp.shape[0]:, kp.shape[0]:] = np.diag(Hll[kl])
    d = 1.0 / np.sqrt(np.diag(H))
    Hs = H * np.outer(d, d)
    Hs = 0.5 * (Hs + Hs.T)
    ev = np.linalg.eigvalsh(Hs)
    kappa = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
    Sig = np.linalg.inv(Hs) * np.outer(d, d)
    Wk = W[np.ix_(kp, kl)]
    S = Hpp[np.ix_(kp, kp)] - (Wk / Hll[kl]) @ Wk.T
    Lc = np.linalg.cholesky(0.5 * (S + S.T))
    return SimpleNamespace(Sig=Sig, kp=kp, kl=kl, kappa=kappa, Lc=Lc, Hpp=Hpp, W=W, Hll=Hll, P=P, L=L)


def kept_jacobian(ref, pj, l):
    """[Jp | j_rho] restricted to the unknowns of ref.Sig (the excluded trajectory unknowns contribute nothing)."""
    J = np.zeros((3, ref.kp.shape[0] + ref.kl.shape[0]))
    J[:, :ref.kp.shape[0]] = pj.Jp[:, ref.kp]
    J[:, ref.kp.shape[0] + int(np.nonzero(ref.kl == l)[0][0])] = pj.jrho
    return J


def point_cov_reference(ref, pj, l, route="full"):
    """(3 x 3, status) of landmark l.  pj None (point_jacobian: not computable): NaN, NONE.  Hll == 0: +inf on the diagonal and 0 elsewhere,
    NO_INFO.  route "full": J Sigma J^T over the joint covariance; "schur": (L^-1 G)^T (L^-1 G) + j_rho j_rho^T / Hll with
    G = Jp^T - w_l j_rho^T / Hll, the identity the device uses, with numpy.linalg.cholesky."""
    if pj is None:
        return np.full((3, 3), np.nan), NONE
    h = ref.Hll[l]
    if not h > 0:
        return np.diag(np.full(3, np.inf)), NO_INFO
    if route == "full":
        J = kept_jacobian(ref, pj, l)
        return J @ ref.Sig @ J.T, OK
    G = pj.Jp[:, ref.kp].T - np.outer(ref.W[ref.kp, l], pj.jrho) / h
    Y = np.linalg.solve(ref.Lc, G)
    return Y.T @ Y + np.outer(pj.jrho, pj.jrho) / h, OK


def bound(ref, pj, l):
    """(tolerance, g): cov_helpers.bound(kappa_s) * g with g = posecov_helpers.amplification of [Jp | j_rho] over the joint covariance."""
    g = ph.amplification(kept_jacobian(ref, pj, l), ref.Sig)
    return ch.bound(ref.kappa) * g, g


def point_atol(w):
    """The sensor-pose test's atol 1e-11 times max(1, the window's largest depth in metres): a rotation error acts at the lever arm."""
    r = np.asarray(w.rho, float)
    r = r[(r > 0) & np.isfinite(r)]
    return 1e-11 * max(1.0, float(np.max(1.0 / r)) if r.shape[0] else 1.0)
