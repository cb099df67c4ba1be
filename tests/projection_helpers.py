"""NumPy fp64 reference of ctvio_project_landmarks_batch (tests/test_projection_reference.py, tests/test_projjac_host.py,
tests/test_gpu_project_landmarks.py).

Definition (include/ctvio.h): landmark l anchored as in tests/lmpoint_helpers.py (X = R_C(tau_i) p_i / rho + p_C(tau_i)); with
tau_q = t + row * int(ld * 1e9) and the camera pose T_Cq = T_I(tau_q) (q_CI, p_CI): y = R_Cq^T (X - p_Cq), proj = (y.x / y.z, y.y / y.z, y.z).
Cov(proj.xy) = J Sigma J^T with J = [Jp | j] (2 x (P + L)) over the joint covariance of lmpoint_helpers.joint_reference.  With
Pi = (1 / y.z) [[1, 0, -z0], [0, 1, -z1]] and M = Pi R_Cq^T: Jp = M Jp_X (lmpoint_helpers.point_jacobian, line-delay column included)
+ Pi ([y]x J_theta - R_Cq^T J_p) (posecov_helpers.pose_jacobian with the camera extrinsic at tau_q) + row_q Pi ([y]x omega_C - R_Cq^T v_C) in
the line-delay column; j = M j_rho.  The row of a query may be iterated first: row <- clamp(rint(fy y.y / y.z + cy), 0, rows - 1).
"""
from types import SimpleNamespace

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import cov_helpers as ch
import lmpoint_helpers as lh
import posecov_helpers as ph

OK, SINGULAR, NO_INFO, NONE = 0, 1, 2, 3
NAN3 = np.full(3, np.nan)


def query_time(w, t_ns, row):
    """The time exactly as the factors take it: the line delay truncated to integer ns."""
    return int(t_ns) + int(row) * int(np.int64(w.ld * 1e9))


def camera_point(w, X, tau_q):
    """y = R_Cq^T (X - p_Cq) from the oracle's NumPy spline evaluation, or None outside the spline."""
    if not ph.segment(w, tau_q)[2]:
        return None
    R, p = ph.pose_numpy(w, tau_q, w.q_CI, w.p_CI)
    return R.inv().apply(X - p)


def project(w, l, t_ns, row, row_model=None):
    """(proj3, final row, status).  row_model = (fy, cy, rows, iterations): the row iteration of the entry.  NONE (NaN, row -1): the landmark
    is not computable, or at any row visited tau_q is outside the spline or y.z <= 0 or y is not finite."""
    X, st = lh.point(w, l)
    if st != lh.OK:
        return NAN3.copy(), -1, NONE
    row = int(row)
    its = int(row_model[3]) if row_model is not None else 0
    for it in range(its + 1):
        y = camera_point(w, X, query_time(w, t_ns, row))
        if y is None or not np.isfinite(y).all() or not y[2] > 0:
            return NAN3.copy(), -1, NONE
        if it < its:
            fy, cy, rows = float(row_model[0]), float(row_model[1]), int(row_model[2])
            row = int(min(max(np.rint(fy * y[1] / y[2] + cy), 0.0), rows - 1.0))
    return np.array([y[0] / y[2], y[1] / y[2], y[2]]), row, OK


def projection_jacobian(w, l, t_ns, row):
    """Analytic [Jp | j] at a GIVEN row: a namespace (proj (3,), y, Jp (2, P), j (2,), J (2, P + L), Ja / Jq: the anchor / query knot terms
    alone (2, P), tau_q, row, knots: the knots either time depends on, const: cov_helpers.constant_mask), or None where the projection is not
    computable."""
    import np_oracle
    proj, _, st = project(w, l, t_ns, row)
    if st != OK:
        return None
    pa = lh.point_jacobian(w, l)
    tau_q = query_time(w, t_ns, row)
    jq = ph.pose_jacobian(w, tau_q, w.q_CI, w.p_CI)
    RCI = Rot.from_quat(np.asarray(w.q_CI, float)).as_matrix()
    p_CI = np.asarray(w.p_CI, float)
    RCq = jq.R @ RCI
    y = RCq.T @ (pa.X - (jq.p + jq.R @ p_CI))
    Pi = np.array([[1.0, 0.0, -y[0] / y[2]], [0.0, 1.0, -y[1] / y[2]]]) / y[2]
    M = Pi @ RCq.T
    Ja = M @ pa.Jp
    Jq = Pi @ (ph.hat(y) @ jq.J[0:3] - RCq.T @ jq.J[3:6])
    Jp = Ja + Jq
    idt = 1e9 / w.dt_ns
    sa, ua = np.array([jq.s]), np.array([jq.u])
    _, om = np_oracle._rot_eval(w.quat, sa, ua, idt, True)
    v = np_oracle._pos_eval(w.pos, sa, ua, idt, 1)[0]
    om_C = RCI.T @ om[0]
    v_C = v + jq.R @ np.cross(om[0], p_CI)
    Jp[:, w.P - 1] += int(row) * (Pi @ (np.cross(y, om_C) - RCq.T @ v_C))
    j = M @ pa.jrho
    J = np.zeros((2, w.P + w.L))
    J[:, :w.P] = Jp
    J[:, w.P + l] = j
    Ja = Ja.copy(); Ja[:, w.P - 1] = 0.0
    return SimpleNamespace(proj=proj, y=y, Jp=Jp, j=j, J=J, Ja=Ja, Jq=Jq, tau_q=tau_q, row=int(row), knots=sorted(set(pa.knots) | set(jq.knots)),
                           knots_a=pa.knots, knots_q=jq.knots, s_a=pa.s, s_q=jq.s, u_q=jq.u, const=np.asarray(ch.constant_mask(w)).reshape(-1)[:w.P])


def kept_jacobian(ref, pj, l):
    """[Jp | j] restricted to the unknowns of ref.Sig (the excluded trajectory unknowns contribute nothing)."""
    J = np.zeros((2, ref.kp.shape[0] + ref.kl.shape[0]))
    J[:, :ref.kp.shape[0]] = pj.Jp[:, ref.kp]
    J[:, ref.kp.shape[0] + int(np.nonzero(ref.kl == l)[0][0])] = pj.j
    return J


def proj_cov_reference(ref, pj, l, route="full"):
    """(2 x 2, status) on a lmpoint_helpers.joint_reference.  pj None: NaN, NONE.  Hll == 0, or a knot either time depends on with an
    untouched, non-constant unknown: +inf on the diagonal and 0 elsewhere, NO_INFO.  route "full": J Sigma J^T over the joint covariance;
    "schur": (L^-1 G)^T (L^-1 G) + j j^T / Hll with G = Jp^T - w_l j^T / Hll, the identity the device uses, with numpy.linalg.cholesky."""
    if pj is None:
        return np.full((2, 2), np.nan), NONE
    h = ref.Hll[l]
    free_untouched = (np.diag(ref.Hpp) == 0.0) & ~pj.const
    if not h > 0 or any(free_untouched[6 * k:6 * k + 6].any() for k in pj.knots):
        return np.diag(np.full(2, np.inf)), NO_INFO
    if route == "full":
        J = kept_jacobian(ref, pj, l)
        return J @ ref.Sig @ J.T, OK
    G = pj.Jp[:, ref.kp].T - np.outer(ref.W[ref.kp, l], pj.j) / h
    Y = np.linalg.solve(ref.Lc, G)
    return Y.T @ Y + np.outer(pj.j, pj.j) / h, OK


def bound(ref, pj, l):
    """(tolerance, g): cov_helpers.bound(kappa_s) * g with g = posecov_helpers.amplification of [Jp | j] over the joint covariance."""
    g = ph.amplification(kept_jacobian(ref, pj, l), ref.Sig)
    return ch.bound(ref.kappa) * g, g


def chi2_reference(proj, cov, obs, img_w):
    """(e^T (Cov + I / img_w^2)^-1 e, kappa_2 of the 2 x 2) from the given bits, in extended precision."""
    A = np.asarray(cov, np.longdouble).reshape(2, 2) + np.eye(2, dtype=np.longdouble) / (np.longdouble(img_w) * np.longdouble(img_w))
    e = np.asarray(obs, np.longdouble).reshape(2) - np.asarray(proj, np.longdouble).reshape(-1)[:2]
    det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    val = (A[1, 1] * e[0] * e[0] - (A[0, 1] + A[1, 0]) * e[0] * e[1] + A[0, 0] * e[1] * e[1]) / det
    ev = np.linalg.eigvalsh(np.asarray(A, float))
    return float(val), float(ev[-1] / ev[0])


def value_atol(w, proj):
    """Tolerances of proj3 against the helper: xy (a point error of lmpoint_helpers.point_atol at the query depth, through Pi) and depth."""
    a = lh.point_atol(w)
    z = np.abs(proj[:2])
    return a / proj[2] * (1.0 + z.max()) + 1e-12 * z, a
