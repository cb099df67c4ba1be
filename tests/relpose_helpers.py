"""NumPy fp64 reference of ctvio_relative_pose_batch (tests/test_relpose_reference.py, tests/test_relpose_host.py,
tests/test_gpu_relative_pose.py).

Definition (include/ctvio.h): with (R_a, p_a), (R_b, p_b) the poses at t_a and t_b (body, or T_I(t) T_SI), R_ab = R_a^T R_b and p_ab =
R_a^T (p_b - p_a).  Sigma_rel = J_rel Sigma J_rel^T with Sigma the covariance of the trajectory unknowns (tests/cov_helpers.py) and
  J_rel = A_a J_a + A_b J_b,   A_a = [[-R_ab^T, 0], [[p_ab]x, -R_a^T]],   A_b = [[I, 0], [0, R_a^T]],
J_a, J_b the 6 x P pose Jacobians of tests/posecov_helpers.py at the two times; tangent (dtheta 0..2, dp 3..5) of R_ab <- R_ab exp(dtheta),
p_ab <- p_ab + dp (dp in frame a).
"""
from types import SimpleNamespace

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import navstate_helpers as nh
import posecov_helpers as ph
from posecov_helpers import OK, OUTSIDE, SINGULAR, UNTOUCHED, segment, time_of   # noqa: F401  (the statuses and the time rule are the pose entry's)

CAP = 1e-3            # what every check asserts on its own bound: the errors these tests exist to catch (a wrong sign, R_ab for R_ab^T, the wrong
                      # frame for dp, a missing overlap sum) are O(1) to O(0.1)
OFF = ~np.eye(6, dtype=bool)


def _sensor(jac, q_SI, p_SI):
    """(R, p) of the pose a posecov_helpers.pose_jacobian result describes: jac.R, jac.p are the body's."""
    if q_SI is None:
        return jac.R, jac.p
    q = np.asarray(q_SI, float)
    return jac.R @ Rot.from_quat(q / np.linalg.norm(q)).as_matrix(), jac.p + jac.R @ np.asarray(p_SI, float)


def rel_jacobian(w, t_a, t_b, q_SI=None, p_SI=None):
    """The 6 x P Jacobian of the increment between absolute times t_a and t_b of window w.  Returns a namespace (J, a, b: the two pose_jacobian
    results, knots: the sorted union of the knots both poses depend on, R_ab, p_ab, R_a), or None where either time is outside the spline."""
    a, b = ph.pose_jacobian(w, t_a, q_SI, p_SI), ph.pose_jacobian(w, t_b, q_SI, p_SI)
    if a is None or b is None:
        return None
    Ra, pa = _sensor(a, q_SI, p_SI)
    Rb, pb = _sensor(b, q_SI, p_SI)
    R_ab, p_ab = Ra.T @ Rb, Ra.T @ (pb - pa)
    A_a, A_b = np.zeros((6, 6)), np.eye(6)
    A_a[0:3, 0:3] = -R_ab.T
    A_a[3:6, 0:3] = ph.hat(p_ab)
    A_a[3:6, 3:6] = -Ra.T
    A_b[3:6, 3:6] = Ra.T
    return SimpleNamespace(J=A_a @ a.J + A_b @ b.J, a=a, b=b, knots=sorted(set(a.knots) | set(b.knots)), R_ab=R_ab, p_ab=p_ab, R_a=Ra)


def rel_numpy(w, t_a, t_b, q_SI=None, p_SI=None):
    """(R_ab as a Rotation, p_ab) from the oracle's NumPy spline evaluation (posecov_helpers.pose_numpy)."""
    q = None if q_SI is None else np.asarray(q_SI, float) / np.linalg.norm(q_SI)
    Ra, pa = ph.pose_numpy(w, t_a, q, p_SI)
    Rb, pb = ph.pose_numpy(w, t_b, q, p_SI)
    return Ra.inv() * Rb, Ra.inv().apply(pb - pa)


def rel_cov_reference(ref, jac, route="full"):
    """The status and zero rules on a cov_helpers.cov_reference result over ALL P unknowns (sel = range(P)): returns (6 x 6, status).
    jac None (either time outside the spline): NaN, 3.  A knot either pose depends on with an untouched, non-constant unknown: +inf on the
    diagonal and 0 elsewhere, 2.  Otherwise J Sigma J^T with the excluded unknowns' rows and columns zero (constant ones contribute nothing), 0."""
    if jac is None:
        return np.full((6, 6), np.nan), OUTSIDE
    free_untouched = ref.untouched & ~ref.const
    if any(free_untouched[6 * k:6 * k + 6].any() for k in jac.knots):
        return np.diag(np.full(6, np.inf)), UNTOUCHED
    Sig = np.array(ref.cov_full if route == "full" else ref.cov_schur)
    Sig[~np.isfinite(Sig)] = 0.0          # (+inf diagonals of untouched unknowns elsewhere in the window: J is zero there)
    return jac.J @ Sig @ jac.J.T, OK


row_amplification = nh.row_amplification


def entry_bounds(tol, g):
    """The 6 x 6 bound tol sqrt(g_a g_b)."""
    return tol * np.sqrt(np.outer(g, g))


entry_errors = nh.entry_errors
