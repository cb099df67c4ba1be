"""NumPy fp64 reference of ctvio_imu_gate_batch (tests/test_imugate_reference.py, tests/test_gpu_imu_gate.py).

Definition (include/ctvio.h): sample m = (t, bias state b, gyro, acc) of the window itself, w = imu_w.  z = (omega(t) + bg_b, f(t) + ba_b)
(rates_helpers.rates_numpy), r = w (z - meas); J = w (the omega and f rows of rates_helpers.rates_jacobian plus its one-hot bias rows), 6 x P;
A = J Sigma J^T on a lmpoint_helpers.joint_reference (excluded unknowns contribute nothing); redundancy = lambda_min(I - A);
C_loo = (I - A)^-1 - I; chi2 = r^T (I - A)^-1 r.  Statuses: 2 an untouched non-constant unknown under the sample's knots or bias state,
4 redundancy < min_redundancy (1, a failed factorisation, has no reference; 3 cannot occur).  brute_force() is the independent route:
H minus the sample's own J^T J, Jacobi-scaled and inverted.

The tolerance, hat_bound = cov_helpers.bound(kappa_s) |A|_2, is NORM-WISE and carries no row amplification: J^T J <= H gives
|Hs^-1/2 Js^T|^2 = |A|, so |Hs^-1 Js^T|^2 <= |A| / lambda_min(Hs), and a backward error E of the factorisation (|E| <= 4 * 2^-53 |Hs|) moves
A = Js Hs^-1 Js^T by at most |E| |Hs^-1 Js^T|^2 <= 4 * 2^-53 kappa_s |A|.  (The entrywise bound of the body-rates test would multiply by the
f rows' amplification, which reaches 1e6 on these windows: vacuous.)
"""
from types import SimpleNamespace

import numpy as np

import cov_helpers as ch
import rates_helpers as rh
import visgate_helpers as vg

OK, SINGULAR, NO_INFO, WEAK = 0, 1, 2, 4
EPS = 2.0 ** -53
STEP = 64 * EPS          # the 6 x 6 step's own rounding, absolute on the redundancy (the entries of I - A are at most 1)
INF6 = np.diag(np.full(6, np.inf))


def sample_values(w, m):
    """(z, r) of sample m: the predicted reading and the whitened residual."""
    rates, bias = rh.rates_numpy(w, int(w.imu_t[m]), int(w.imu_bias[m]))
    z = rates[:6] + bias
    meas = np.concatenate([w.imu_gyro[m], w.imu_acc[m]])
    return z, np.asarray(w.imu_w, float) * (z - meas)


def sample_jacobian(w, m):
    """(6 x P whitened Jacobian of the residual of sample m, the rates_jacobian namespace)."""
    jac = rh.rates_jacobian(w, int(w.imu_t[m]), int(w.imu_bias[m]))
    assert jac is not None
    return (jac.J[0:6] + jac.J[9:15]) * np.asarray(w.imu_w, float)[:, None], jac


def kept(ref, J6):
    """J over the unknowns of ref.Sig (the excluded trajectory unknowns contribute nothing; the landmarks' columns are zero)."""
    J = np.zeros((6, ref.kp.shape[0] + ref.kl.shape[0]))
    J[:, :ref.kp.shape[0]] = J6[:, ref.kp]
    return J


def hat_bound(ref, A):
    """cov_helpers.bound(kappa_s) |A|_2 (see the module's docstring)."""
    return ch.bound(ref.kappa) * float(np.linalg.norm(A, 2))


def sample_reference(w, ref, m, min_red=0.01):
    """The reference of sample m on a lmpoint_helpers.joint_reference (None: values only): a namespace (m, frame, status, z, res, J: kept,
    A, redundancy, cov, chi2, tol: hat_bound)."""
    z, r = sample_values(w, m)
    out = SimpleNamespace(m=m, frame=int(w.imu_bias[m]), status=OK, z=z, res=r, J=None, A=None, redundancy=np.nan, cov=np.full((6, 6), np.nan),
                          chi2=np.nan, tol=0.0)
    if ref is None:
        return out
    J6, jac = sample_jacobian(w, m)
    idx = [j for k in jac.knots for j in range(6 * k, 6 * k + 6)] + list(range(6 * w.K + 6 * out.frame, 6 * w.K + 6 * out.frame + 6))
    const, untouched = ch.constant_mask(w), np.diag(ref.Hpp) == 0.0
    if any(untouched[j] and not const[j] for j in idx):
        out.status, out.redundancy, out.cov, out.chi2 = NO_INFO, 0.0, INF6.copy(), 0.0
        return out
    out.J = kept(ref, J6)
    A = out.J @ ref.Sig @ out.J.T
    out.A = 0.5 * (A + A.T)
    out.tol = hat_bound(ref, out.A)
    M = np.eye(6) - out.A
    out.redundancy = float(np.linalg.eigvalsh(M)[0])
    if out.redundancy < min_red:
        out.status, out.cov, out.chi2 = WEAK, INF6.copy(), 0.0
        return out
    Mi = np.linalg.inv(M)
    out.cov = 0.5 * (Mi + Mi.T) - np.eye(6)
    out.chi2 = float(r @ np.linalg.solve(M, r))
    return out


def chi2_of(res, A):
    """r^T (I - A)^-1 r from given bits."""
    return float(res @ np.linalg.solve(np.eye(6) - A, res))


def cov_error(C, ref_cov):
    """|C - ref|_2 / |ref + I|_2: the metric of cov36 (|ref + I|_2 = 1 / redundancy)."""
    return float(np.linalg.norm(np.asarray(C) - ref_cov, 2) / np.linalg.norm(ref_cov + np.eye(6), 2))


def brute_force(w, ref, b):
    """(J (H - J^T J)^-1 J^T, its norm-wise bound relative to |C|_2, kappa of the downdated scaled system): the downdated system inverted
    after Jacobi scaling, as joint_reference inverts the full one.  The bound is hat_bound's argument on the downdated system:
    |Hd_s^-1 Js^T|^2 <= |C| / lambda_min(Hd_s), so the error is at most cov_helpers.bound(kappa_d) |C|_2."""
    Hd = vg.kept_system(ref) - b.J.T @ b.J
    d = 1.0 / np.sqrt(np.diag(Hd))
    Hs = Hd * np.outer(d, d)
    Hs = 0.5 * (Hs + Hs.T)
    ev = np.linalg.eigvalsh(Hs)
    kappa = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
    Sig = np.linalg.inv(Hs) * np.outer(d, d)
    C = b.J @ Sig @ b.J.T
    return 0.5 * (C + C.T), ch.bound(kappa), kappa, Sig


def frame_reference(w, samples):
    """frame_stats (F, 4) from per-sample references: the number of status-0 samples naming the bias state, their mean chi2 (NaN: none), the
    largest chi2 (0: none), the smallest redundancy over status 0 or 4 (+inf: none)."""
    st = np.zeros((w.F, 4))
    for f in range(w.F):
        mine = [b for b in samples if b.frame == f]
        chis = [b.chi2 for b in mine if b.status == OK]
        reds = [b.redundancy for b in mine if b.status in (OK, WEAK)]
        st[f] = (len(chis), np.mean(chis) if chis else np.nan, max(chis) if chis else 0.0, min(reds) if reds else np.inf)
    return st
