"""Helpers of the blocked marginalisation tests (csrc/marg_blocked.hpp): the config-5 drop sets of the issue's windows, a NumPy
model of the device's block two-sided Jacobi schedule, and the yardsticks a prior is compared with.  The model restates what
csrc/jacobi_core.hpp holds for both device paths (rr_pair, jacobi_cs, jacobi_converged) independently: it does not call the C++, and
tests/test_jacobi_core_host.py compares the two."""
import importlib

import numpy as np

cv = importlib.import_module("ctrl-vio_amd")

BLK = 32                     # MB_BLK: columns per block; a block pair is one 64 x 64 sub-problem
MAX_SWEEPS = 40              # MB_MAX_SWEEPS


def anchor_frames(w):
    """Frame index of every landmark's anchor (-1: no visual block)."""
    frames = np.unique(np.concatenate([w.v_ti, w.v_tj]))
    a = -np.ones(w.L, np.int64)
    a[w.v_lm] = np.searchsorted(frames, w.v_ti)
    return a


def drop_roles(w, drop_frames, keep_frames=None):
    """MARGIN_OLD-like role: knots 0-1 and bias state 0 marginalised, with the landmarks anchored in `drop_frames`; every other pose
    unknown kept, plus the landmarks anchored in `keep_frames`; the remaining landmarks are not involved (-1)."""
    a = anchor_frames(w)
    role = np.zeros(w.N, np.int8)
    role[:12] = 1
    role[6 * w.K:6 * w.K + 6] = 1
    lr = np.full(w.L, -1, np.int8)
    lr[np.isin(a, drop_frames)] = 1
    if keep_frames is not None:
        lr[np.isin(a, keep_frames)] = 0
    role[w.P:] = lr
    return role


def config5_window(seed=1500):
    w = cv.synth.make_window("config5", seed=seed)
    w.cauchy_a = 1.0                   # the reference marginalises with CauchyLoss(1.0)
    return w


# ---------------------------------------------------------------- model of the device schedule

def rr_pair(np_, s, i):
    """jacobi_core.hpp rr_pair: round-robin tournament over np_ players, step s, pair i -> (p < q)."""
    r = np_ - 1
    if i == 0:
        a, b = r, s
    else:
        a, b = (s + i) % r, (s + r - i) % r
    return min(a, b), max(a, b)


def jacobi_cs(app, aqq, apq):
    """jacobi_core.hpp jacobi_cs on arrays of pivots: (c, s) of the rotation that annihilates apq; the identity where apq = 0."""
    c = np.ones(apq.shape); sn = np.zeros(apq.shape)
    nz = apq != 0.0
    theta = (aqq[nz] - app[nz]) / (2.0 * apq[nz])
    with np.errstate(over="ignore"):               # theta^2 = inf gives tt = 0, as on the device
        tt = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c[nz] = 1.0 / np.sqrt(tt * tt + 1.0); sn[nz] = tt * c[nz]
    return c, sn


def inner_sweep(T):
    """One parallel cyclic Jacobi sweep on the 64 x 64 sub-problem T (in place): k_mb_pair, i.e. one sweep of jacobi_packed (jacobi_cs,
    jacobi_diag_update, jacobi_block_update, rotate_cols of jacobi_core.hpp).  Returns Q with T_out = Q^T T_in Q."""
    d = T.shape[0]
    Q = np.eye(d)
    pairs = [np.array([rr_pair(d, s, i) for i in range(d // 2)]) for s in range(d - 1)]
    for pq in pairs:
        p, q = pq[:, 0], pq[:, 1]
        apq, app, aqq = T[q, p], T[p, p], T[q, q]
        c, sn = jacobi_cs(app, aqq, apq)
        dpp = c * c * app - 2.0 * c * sn * apq + sn * sn * aqq
        dqq = sn * sn * app + 2.0 * c * sn * apq + c * c * aqq
        for M in (T,):
            Mp, Mq = M[:, p].copy(), M[:, q].copy()
            M[:, p] = c * Mp - sn * Mq; M[:, q] = sn * Mp + c * Mq
            Mp, Mq = M[p, :].copy(), M[q, :].copy()
            M[p, :] = c[:, None] * Mp - sn[:, None] * Mq; M[q, :] = sn[:, None] * Mp + c[:, None] * Mq
        T[p, p] = dpp; T[q, q] = dqq; T[p, q] = 0.0; T[q, p] = 0.0
        Qp, Qq = Q[:, p].copy(), Q[:, q].copy()
        Q[:, p] = c * Qp - sn * Qq; Q[:, q] = sn * Qp + c * Qq
    return Q


def converged(off, d2, nd, sweep, prev_off):
    """jacobi_core.hpp jacobi_converged (the oracle's rule, with its rounding-floor clause), restated."""
    floor_rel = max(1e-28, 4.0 * nd * nd * 4.93e-32)
    return off <= 1e-60 or off <= 1e-32 * d2 or (sweep >= 12 and off <= floor_rel * d2 and off > 0.25 * prev_off)


def padded(nd):
    return max(64, (nd + 63) // 64 * 64)


def block_jacobi(A):
    """Block two-sided Jacobi as the device runs it.  A: (nd, nd) symmetric.  Returns (eigenvalues, V, sweeps): A = V diag(e) V^T,
    unsorted; padded columns dropped."""
    nd = A.shape[0]
    D = padded(nd)
    nb = D // BLK
    B = np.zeros((D, D)); B[:nd, :nd] = A
    V = np.eye(D)
    prev = 1e300
    for sweep in range(MAX_SWEEPS):
        off = float(np.sum(np.tril(B, -1) ** 2)); d2 = float(np.sum(np.diag(B) ** 2))
        if converged(off, d2, nd, sweep, prev):
            return np.diag(B)[:nd].copy(), V[:nd, :nd].copy(), sweep
        prev = off
        for s in range(nb - 1):
            groups = []
            for i in range(nb // 2):
                p, q = rr_pair(nb, s, i)
                idx = np.r_[p * BLK:(p + 1) * BLK, q * BLK:(q + 1) * BLK]
                T = B[np.ix_(idx, idx)].copy()
                Q = inner_sweep(T)
                groups.append((idx, Q, T))
            for idx, Q, _ in groups:                 # column phase, then row phase
                B[:, idx] = B[:, idx] @ Q
                V[:, idx] = V[:, idx] @ Q
            for idx, Q, _ in groups:
                B[idx, :] = Q.T @ B[idx, :]
            for idx, _, T in groups:                 # the diagonal sub-problems keep their in-LDS rotation
                B[np.ix_(idx, idx)] = T
    raise RuntimeError("block Jacobi did not converge")


def blocked_marginalize(H, g, role, eps=1e-8):
    """MarginalizationInfo::marginalize with both eigen-problems on block_jacobi: kept, J0 (rows in ascending eigenvalue order), r0."""
    im = np.where(role == 1)[0]; ik = np.where(role == 0)[0]
    n = ik.size
    Amr = H[np.ix_(im, ik)]
    if im.size:
        em, Vm, _ = block_jacobi(H[np.ix_(im, im)])
        inv = np.where(em > eps, 1.0 / np.where(em > eps, em, 1.0), 0.0)
        X = Vm @ (inv[:, None] * (Vm.T @ np.c_[Amr, g[im]]))
        Ap = H[np.ix_(ik, ik)] - Amr.T @ X[:, :n]
        Ap = 0.5 * (Ap + Ap.T)
        bp = g[ik] - Amr.T @ X[:, n]
    else:
        Ap, bp = H[np.ix_(ik, ik)].copy(), g[ik].copy()
    e, V, _ = block_jacobi(Ap)
    order = np.lexsort((np.arange(n), e))
    S = np.where(e > eps, e, 0.0)
    J0 = (np.sqrt(S)[:, None] * V.T)[order]
    r0 = np.where(S > 0, (V.T @ bp) / np.sqrt(np.where(S > 0, S, 1.0)), 0.0)[order]
    return ik, J0, r0


# ---------------------------------------------------------------- yardsticks

def prior_errors(J0, r0, Jo, ro):
    """(J0^T J0 relative to its largest entry, J0^T r0 relative, J0^T J0 after diagonal scaling max |dH_ij| / sqrt(H_ii H_jj)).  The
    scaling floors H_ii at eps = 1e-8, the absolute resolution of the prior (an unknown the prior does not constrain has H_ii = 0)."""
    Ha, Ho = J0.T @ J0, Jo.T @ Jo
    ga, go = J0.T @ r0, Jo.T @ ro
    dH = np.abs(Ha - Ho)
    dg = np.sqrt(np.maximum(np.diag(Ho), 1e-8))
    return (dH.max() / np.abs(Ho).max(), np.abs(ga - go).max() / max(np.abs(go).max(), 1e-300),
            (dH / np.outer(dg, dg)).max())


def rank(J0):
    return int(np.count_nonzero(np.any(J0 != 0.0, axis=1)))


def near_eps(J0, eps=1e-8):
    """The kept eigenvalues of A' within 10x of eps (squared row norms of J0)."""
    S = np.sum(J0 * J0, axis=1)
    return np.sort(S[(S > 0) & (S <= 10 * eps)])
