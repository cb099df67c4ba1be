"""NumPy fp64 reference of ctvio_covariance_batch (tests/test_cov_reference.py, tests/test_gpu_covariance.py).

Definition (include/ctvio.h): H = [[Hpp, W], [W^T, diag(Hll)]] without damping; a trajectory unknown is excluded if it is constant or if
no factor touches it (H_jj == 0 exactly); Sigma = (H restricted to the other unknowns)^-1.  A constant selected unknown gives a zero row
and column, an untouched one +inf on its diagonal and 0 elsewhere; a landmark with Hll == 0 has variance +inf.
"""
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -53


def constant_mask(w):
    """[P] True where the window holds a trajectory unknown constant (fixed_upto, knot_const, lock_bg / lock_ba, fix_ld)."""
    K, F, P = w.K, w.F, w.P
    c = np.zeros(P, bool)
    if w.fixed_upto >= 0:
        c[:6 * min(w.fixed_upto + 1, K)] = True
    if getattr(w, "knot_const", None) is not None:
        for k in np.nonzero(np.asarray(w.knot_const))[0]:
            c[6 * k:6 * k + 6] = True
    for f in range(F):
        if w.lock_bg:
            c[6 * K + 6 * f:6 * K + 6 * f + 3] = True
        if w.lock_ba:
            c[6 * K + 6 * f + 3:6 * K + 6 * f + 6] = True
    if w.fix_ld:
        c[P - 1] = True
    return c


def tiny_selection(w):
    """The four newest touched knots, the last bias state, the line delay and one index of the untouched last knot: 32 unknowns."""
    K, P = w.K, w.P
    return list(range(6 * (K - 5), 6 * (K - 1))) + list(range(P - 7, P)) + [6 * (K - 1) + 2]


def scattered_selection(w, n=32):
    return sorted(set(int(round(x)) for x in np.linspace(0, w.P - 1, n)))


def cov_metric(a, b):
    """max |a - b| / sqrt(b_ii b_jj) over the pairs whose reference entries (b) are finite with a finite, positive diagonal."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    d = np.diag(b)
    ok = np.isfinite(d) & (d > 0)
    if not ok.any():
        return 0.0
    s = np.sqrt(d[ok])
    return float(np.max(np.abs(a[np.ix_(ok, ok)] - b[np.ix_(ok, ok)]) / np.outer(s, s)))


def rel_metric(a, b):
    """max relative error over the finite reference entries."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    ok = np.isfinite(b)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0


def _expand(sig_kept, kept_idx, const, untouched, sel):
    """The selected block with the zero / +inf rules applied."""
    P = const.shape[0]
    pos = -np.ones(P, int)
    pos[kept_idx] = np.arange(kept_idx.shape[0])
    n = len(sel)
    out = np.zeros((n, n))
    for a, i in enumerate(sel):
        for b, j in enumerate(sel):
            if pos[i] >= 0 and pos[j] >= 0:
                out[a, b] = sig_kept[pos[i], pos[j]]
        if untouched[i] and not const[i]:
            out[a, a] = np.inf
    return out


def cov_reference(Hpp, W, Hll, active, sel):
    """Hpp (P, P), W (P, L), Hll (L,) as ctvio_linearize returns them; active: [P], non-zero where the unknown is NOT constant; sel: selected
    trajectory unknowns.  Returns a namespace with
      cov_full, rho_full    the selected block and the inverse-depth variances by the Jacobi-scaled inverse of the un-eliminated system,
      cov_schur, rho_schur  the same by Schur complement + numpy.linalg.cholesky + triangular solves,
      e_cpu                 their normalised difference (the larger of the block's and the variances'),
      kappa                 the scaled condition number (eigenvalues of D^-1/2 H D^-1/2 of the system that is inverted),
      const, untouched      [P] flags of the excluded unknowns."""
    Hpp = np.asarray(Hpp, float); Hll = np.asarray(Hll, float).reshape(-1)
    P, L = Hpp.shape[0], Hll.shape[0]
    W = np.asarray(W, float).reshape(P, L) if L else np.zeros((P, 0))
    const = ~(np.asarray(active).reshape(-1)[:P] != 0)
    untouched = np.diag(Hpp) == 0.0
    kp = np.nonzero(~const & ~untouched)[0]
    kl = np.nonzero(Hll > 0)[0]
    sel = [int(i) for i in sel]
    # ---- route A: the full system, Jacobi scaled
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
    cov_full = _expand(Sig[:kp.shape[0], :kp.shape[0]], kp, const, untouched, sel)
    rho_full = np.full(L, np.inf)
    rho_full[kl] = np.diag(Sig)[kp.shape[0]:]
    # ---- route B: Schur complement, Cholesky, triangular solves
    Wk = W[np.ix_(kp, kl)]
    S = Hpp[np.ix_(kp, kp)] - (Wk / Hll[kl]) @ Wk.T
    S = 0.5 * (S + S.T)
    Lc = np.linalg.cholesky(S)
    Y = np.linalg.solve(Lc, np.eye(kp.shape[0]))   # (L^-1; numpy has no triangular solve, the LU of a triangular matrix is itself)
    cov_schur = _expand(Y.T @ Y, kp, const, untouched, sel)
    rho_schur = np.full(L, np.inf)
    if kl.shape[0]:
        Z = np.linalg.solve(Lc, Wk / Hll[kl])
        rho_schur[kl] = 1.0 / Hll[kl] + np.sum(Z * Z, axis=0)
    e_cpu = max(cov_metric(cov_schur, cov_full), rel_metric(rho_schur, rho_full))
    return SimpleNamespace(cov_full=cov_full, rho_full=rho_full, cov_schur=cov_schur, rho_schur=rho_schur, e_cpu=e_cpu, kappa=kappa,
                           const=const, untouched=untouched)


def bound(kappa):
    """First-order bound of a Cholesky-based inverse in fp64: 4 kappa_s 2^-53."""
    return 4.0 * kappa * EPS
