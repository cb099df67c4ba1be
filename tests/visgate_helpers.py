"""NumPy fp64 reference of ctvio_visual_gate_batch (tests/test_visgate_reference.py, tests/test_gpu_visual_gate.py).

Definition (include/ctvio.h): block b = (l, t_j, row_j, p_j) of the window itself.  (proj.xy, depth) = projection_helpers.project for the
query (l, t_j, row_j); r = img_w (proj.xy - p_j), s = |r|^2, weight = rho'(s) = 1 / (1 + s / a^2) with a the block's Cauchy width (v_cauchy,
else cauchy_a; <= 0: no loss, weight 1).  Corrector S = sqrt(rho') (I - alpha r r^T / s) with Ceres' rule alpha = 0 where s == 0 or
rho'' <= 0 (the Cauchy loss: always), else alpha = 1 - sqrt(max(0, 1 + 2 s rho'' / rho')).  Cw = img_w^2 C with C
projection_helpers.proj_cov_reference on a lmpoint_helpers.joint_reference; A = S Cw S, redundancy = lambda_min(I - A),
C_loo = Cw + Cw S (I - A)^-1 S Cw, chi2 = r^T (C_loo + I)^-1 r.  Statuses: 3 not computable, 2 no information, 4 redundancy < min_redundancy
(1, a failed factorisation, has no reference).  brute_force() is the independent route: H minus the block's own J~^T J~, inverted.
"""
from types import SimpleNamespace

import numpy as np

import cov_helpers as ch
import posecov_helpers as ph
import projection_helpers as pr

OK, SINGULAR, NO_INFO, NONE, WEAK = 0, 1, 2, 3, 4
EPS = 2.0 ** -53
INF2 = np.diag(np.full(2, np.inf))


def cauchy_width(w, v):
    vc = getattr(w, "v_cauchy", None)
    return float(vc[v]) if vc is not None else float(w.cauchy_a)


def corrector(r, a):
    """(weight rho'(s), S (2, 2)) of the whitened residual r under CauchyLoss(a); a <= 0: (1, I)."""
    r = np.asarray(r, float)
    s = float(r @ r)
    if not a > 0:
        return 1.0, np.eye(2)
    rho1 = 1.0 / (1.0 + s / (a * a))
    rho2 = -(1.0 / (a * a)) * rho1 * rho1
    if s == 0.0 or rho2 <= 0.0:
        return rho1, np.sqrt(rho1) * np.eye(2)
    alpha = 1.0 - np.sqrt(max(0.0, 1.0 + 2.0 * s * rho2 / rho1))
    return rho1, np.sqrt(rho1) * (np.eye(2) - alpha * np.outer(r, r) / s)


def lambda_min(M):
    """The smaller eigenvalue of a symmetric 2 x 2 in closed form."""
    return 0.5 * (M[0, 0] + M[1, 1]) - np.sqrt((0.5 * (M[0, 0] - M[1, 1])) ** 2 + M[0, 1] ** 2)


def chi2_reference(r, cov):
    """(r^T (cov + I)^-1 r, kappa_2 of the 2 x 2) from the given bits, in extended precision."""
    return pr.chi2_reference(np.zeros(2), cov, r, 1.0)


def block_reference(w, ref, v, min_redundancy=0.01):
    """The reference of block v on a lmpoint_helpers.joint_reference: a namespace (status, res (2,), weight, depth, S, pj, Cw, A, redundancy,
    cov, chi2, tol, g: projection_helpers.bound of the block's query, K = C_loo Cw^-1).  NaN where the status says so."""
    l, t, row = int(w.v_lm[v]), int(w.v_tj[v]), int(w.v_rowj[v])
    nan = np.nan
    out = SimpleNamespace(v=v, l=l, status=NONE, res=np.full(2, nan), weight=nan, depth=nan, S=None, pj=None, Cw=None, A=None, redundancy=nan,
                          cov=np.full((2, 2), nan), chi2=nan, tol=0.0, g=0.0, K=None)
    proj, _, sv = pr.project(w, l, t, row)
    if sv != pr.OK:
        return out
    out.res = w.img_w * (proj[:2] - np.asarray(w.v_pj[v], float))
    out.depth = float(proj[2])
    out.weight, out.S = corrector(out.res, cauchy_width(w, v))
    if ref is None:
        out.status = OK
        return out
    out.pj = pr.projection_jacobian(w, l, t, row)
    C, sc = pr.proj_cov_reference(ref, out.pj, l)
    if sc == pr.NO_INFO:
        out.status, out.redundancy, out.cov, out.chi2 = NO_INFO, 0.0, INF2.copy(), 0.0
        return out
    out.tol, out.g = pr.bound(ref, out.pj, l)
    S = out.S
    out.Cw = w.img_w ** 2 * C
    out.A = S @ out.Cw @ S
    M = np.eye(2) - out.A
    out.redundancy = float(lambda_min(0.5 * (M + M.T)))
    if out.redundancy < min_redundancy:
        out.status, out.cov, out.chi2 = WEAK, INF2.copy(), 0.0
        return out
    T = out.Cw @ S
    cov = out.Cw + T @ np.linalg.solve(M, T.T)
    out.cov = 0.5 * (cov + cov.T)
    out.K = np.eye(2) + T @ np.linalg.solve(M, S)      # C_loo = K Cw
    out.chi2 = float(out.res @ np.linalg.solve(out.cov + np.eye(2), out.res))
    out.status = OK
    return out


def loo_amplification(b):
    """First-order: C_loo = (Cw^-1 - S^2)^-1, so dC_loo = K dCw K^T with K = C_loo Cw^-1 = (I - Cw S^2)^-1, whose norm is 1 / redundancy.  An
    error of tol sqrt(Cw_cc Cw_dd) per entry of Cw becomes at most tol t_a t_b in C_loo with t = |K| sqrt(diag Cw); relative to
    sqrt(C_loo_aa C_loo_bb) that is at most tol max_a t_a^2 / C_loo_aa -- 1 / redundancy for an isotropic block (posecov_helpers.amplification's
    argument, one step further)."""
    t = np.abs(b.K) @ np.sqrt(np.diag(b.Cw))
    return float(np.max(t ** 2 / np.diag(b.cov)))


def loo_bound(b):
    """The bound of cov4 in cov_helpers.cov_metric: the projection bound through loo_amplification, plus the 2 x 2 step's own rounding -- a
    2 x 2 solve against I - A (condition <= 1 / redundancy) and a handful of products: 64 * 2^-53 / redundancy, relative to the largest entry
    of C_loo, so times lambda_max / the smallest diagonal entry."""
    ev = np.linalg.eigvalsh(b.cov)
    return b.tol * loo_amplification(b) + 64 * EPS / b.redundancy * float(ev[-1] / np.min(np.diag(b.cov)))


def redundancy_bound(b):
    """|d redundancy| <= |dA|_2 <= |S|_2^2 |dCw|_2 <= |S|_2^2 2 tol max diag(Cw) (an entrywise error tol sqrt(Cw_aa Cw_bb) of a 2 x 2), plus
    the closed form's own rounding 16 * 2^-53 (the entries of I - A are at most 1).  Relative to the redundancy this is the amplification
    1 / redundancy."""
    return 2.0 * b.tol * float(np.linalg.norm(b.S, 2) ** 2 * np.max(np.diag(b.Cw))) + 16 * EPS


def kept_system(ref):
    """H over the unknowns of ref.Sig, as lmpoint_helpers.joint_reference assembles it."""
    kp, kl = ref.kp, ref.kl
    n = kp.shape[0] + kl.shape[0]
    H = np.zeros((n, n))
    H[:kp.shape[0], :kp.shape[0]] = ref.Hpp[np.ix_(kp, kp)]
    H[:kp.shape[0], kp.shape[0]:] = ref.W[np.ix_(kp, kl)]
    H[kp.shape[0]:, :kp.shape[0]] = ref.W[np.ix_(kp, kl)].T
    H[kp.shape[0]:, kp.shape[0]:] = np.diag(ref.Hll[kl])
    return H


def corrected_jacobian(w, ref, b):
    """(J, J~): img_w [Jp | j] over the kept unknowns, and S times it -- the block's rows as the linearisation holds them."""
    J = w.img_w * pr.kept_jacobian(ref, b.pj, b.l)
    return J, b.S @ J


def brute_force(w, ref, b):
    """(J (H - J~^T J~)^-1 J^T, its bound in cov_helpers.cov_metric): the downdated system inverted after Jacobi scaling, as joint_reference
    inverts the full one; the bound is cov_helpers.bound(kappa of the downdated, scaled system) times posecov_helpers.amplification of J over
    that inverse."""
    J, Jt = corrected_jacobian(w, ref, b)
    Hd = kept_system(ref) - Jt.T @ Jt
    d = 1.0 / np.sqrt(np.diag(Hd))
    Hs = Hd * np.outer(d, d)
    Hs = 0.5 * (Hs + Hs.T)
    ev = np.linalg.eigvalsh(Hs)
    kappa = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
    Sig = np.linalg.inv(Hs) * np.outer(d, d)
    C = J @ Sig @ J.T
    return 0.5 * (C + C.T), ch.bound(kappa) * ph.amplification(J, Sig), kappa


def landmark_reference(w, blocks):
    """(lm_stats (L, 3), lm_count (L,)) from per-block references: count and mean |proj - p_j| over the blocks whose status is not 3, the
    largest chi2 over status 0 (0: none), the smallest redundancy over status 0 or 4 (+inf: none)."""
    stats = np.zeros((w.L, 3)); cnt = np.zeros(w.L, np.int32)
    stats[:, 0] = np.nan; stats[:, 2] = np.inf
    for l in range(w.L):
        bs = [b for b in blocks if b.l == l and b.status != NONE]
        cnt[l] = len(bs)
        if bs:
            stats[l, 0] = np.mean([np.sqrt(b.res @ b.res) / w.img_w for b in bs])
        chis = [b.chi2 for b in bs if b.status == OK]
        reds = [b.redundancy for b in bs if b.status in (OK, WEAK)]
        stats[l, 1] = max(chis) if chis else 0.0
        stats[l, 2] = min(reds) if reds else np.inf
    return stats, cnt
