"""CPU: NumPy model of k_cov_solve's schedule (csrc/kernels_cov.hpp) on the oracle's normal matrix of real windows -- block forward substitution
over 32-row blocks with the inverses of the diagonal blocks, L read inside the tile-row envelope only (every entry left of it is NaN in the
model: a read would poison the result), the two interleaved partial sums per half block, the start at the first non-zero block -- against the
reference of tests/cov_helpers.py at its bound.  Pins the algorithm the kernel states; the kernel itself is checked on the GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def model_solve(Lf, env, B):
    """Y = L^-1 B as k_cov_solve forms it.  Lf: the factor with NaN left of the envelope; env: first tile column per 16-row tile."""
    P = Lf.shape[0]
    nblk = (P + 31) // 32
    PP = 32 * nblk
    Y = np.zeros((PP, B.shape[1]))
    Y[:P] = B
    nz = np.nonzero(B.any(axis=1))[0]
    if nz.shape[0] == 0:
        return Y[:P]
    b0 = int(nz[0]) // 32
    for b in range(b0, nblk):
        nb = min(32, P - 32 * b)
        Linv = np.eye(32)
        Linv[:nb, :nb] = np.linalg.inv(np.tril(Lf[32 * b:32 * b + nb, 32 * b:32 * b + nb]))
        T = Y[32 * b:32 * b + 32].copy()
        for h in range(2):
            R = 2 * b + h
            if 16 * R >= P:
                continue
            rows = slice(16 * R, min(16 * R + 16, P))
            kbeg = max(16 * int(env[min(R, P // 16)]), 32 * b0)
            part = [np.zeros((rows.stop - rows.start, B.shape[1])) for _ in range(2)]
            for kt in range(kbeg // 16, 2 * b):
                part[(kt - kbeg // 16) % 2] += Lf[rows, 16 * kt:16 * kt + 16] @ Y[16 * kt:16 * kt + 16]
            T[16 * h:16 * h + rows.stop - rows.start] -= part[0] + part[1]
        Y[32 * b:32 * b + 32] = Linv @ T
    return Y[:P]


@pytest.mark.parametrize("cfg,seed,kw", [("tiny", 7, {}), ("config1", 1400, dict(F=16, L=60, M=750))], ids=["tiny", "k34"])
def test_substitution_schedule_inside_the_envelope(cv, oracle, cfg, seed, kw):
    import cov_helpers as ch
    w = cv.synth.make_window(cfg, seed=seed, **kw)
    P, L = w.P, w.L
    H, _, _ = oracle.OracleWindow(w).build_normal()
    Hpp, W, Hll = H[:P, :P], H[:P, P:], np.diag(H)[P:].copy()
    active = ~ch.constant_mask(w)
    sel = ch.tiny_selection(w) if cfg == "tiny" else ch.scattered_selection(w, 40)
    ref = ch.cov_reference(Hpp, W, Hll, active, sel)
    keep = active & ~ref.untouched
    dinv = np.where(Hll > 0, 1.0 / np.where(Hll > 0, Hll, 1.0), 0.0)
    Wm = W * keep[:, None]
    S = np.where(np.outer(keep, keep), Hpp - (Wm * dinv) @ Wm.T, np.eye(P))
    Lf = np.linalg.cholesky(0.5 * (S + S.T))
    env = cv.packer.reduced_system_envelope(w)
    for r in range(P):                                   # never stored by the panel Cholesky, never to be read
        assert not Lf[r, :16 * int(env[r // 16])].any()  # (structurally zero: the envelope holds the fill)
        Lf[r, :16 * int(env[r // 16])] = np.nan
    Bsel = np.zeros((P, len(sel)))
    for c, j in enumerate(sel):
        if keep[j]:
            Bsel[j, c] = 1.0
    Ysel = np.concatenate([model_solve(Lf, env, Bsel[:, c:c + 16]) for c in range(0, len(sel), 16)], axis=1)
    cov = Ysel.T @ Ysel
    for c, j in enumerate(sel):
        if not keep[j]:
            cov[c, :] = 0.0; cov[:, c] = 0.0
            if ref.untouched[j] and active[j]:
                cov[c, c] = np.inf
    var = np.full(L, np.inf)
    obs = np.nonzero(Hll > 0)[0]
    for c in range(0, obs.shape[0], 16):
        ls = obs[c:c + 16]
        Y = model_solve(Lf, env, Wm[:, ls] * dinv[ls])
        var[ls] = dinv[ls] + np.sum(Y * Y, axis=0)
    tol = ch.bound(ref.kappa)
    e, er = ch.cov_metric(cov, ref.cov_full), ch.rel_metric(var, ref.rho_full)
    print(f"{cfg}: kappa_s {ref.kappa:.3g}, bound {tol:.3g}, model error block {e:.3g}, var_rho {er:.3g}")
    assert np.isfinite(cov[np.isfinite(ref.cov_full)]).all()
    assert np.array_equal(np.isinf(cov), np.isinf(ref.cov_full))
    assert e <= tol and er <= tol
