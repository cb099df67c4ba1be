"""CPU: the NumPy model of the blocked device marginalisation (csrc/marg_blocked.hpp; tests/marg_blocked_helpers.py) -- 32-column blocks
padded to a multiple of 64, round-robin block pairs, one inner parallel Jacobi sweep per 64 x 64 sub-problem, explicit Q, the oracle's
convergence rule -- on the config-5 drop set (m 268 / n 553, diag(A) spanning 0 .. 1e14) against the oracle's cyclic Jacobi, with the GPU
test's criteria.  A Householder-class solver misses the scaled criterion by four orders (host leg: 1.5e-4, rank 549)."""
import numpy as np
import pytest

import marg_blocked_helpers as mb


def test_padding_is_exact():
    """Padded columns meet only zeros: they stay exact zero eigenpairs, and the real eigenpairs are those of the matrix."""
    rng = np.random.default_rng(4)
    X = rng.standard_normal((70, 40)) * np.logspace(0, 6, 40)
    A = X @ X.T                                        # 70 x 70, rank 40: padded to 128, four blocks
    e, V, sweeps = mb.block_jacobi(A)
    assert sweeps > 0
    np.testing.assert_allclose(V @ np.diag(e) @ V.T, A, rtol=0, atol=1e-12 * np.abs(A).max())
    np.testing.assert_allclose(V.T @ V, np.eye(70), rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.sort(e), np.linalg.eigvalsh(A), rtol=0, atol=1e-11 * np.abs(A).max())


def test_block_jacobi_matches_oracle_on_config5_drop_set(oracle):
    w = mb.config5_window(1500)
    role = mb.drop_roles(w, [0, 1])
    assert (role == 1).sum() == 268 and (role == 0).sum() == 553
    H, g, _ = oracle.OracleWindow(w.copy()).build_normal()
    ko, Jo, ro = oracle.OracleWindow(w.copy()).marginalize(role, 1e-8)
    kept, J0, r0 = mb.blocked_marginalize(H, g, role, 1e-8)
    assert np.array_equal(kept, ko)
    eH, eg, eS = mb.prior_errors(J0, r0, Jo, ro)
    print(f"model vs oracle: J0'J0 {eH:.2e}, J0'r0 {eg:.2e}, scaled {eS:.2e}, rank {mb.rank(J0)} / {mb.rank(Jo)}")
    assert eH <= 1e-7 and eg <= 1e-7
    assert eS <= 1e-8                                  # measured 8.9e-11
    assert mb.rank(J0) == mb.rank(Jo) == 547
