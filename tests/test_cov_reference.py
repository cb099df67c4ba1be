"""CPU: the NumPy reference of the covariance (tests/cov_helpers.py: the Jacobi-scaled full inverse and the Schur + Cholesky route) against
the 50-digit fixtures of tests/golden/make_cov_golden.py, computed on the oracle's normal matrix.  Bound: 4 kappa_s 2^-53, the first-order
bound of a Cholesky-based inverse, with kappa_s the scaled condition number the helper returns."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

CASES = [("cov_tiny_seed7", "tiny", 7), ("cov_config1_seed1000", "config1", 1000)]


@pytest.fixture(scope="module")
def references(cv, oracle, golden_dir):
    """name -> (fixture, window at the fixture's state, the helper's result on the oracle's H); each computed once."""
    import cov_helpers as ch
    out = {}
    for name, cfg, seed in CASES:
        fx = np.load(os.path.join(golden_dir, name + ".npz"))
        w = cv.synth.make_window(cfg, seed=seed)
        w.quat[:] = fx["quat"]; w.pos[:] = fx["pos"]; w.bias[:] = fx["bias"]; w.rho[:] = fx["rho"]; w.ld = float(fx["ld"])
        H, _, _ = oracle.OracleWindow(w).build_normal()
        P = w.P
        ref = ch.cov_reference(H[:P, :P], H[:P, P:], np.diag(H)[P:], ~ch.constant_mask(w), fx["sel"])
        out[name] = (fx, w, ref)
    return out


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_both_routes_against_50_digits(references, name):
    import cov_helpers as ch
    fx, w, ref = references[name]
    tol = ch.bound(ref.kappa)
    errs = {}
    for route, cov, rho in (("full", ref.cov_full, ref.rho_full), ("schur", ref.cov_schur, ref.rho_schur)):
        errs[route] = (ch.cov_metric(cov, fx["block"]), ch.rel_metric(rho, fx["var_rho"]))
    print(f"{name}: kappa_s {ref.kappa:.3g}, bound {tol:.3g}, errors (block, var_rho) {errs}, route difference {ref.e_cpu:.3g}")
    assert np.isfinite(ref.kappa) and tol < 1e-3, ref.kappa       # (a bound that says nothing would be no check)
    for route, (eb, er) in errs.items():
        assert eb <= tol, (route, eb, tol)
        assert er <= tol, (route, er, tol)
    assert ref.e_cpu <= 2 * tol
    for cov in (ref.cov_full, ref.cov_schur):    # the zero / +inf rules, entry for entry
        assert np.array_equal(np.isinf(cov), np.isinf(fx["block"]))
        assert np.array_equal(cov == 0, fx["block"] == 0)
    assert np.array_equal(np.isinf(ref.rho_full), np.isinf(fx["var_rho"]))


def test_fixture_diagonal_agrees_with_its_block(references):
    """sigma_diag covers every trajectory unknown: on the selected ones it is the block's diagonal; tiny's last knot is untouched."""
    for name, (fx, w, ref) in references.items():
        assert np.array_equal(fx["sigma_diag"][fx["sel"]], np.diag(fx["block"]))
    fx, w, _ = references["cov_tiny_seed7"]
    assert np.all(np.isinf(fx["sigma_diag"][6 * (w.K - 1):6 * w.K]))
    assert np.isfinite(fx["sigma_diag"][:6 * (w.K - 1)]).all()
