"""CPU: the NumPy restatement of the triangulation (tests/tri_helpers.py) recovers the true depths at the true state, and the model of the
kernel's one-sided Jacobi agrees with the SVD."""
import numpy as np
import pytest

import tri_helpers as th

CASES = [("tiny", 7), ("tumrs", 1000)]


@pytest.fixture(scope="module")
def truth_windows(cv):
    return {c: cv.synth.make_window(c[0], seed=c[1], return_truth=True, pix_sigma=0.0)[1] for c in CASES}


@pytest.mark.parametrize("case", CASES)
def test_row_time_triangulation_recovers_the_true_depths(truth_windows, case):
    """At the true state with noise-free pixels every landmark's row-time depth is 1 / rho_true within 1e-2 relative (the residue is the
    row rounding of the synthetic projection: 1.2e-3 on tiny/7, 3.1e-3 on tumrs/1000); frame-time triangulation is far off."""
    w = truth_windows[case]
    depth, flag, _ = th.triangulate_ref(w, row_times=1)
    assert flag.shape == (w.L,) and np.all(flag == th.OK)      # no landmark left out
    err = th.rel_err(depth, 1.0 / w.rho)
    print(case, "row-time max rel err", err.max())
    assert err.max() < 1e-2
    d0, f0, _ = th.triangulate_ref(w, row_times=0)
    assert th.rel_err(d0, 1.0 / w.rho).max() > 10 * err.max()


@pytest.mark.parametrize("case", CASES)
def test_hestenes_model_matches_the_svd(truth_windows, case):
    """The kernel's iteration (pair order, rotation, stop rule) against np.linalg.svd: 1e-10 relative on every landmark, both time modes."""
    w = truth_windows[case]
    worst, worst_sweeps, cond = 0.0, 0, 1.0
    for row_times in (1, 0):
        for l in range(w.L):
            A = th.build_A(w, l, row_times)
            assert A is not None
            d, sweeps = th.hestenes_depth(A)
            worst = max(worst, float(th.rel_err(d, th.svd_depth(A))))
            worst_sweeps = max(worst_sweeps, sweeps)
            sv = th.singular_values(A)
            cond = min(cond, sv[2] / sv[0])
    print(case, "hestenes vs svd max rel err", worst, "sweeps", worst_sweeps, "min sigma3/sigma1", cond)
    assert worst < 1e-10
    assert worst_sweeps < th.MAX_SWEEPS      # the stop rule ends the iteration, not the cap
