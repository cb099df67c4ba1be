"""What the tests of the visual-block flags and of ctvio_cull_visual share (tests/test_cull_reference.py, tests/test_gpu_visual_active.py,
tests/test_gpu_cull_visual.py): the corrupted windows of the issue's scenario, the off set of the parity tests, and the decision rules of
include/ctvio.h (ctvio_cull_options) as a NumPy function over a gate result.

Statuses are visgate_helpers' plus INACTIVE = 5."""
import numpy as np

import visgate_helpers as vg
from test_visgate_reference import BLOCK_ARRAYS, without_blocks as _without_blocks  # noqa: F401

INACTIVE = 5
CHI2_99 = 9.21      # the 99 % point of chi-square with 2 degrees of freedom: ctvio_default_cull_options' chi2_max


def corrupted(w, seed=5, sigma=0.05):
    """(w with max(3, V // 20) of its observations shifted by N(0, sigma) in normalised image coordinates, the shifted blocks, sorted)."""
    rng = np.random.default_rng(seed)
    bad = np.sort(rng.choice(w.V, size=max(3, w.V // 20), replace=False))
    x = w.copy()
    x.v_pj[bad] += rng.normal(0, sigma, (bad.size, 2))
    return x, bad


def off_set(w, bad):
    """The off set of the parity tests: bad plus every block of landmark 0 (which leaves one landmark without any factor), sorted."""
    return np.unique(np.concatenate([np.asarray(bad), np.nonzero(np.asarray(w.v_lm) == 0)[0]]))


def flags(w, off):
    a = np.ones(w.V, np.uint8)
    a[np.asarray(off, int)] = 0
    return a


def without_blocks(w, drop):
    """w without the blocks `drop` (test_visgate_reference.without_blocks): the landmarks keep their indices, so one without blocks stays an
    unknown without a factor."""
    return _without_blocks(w, np.asarray(drop, int))


def decide(v_lm, status, chi2, lm_stats, lm_count, active, chol_fail=False, chi2_max=CHI2_99, mean_error_max=0.0, worst_only=0, drop_uncomputable=1):
    """The blocks ctvio_cull_visual switches off (bool (V,)), from what ctvio_visual_gate returns at the same state and flags.  Block rule: active,
    status 0, chi2 > chi2_max (worst_only: per landmark the largest such chi2 alone; a tie goes to the first block).  Landmark rule: the active
    status-0 blocks of a landmark with lm_count > 0 and lm_stats[:, 0] > mean_error_max.  drop_uncomputable: active blocks of status 3.  Blocks of
    status 1, 2, 4 and inactive ones are never touched; a window whose factorisation failed loses nothing."""
    v_lm = np.asarray(v_lm); status = np.asarray(status); active = np.asarray(active) != 0
    off = np.zeros(status.shape[0], bool)
    if chol_fail:
        return off
    ok = active & (status == vg.OK)
    if chi2_max > 0:
        cand = ok & (np.nan_to_num(np.asarray(chi2), nan=0.0) > chi2_max)
        if worst_only:
            for l in np.unique(v_lm[cand]):
                vs = np.nonzero(cand & (v_lm == l))[0]
                off[vs[np.argmax(np.asarray(chi2)[vs])]] = True
        else:
            off |= cand
    if mean_error_max > 0:
        hit = (np.asarray(lm_count) > 0) & (np.nan_to_num(np.asarray(lm_stats)[:, 0], nan=0.0) > mean_error_max)
        off |= ok & hit[v_lm]
    if drop_uncomputable:
        off |= active & (status == vg.NONE)
    return off


def s_zero_reference(Cw, r):
    """visgate_helpers.block_reference's formulas with S = 0 (an inactive block): (redundancy, C_loo, chi2)."""
    S = np.zeros((2, 2))
    A = S @ Cw @ S
    M = np.eye(2) - A
    T = Cw @ S
    cov = Cw + T @ np.linalg.solve(M, T.T)
    return float(vg.lambda_min(0.5 * (M + M.T))), cov, float(r @ np.linalg.solve(cov + np.eye(2), r))
