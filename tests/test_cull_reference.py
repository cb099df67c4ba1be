"""CPU: the scenario ctvio_cull_visual was designed on, with the oracle and the NumPy gate reference (tests/visgate_helpers.py) alone.  A
window with a few shifted observations is solved, every block is gated on the oracle's H, and the 99 % point separates the shifted blocks
from the clean ones (the two tables of the design, pinned); the decision rules of cull_helpers.decide on that gate; the oracle accepts the
reduced window -- the landmark left without a factor has a zero row and column and does not move --; and block_reference's formulas with
S = 0 give redundancy 1 and C_loo = Cw: the gate of an inactive block is the re-admission test."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# name -> (config, seed, shifted blocks, smallest chi2 of the shifted blocks >=, largest chi2 of the clean status-0 blocks <=, clean blocks of status 4)
TABLE = {"tiny": ("tiny", 7, 3, 182.0, 3.33, None), "config1": ("config1", 1000, 10, 511.0, 5.42, 1)}


@pytest.fixture(scope="module")
def gated(cv, oracle):
    """name -> (the corrupted window after the oracle's 15 iterations, the shifted blocks, the per-block references, (lm_stats, lm_count))."""
    import cull_helpers as cu
    import visgate_helpers as vg
    from test_projection_reference import oracle_reference
    out = {}
    for name, (cfg, seed, *_) in TABLE.items():
        w, bad = cu.corrupted(cv.synth.make_window(cfg, seed=seed))
        oracle.OracleWindow(w).solve(15)
        ref = oracle_reference(oracle, w)
        R = [vg.block_reference(w, ref, v) for v in range(w.V)]
        out[name] = (w, bad, R, vg.landmark_reference(w, R))
    return out


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_separation_table(gated, name):
    import cull_helpers as cu
    import visgate_helpers as vg
    w, bad, R, (lms, cnt) = gated[name]
    _, _, nbad, lo_bad, hi_clean, nweak = TABLE[name]
    assert bad.shape[0] == nbad
    st = np.array([b.status for b in R]); chi = np.array([b.chi2 for b in R])
    clean = np.setdiff1d(np.arange(w.V), bad)
    print(f"{name}: shifted chi2 >= {chi[bad].min():.4g}, clean status-0 chi2 <= {chi[clean][st[clean] == vg.OK].max():.4g}, "
          f"clean statuses {np.bincount(st[clean]).tolist()}")
    assert (st[bad] == vg.OK).all() and chi[bad].min() >= lo_bad
    assert np.isin(st[clean], (vg.OK, vg.WEAK)).all() and chi[clean][st[clean] == vg.OK].max() <= hi_clean
    if nweak is not None:
        assert (st[clean] == vg.WEAK).sum() == nweak
    off = cu.decide(w.v_lm, st, chi, lms, cnt, np.ones(w.V, np.uint8))
    assert np.array_equal(np.nonzero(off)[0], bad)                 # the 99 % point separates them without error
    assert not off[st == vg.WEAK].any()


def test_rules(gated):
    """worst_only takes one block per landmark (the arg-max); the landmark rule takes whole landmarks; inactive blocks, blocks of status 1, 2, 4
    are never touched; status 3 goes with drop_uncomputable alone; a failed factorisation loses nothing; chi2_max <= 0 switches the block rule off."""
    import cull_helpers as cu
    import visgate_helpers as vg
    w, bad, R, (lms, cnt) = gated["config1"]
    st = np.array([b.status for b in R]); chi = np.array([b.chi2 for b in R])
    on = np.ones(w.V, np.uint8)
    one = cu.decide(w.v_lm, st, chi, lms, cnt, on, worst_only=1)
    for l in np.unique(w.v_lm[bad]):
        vs = bad[w.v_lm[bad] == l]
        assert one[vs].sum() == 1 and one[vs[np.argmax(chi[vs])]]
    assert one.sum() == np.unique(w.v_lm[bad]).shape[0]
    by_lm = cu.decide(w.v_lm, st, chi, lms, cnt, on, chi2_max=0.0, mean_error_max=0.01)
    hit = np.nonzero(lms[:, 0] > 0.01)[0]
    assert hit.shape[0] > 0 and np.array_equal(by_lm, np.isin(w.v_lm, hit) & (st == vg.OK))
    assert not cu.decide(w.v_lm, st, chi, lms, cnt, on, chi2_max=0.0).any()
    assert not cu.decide(w.v_lm, st, chi, lms, cnt, on, chol_fail=True).any()
    some = on.copy(); some[bad[:2]] = 0
    assert np.array_equal(np.nonzero(cu.decide(w.v_lm, st, chi, lms, cnt, some))[0], bad[2:])
    st2 = st.copy(); st2[bad[0]] = vg.NONE; st2[bad[1]] = vg.SINGULAR; st2[bad[2]] = vg.NO_INFO; st2[bad[3]] = vg.WEAK
    assert np.array_equal(np.nonzero(cu.decide(w.v_lm, st2, chi, lms, cnt, on))[0], np.r_[bad[0], bad[4:]])
    assert np.array_equal(np.nonzero(cu.decide(w.v_lm, st2, chi, lms, cnt, on, drop_uncomputable=0))[0], bad[4:])


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_oracle_accepts_the_reduced_window(oracle, gated, name):
    """The window without the off set of the parity tests (the shifted blocks and every block of landmark 0): finite normal equations with a
    zero row and column for landmark 0, whose inverse depth a solve does not move."""
    import cull_helpers as cu
    w, bad, _, _ = gated[name]
    x = cu.without_blocks(w, cu.off_set(w, bad))
    assert x.L == w.L and x.V == w.V - cu.off_set(w, bad).shape[0]
    H, g, cost = oracle.OracleWindow(x.copy()).build_normal()
    P = x.P
    assert np.isfinite(H).all() and np.isfinite(g).all() and np.isfinite(cost)
    assert (H[P, :] == 0).all() and (H[:, P] == 0).all() and g[P] == 0
    y = x.copy()
    sm = oracle.OracleWindow(y).solve(4)
    assert np.isfinite(sm.final_cost) and y.rho[0] == x.rho[0]


def test_s_zero_is_the_readmission_gate(gated):
    """block_reference's formulas with S = 0: A = 0, redundancy exactly 1, C_loo = Cw to the bit, chi2 = r^T (Cw + I)^-1 r."""
    import cull_helpers as cu
    w, bad, R, _ = gated["tiny"]
    for b in R:
        red, cov, chi = cu.s_zero_reference(b.Cw, b.res)
        assert red == 1.0 and np.array_equal(cov, b.Cw)
        assert chi == pytest.approx(float(b.res @ np.linalg.solve(b.Cw + np.eye(2), b.res)), rel=1e-14)
