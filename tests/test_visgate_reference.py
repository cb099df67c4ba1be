"""CPU: the NumPy reference of the leave-one-out visual gate (tests/visgate_helpers.py) on the oracle's normal matrix.  The corrector S against
what the oracle's linearisation holds for a block (H with the block minus H without it); the Woodbury form of C_loo against the brute-force
route -- H minus the block's own corrected J~^T J~, inverted --; the quantities of the formulation's table; statuses, constants, fix_ld,
per-block v_cauchy and a <= 0."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

EPS = 2.0 ** -53
# smallest / largest redundancy, blocks whose naive I - img_w^2 C is indefinite, smallest eigenvalue of C_loo.  The redundancies are those of
# S = sqrt(rho') I, which Corrector's rule gives for the Cauchy loss (test_corrector_is_what_the_linearisation_applies); with the unguarded
# alpha they would read [0.224, 0.998] and [0.056, 0.994].
TABLE = {"tiny": (0.0679, 0.9583, 32, 0.479), "config1": (0.0504, 0.9929, 5, 0.0027)}
BLOCK_ARRAYS = ("v_lm", "v_ti", "v_tj", "v_rowi", "v_rowj", "v_pi", "v_pj")


def oracle_reference(oracle, w):
    from test_projection_reference import oracle_reference as o
    return o(oracle, w)


def fixture_window(cv, golden_dir, cfg, seed):
    fx = np.load(os.path.join(golden_dir, f"cov_{cfg}_seed{seed}.npz"))
    w = cv.synth.make_window(cfg, seed=seed)
    w.quat[:] = fx["quat"]; w.pos[:] = fx["pos"]; w.bias[:] = fx["bias"]; w.rho[:] = fx["rho"]; w.ld = float(fx["ld"])
    return w


def without_blocks(w, drop):
    x = w.copy()
    keep = np.ones(w.V, bool)
    keep[np.asarray(drop)] = False
    for a in BLOCK_ARRAYS:
        setattr(x, a, getattr(x, a)[keep])
    if x.v_cauchy is not None:
        x.v_cauchy = x.v_cauchy[keep]
    return x


@pytest.fixture(scope="module")
def refs(cv, oracle, golden_dir):
    """name -> (window at the covariance fixture's state, the joint reference on the oracle's H, the per-block references); computed once."""
    import visgate_helpers as vg
    out = {}
    for name, cfg, seed in (("tiny", "tiny", 7), ("config1", "config1", 1000)):
        w = fixture_window(cv, golden_dir, cfg, seed)
        ref = oracle_reference(oracle, w)
        out[name] = (w, ref, [vg.block_reference(w, ref, v) for v in range(w.V)])
    return out


def brute_force_check(w, ref, R, what):
    import cov_helpers as ch
    import visgate_helpers as vg
    worst = 0.0
    for b in R:
        assert b.status == vg.OK, (what, b.v, b.status)
        C, tol, kappa = vg.brute_force(w, ref, b)
        tol = tol + vg.loo_bound(b)      # (both routes carry the error of their own inverse)
        e = ch.cov_metric(b.cov, C)
        assert np.isfinite(kappa) and tol < 1e-2, (what, b.v, kappa, tol)
        assert e <= tol, (what, b.v, e, tol, b.redundancy)
        worst = max(worst, e / tol)
    print(f"{what}: {len(R)} blocks, Woodbury against the downdated inverse: worst {worst:.3g} of the bound")


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_formulation_table(refs, name):
    """What the formulation was checked on (TABLE): I - A positive definite for every block, the redundancies well above the default
    min_redundancy; the naive unit-weight I - img_w^2 C is indefinite for all 32 blocks of `tiny` and some of `config1`; C_loo positive
    definite."""
    import visgate_helpers as vg
    w, ref, R = refs[name]
    assert w.V == (32 if name == "tiny" else 201)
    red = np.array([b.redundancy for b in R])
    naive = np.array([vg.lambda_min(np.eye(2) - b.Cw) for b in R])
    loo = np.array([np.linalg.eigvalsh(b.cov)[0] for b in R])
    s = np.array([b.res @ b.res for b in R])
    print(f"{name}: median |r|^2 {np.median(s):.3g}, redundancy in [{red.min():.3g}, {red.max():.3g}], naive negative for {(naive < 0).sum()} of "
          f"{w.V}, smallest eigenvalue of C_loo {loo.min():.3g}")
    assert all(b.status == vg.OK for b in R)
    lo, hi = TABLE[name][:2]
    assert abs(red.min() - lo) < 1e-3 and abs(red.max() - hi) < 1e-3, (red.min(), red.max())
    assert (naive < 0).sum() == TABLE[name][2]
    assert loo.min() > 0 and abs(loo.min() / TABLE[name][3] - 1) < 0.02, loo.min()


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_woodbury_against_the_downdated_system(refs, name):
    """Every block of `tiny`, every eighth of `config1`: C_loo = J (H - J~^T J~)^-1 J^T within the sum of the two routes' bounds."""
    w, ref, R = refs[name]
    brute_force_check(w, ref, R if name == "tiny" else R[::8], name)


def test_corrector_is_what_the_linearisation_applies(cv, oracle, refs):
    """H(window) - H(window without block v) = J~^T J~ with J~ = S img_w [Jp | j]: the oracle's robustified rows of that block.  The
    difference of two sums of squares rounds at 2^-53 of the larger diagonal entry per term (64 terms at most per entry); the helper's
    Jacobian agrees with the oracle's to 1e-9 of its largest entry (tests/test_projection_reference.py: 1e-8 against central differences).
    With the uncorrected alpha = 1 - sqrt(1 + 2 s rho'' / rho') -- Corrector's rule for rho'' <= 0 ignored -- the identity fails by
    orders of magnitude on `tiny`, whose residuals are large: the rule is part of what the linearisation applies."""
    import visgate_helpers as vg
    w, ref, R = refs["tiny"]
    assert not w.fix_ld and w.fixed_upto < 0
    H = oracle.OracleWindow(w.copy()).build_normal()[0]
    P = w.P
    worst, worst_alt = 0.0, np.inf
    for v in range(0, w.V, 3):
        b = R[v]
        Hm = oracle.OracleWindow(without_blocks(w, [v])).build_normal()[0]
        dH = H - Hm
        J = w.img_w * b.pj.J
        Jt = b.S @ J
        want = Jt.T @ Jt
        tol = 64 * EPS * float(np.max(np.diag(H))) + 1e-9 * float(np.abs(want).max())
        e = float(np.abs(dH - want).max())
        worst = max(worst, e / tol)
        assert e <= tol, (v, e, tol)
        s = float(b.res @ b.res)
        a = vg.cauchy_width(w, v)
        rho1 = 1.0 / (1.0 + s / a ** 2); rho2 = -(1.0 / a ** 2) * rho1 ** 2
        alpha = 1.0 - np.sqrt(max(0.0, 1.0 + 2.0 * s * rho2 / rho1))
        Ja = np.sqrt(rho1) * (np.eye(2) - alpha * np.outer(b.res, b.res) / s) @ J
        worst_alt = min(worst_alt, float(np.abs(dH - Ja.T @ Ja).max()) / tol)
        assert b.weight == rho1 and np.array_equal(b.S, np.sqrt(rho1) * np.eye(2))
    print(f"corrector: worst {worst:.3g} of the bound; without Corrector's rule at least {worst_alt:.3g} of it")
    assert worst_alt > 1e3


def test_cauchy_widths(cv, oracle, refs):
    """Per-block v_cauchy mixing 1, 2, 0 and -1: weight and S in closed form, no loss gives (1, I); the brute-force identity holds on the
    oracle's H of that window."""
    import visgate_helpers as vg
    w0 = refs["config1"][0]      # (converged: without a loss an unconverged block of `tiny` carries nearly all of its landmark's information)
    w = w0.copy()
    w.v_cauchy = np.array([(1.0, 2.0, 0.0, -1.0)[v % 4] for v in range(w.V)])
    ref = oracle_reference(oracle, w)
    R = [vg.block_reference(w, ref, v) for v in range(w.V)]
    for v, b in enumerate(R):
        s = float(b.res @ b.res)
        a = w.v_cauchy[v]
        assert b.weight == (1.0 / (1.0 + s / a ** 2) if a > 0 else 1.0), v
        assert np.array_equal(b.S, np.sqrt(b.weight) * np.eye(2)), v
    assert np.array_equal(vg.corrector(np.zeros(2), 2.0)[1], np.eye(2)) and vg.corrector(np.array([3.0, 4.0]), 0.0) == (1.0, pytest.approx(np.eye(2)))
    assert all(b.status == vg.OK for b in R)
    brute_force_check(w, ref, R[::5], "config1, v_cauchy 1 / 2 / <= 0")


def test_constants_and_fix_ld(cv, oracle, refs):
    """fix_ld and fixed_upto = 3: constant unknowns contribute nothing -- they are not in the kept system, and the brute-force identity
    holds there; with fix_ld a block on a row > 0 differs from the free window's far beyond the bound."""
    import cov_helpers as ch
    import visgate_helpers as vg
    w0, _, R0 = refs["tiny"]
    for what, kw in (("fix_ld", dict(fix_ld=True)), ("fixed_upto = 3", dict(fixed_upto=3))):
        w = w0.copy()
        for k, val in kw.items():
            setattr(w, k, val)
        ref = oracle_reference(oracle, w)
        R = [vg.block_reference(w, ref, v) for v in range(w.V)]
        for a, b in zip(R, R0):
            assert np.array_equal(a.res, b.res) and a.weight == b.weight and a.depth == b.depth
        ok = [b for b in R if b.status == vg.OK]
        assert len(ok) >= w.V - 4
        brute_force_check(w, ref, ok, "tiny, " + what)
        assert all(a.redundancy >= b.redundancy - 1e-12 for a, b in zip(R, R0) if a.status == vg.OK)     # (fewer unknowns: the rest predicts better)
        if what == "fix_ld" and w0.ld != 0.0:
            assert max(ch.cov_metric(a.cov, b.cov) for a, b in zip(R, R0) if a.status == vg.OK and w.v_rowj[a.v] > 0) > 1e-6


def test_statuses(cv, oracle, refs):
    """3: rho <= 0, two anchors (everything NaN).  4: the only block of a landmark with a free depth -- the redundancy is zero up to rounding,
    far below min_redundancy / 10.  2: Hll == 0 (rho = 1e154: the depth column underflows in the normal matrix).  The landmark statistics
    follow the statuses."""
    import visgate_helpers as vg
    w0 = refs["tiny"][0]
    w = w0.copy(); w.rho[2] = -1.0
    R = [vg.block_reference(w, oracle_reference(oracle, w), v) for v in range(w.V)]
    assert all((b.status == vg.NONE) == (b.l == 2) for b in R)
    assert all(np.isnan(b.res).all() and np.isnan(b.weight) and np.isnan(b.cov).all() and np.isnan(b.chi2) for b in R if b.l == 2)
    stats, cnt = vg.landmark_reference(w, R)
    assert cnt[2] == 0 and np.isnan(stats[2, 0]) and stats[2, 1] == 0.0 and np.isposinf(stats[2, 2])
    assert all(cnt[l] == (w.v_lm == l).sum() and stats[l, 0] > 0 and stats[l, 1] > 0 and 0 < stats[l, 2] < 1 for l in range(w.L) if l != 2)
    w = w0.copy()
    vs = np.nonzero(w.v_lm == 6)[0]
    w.v_pi[vs[-1], 0] += 1e-3
    R = [vg.block_reference(w, None, v) for v in range(w.V)]
    assert all((b.status == vg.NONE) == (b.l == 6) for b in R)
    vs = np.nonzero(w0.v_lm == 4)[0]
    w = without_blocks(w0, vs[1:])
    R = [vg.block_reference(w, oracle_reference(oracle, w), v) for v in range(w.V)]
    b = R[int(np.nonzero(w.v_lm == 4)[0][0])]
    assert b.status == vg.WEAK and abs(b.redundancy) < 1e-3 and np.isposinf(np.diag(b.cov)).all() and b.chi2 == 0.0, b.redundancy
    assert sum(x.status == vg.WEAK for x in R) == 1
    stats, cnt = vg.landmark_reference(w, R)
    assert cnt[4] == 1 and stats[4, 1] == 0.0 and stats[4, 2] == b.redundancy
    w1 = refs["config1"][0]      # (`tiny` has no camera that looks at another camera's centre)
    for l in range(w1.L):
        w = w1.copy(); w.rho[l] = 1e154
        if any(x.status == vg.OK for x in (vg.block_reference(w, None, v) for v in np.nonzero(w.v_lm == l)[0])):
            break
    else:
        pytest.fail("no landmark whose anchor camera lies in front of an observing one")
    ref = oracle_reference(oracle, w)
    assert ref.Hll[l] == 0.0
    R = [vg.block_reference(w, ref, v) for v in range(w.V)]
    mine = [b for b in R if b.l == l]
    assert any(b.status == vg.NO_INFO for b in mine) and all(b.status in (vg.NO_INFO, vg.NONE) for b in mine)
    assert all(b.redundancy == 0.0 and b.chi2 == 0.0 and np.isposinf(np.diag(b.cov)).all() and np.isfinite(b.res).all() for b in mine if b.status == vg.NO_INFO)
