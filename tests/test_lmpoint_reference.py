"""CPU: the NumPy reference of the landmark points (tests/lmpoint_helpers.py).  The analytic [Jp | j_rho] against central differences of the
NumPy point; the two CPU routes of the 3 x 3 covariance (full inverse of the un-eliminated system, Schur identity + Cholesky) on the oracle's
normal matrix; the status rules; constants."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def test_analytic_jacobian_against_central_differences(cv):
    """Knots: h = 1e-6 through np_oracle.retract: rounding eps / h + truncation h^2 is about 1.1e-10 for O(1) quantities; the bound 1e-8 leaves
    two orders of margin (tests/test_posecov_reference.py); the same flat bound holds here.
    Line delay: a step of 1e-6 s moves the integer-ns anchor time by exactly D = row * 1000 ns; the central difference of X(tau) over +-D has the
    truncation error D^2 / 6 |X'''|, with X''' taken from the five-point stencil of the same NumPy point at the step D, and the rounding error
    eps |X| / D; the bound is row times (twice the truncation estimate + 1e-8).  A landmark at row 0 has the exact zero column on both sides.
    Inverse depth: a relative step of 1e-6: truncation 1e-12 |j_rho| (X is p / rho: the third derivative is 6 |R p| / rho^4) and rounding
    eps |X| / (1e-6 rho), about 1e-10 |j_rho| while |X| is below a hundred depths; the bound is 1e-8 max(1, |j_rho|)."""
    import np_oracle
    import lmpoint_helpers as lh
    w = cv.synth.make_window("config1", seed=1003)
    w.ld = 2.0e-5                                                         # inside the window's box: the row time is not the frame time
    frames = sorted({int(t) for t in w.v_ti})
    picks = []
    for t in (frames[0], frames[len(frames) // 2], frames[-1]):           # the first, a middle and the last anchor frame
        ls = sorted({int(l) for l in w.v_lm[w.v_ti == t]})
        picks.append(max(ls, key=lambda l: lh.anchor_of(w, l)[1]))        # its landmark on the lowest image row: the longest line-delay lever
    h, worst, worst_m = 1e-6, [0.0, 0.0, 0.0], 0.0
    for l in picks:
        pj = lh.point_jacobian(w, l)
        assert pj is not None
        depth = 1.0 / w.rho[l]
        s = pj.s
        cols = list(range(6 * max(s - 1, 0), 6 * min(s + 5, w.K)))         # the four knots and their neighbours (no dependence)
        for j in cols:
            xi = np.zeros(w.N); xi[j] = h
            fd = (lh.point(np_oracle.retract(w, xi), l)[0] - lh.point(np_oracle.retract(w, -xi), l)[0]) / (2 * h)
            e = float(np.abs(fd - pj.Jp[:, j]).max())
            worst[0] = max(worst[0], e)
            worst_m = max(worst_m, e / max(1.0, depth))
            assert e <= 1e-8, (l, j, e)
        rest = [j for j in range(w.P - 1) if j not in cols]
        assert not pj.Jp[:, rest].any()
        # ---- line delay
        t_i, row, p_i = lh.anchor_of(w, l)
        xi = np.zeros(w.N); xi[w.P - 1] = h
        wp, wm = np_oracle.retract(w, xi), np_oracle.retract(w, -xi)
        assert lh.anchor_time(wp, t_i, row) - pj.tau == row * 1000 and pj.tau - lh.anchor_time(wm, t_i, row) == row * 1000
        fd = (lh.point(wp, l)[0] - lh.point(wm, l)[0]) / (2 * h)
        if row == 0:
            assert not fd.any() and not pj.Jp[:, w.P - 1].any()
        else:
            D = row * 1000
            X = [lh.point_at(w, pj.tau + k * D, p_i, w.rho[l]) for k in (-2, -1, 1, 2)]
            x3 = np.abs(X[3] - 2 * X[2] + 2 * X[1] - X[0]) / 2.0 / (D * 1e-9) ** 3
            tol = row * (2 * (D * 1e-9) ** 2 / 6 * float(x3.max()) + 1e-8)
            e = float(np.abs(fd - pj.Jp[:, w.P - 1]).max())
            worst[1] = max(worst[1], e / tol)
            assert e <= tol, (l, row, e, tol)
        # ---- inverse depth
        xi = np.zeros(w.N); xi[w.P + l] = h * w.rho[l]
        fd = (lh.point(np_oracle.retract(w, xi), l)[0] - lh.point(np_oracle.retract(w, -xi), l)[0]) / (2 * h * w.rho[l])
        e = float(np.abs(fd - pj.jrho).max())
        tol = 1e-8 * max(1.0, float(np.abs(pj.jrho).max()))
        worst[2] = max(worst[2], e / tol)
        assert e <= tol, (l, e, tol)
        assert np.array_equal(pj.J[:, w.P + l], pj.jrho) and not np.delete(pj.J[:, w.P:], l, axis=1).any()
    print(f"landmarks {picks}: knots {worst[0]:.3g} (absolute; {worst_m:.3g} per metre of depth), line delay {worst[1]:.3g} of its bound, "
          f"inverse depth {worst[2]:.3g} of its bound")


def oracle_reference(oracle, w):
    import cov_helpers as ch
    import lmpoint_helpers as lh
    H, _, _ = oracle.OracleWindow(w).build_normal()
    P = w.P
    return lh.joint_reference(H[:P, :P], H[:P, P:], np.diag(H)[P:], ~ch.constant_mask(w))


@pytest.fixture(scope="module")
def oracle_refs(cv, oracle, golden_dir):
    """name -> (window at the covariance fixture's state, the joint reference on the oracle's H); computed once."""
    out = {}
    for name, cfg, seed in (("tiny", "tiny", 7), ("config1", "config1", 1000)):
        fx = np.load(os.path.join(golden_dir, f"cov_{cfg}_seed{seed}.npz"))
        w = cv.synth.make_window(cfg, seed=seed)
        w.quat[:] = fx["quat"]; w.pos[:] = fx["pos"]; w.bias[:] = fx["bias"]; w.rho[:] = fx["rho"]; w.ld = float(fx["ld"])
        out[name] = (w, oracle_reference(oracle, w))
    return out


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_two_cpu_routes_agree(oracle_refs, name):
    """Full inverse of the un-eliminated system and the Schur identity with numpy.linalg.cholesky, every landmark of both fixture windows,
    within 2 x the GPU tolerance 4 kappa_s 2^-53 g; the tolerance itself stays below 1e-4."""
    import cov_helpers as ch
    import lmpoint_helpers as lh
    w, ref = oracle_refs[name]
    assert (w.P, w.L) == ((103, 12) if name == "tiny" else (211, 50))
    gs, tols, errs = [], [], []
    for l in range(w.L):
        pj = lh.point_jacobian(w, l)
        a, sa = lh.point_cov_reference(ref, pj, l, "full")
        b, sb = lh.point_cov_reference(ref, pj, l, "schur")
        assert sa == sb == lh.OK, (l, sa, sb)
        tol, g = lh.bound(ref, pj, l)
        e = ch.cov_metric(b, a)
        gs.append(g); tols.append(tol); errs.append(e)
        assert np.isfinite(ref.kappa) and tol < 1e-4, (l, tol)
        assert e <= 2 * tol, (l, e, tol)
        assert (np.diag(a) > 0).all()
    print(f"{name}: g {min(gs):.3g} .. {max(gs):.3g}, bound {min(tols):.3g} .. {max(tols):.3g}, route difference <= {max(errs):.3g}")


def test_status_rules(cv, oracle_refs):
    """rho = -1, a landmark without blocks and a landmark whose blocks name two anchor observations: status 3 and NaN; Hll == 0: status 2."""
    import lmpoint_helpers as lh
    w0, ref = oracle_refs["tiny"]
    w = w0.copy()
    w.rho[2] = -1.0
    X, st = lh.point(w, 2)
    assert st == lh.NONE and np.isnan(X).all() and lh.point_jacobian(w, 2) is None
    c, sc = lh.point_cov_reference(ref, None, 2)
    assert sc == lh.NONE and np.isnan(c).all()
    assert lh.point(w, 3)[1] == lh.OK
    w = w0.copy()
    keep = w.v_lm != 4
    for a in ("v_lm", "v_ti", "v_tj", "v_rowi", "v_rowj", "v_pi", "v_pj"):
        setattr(w, a, getattr(w, a)[keep])
    assert lh.anchor_of(w, 4) is None and lh.point(w, 4)[1] == lh.NONE and lh.point(w, 5)[1] == lh.OK
    w = w0.copy()
    v = np.nonzero(w.v_lm == 6)[0]
    assert v.shape[0] >= 2
    w.v_pi[v[-1], 0] += 1e-3
    assert lh.anchor_of(w, 6) is None and lh.point(w, 6)[1] == lh.NONE
    w = w0.copy()
    w.ld = 1.0                                   # tau far beyond the spline for every row > 0
    l = next(l for l in range(w.L) if lh.anchor_of(w, l)[1] > 0)
    assert lh.point(w, l)[1] == lh.NONE
    ref0 = lh.joint_reference(ref.Hpp, ref.W, np.where(np.arange(ref.L) == 1, 0.0, ref.Hll), np.ones(ref.P))
    c, sc = lh.point_cov_reference(ref0, lh.point_jacobian(w0, 1), 1)
    assert sc == lh.NO_INFO and np.isposinf(np.diag(c)).all() and not c[~np.eye(3, dtype=bool)].any()


def test_constants(cv, oracle):
    """fixed_upto = 3 on `tiny`: a landmark anchored under constant knots alone keeps only its depth term and the free unknowns' share -- the
    covariance equals the one with Jp's knot columns zeroed, and differs from the free window's.  fix_ld = True removes the line-delay column."""
    import cov_helpers as ch
    import lmpoint_helpers as lh
    w = cv.synth.make_window("tiny", seed=7)
    wf = w.copy(); wf.fixed_upto = 3; wf.normalize()
    ref, reff = oracle_reference(oracle, w), oracle_reference(oracle, wf)
    assert not np.isin(np.arange(24), reff.kp).any() and (w.P - 1) in reff.kp
    under = [l for l in range(w.L) if max(lh.point_jacobian(wf, l).knots) <= 3]
    assert under, "no landmark of `tiny` is anchored under knots 0..3"
    for l in under:
        pj = lh.point_jacobian(wf, l)
        assert pj.Jp[:, :24].any()
        a, st = lh.point_cov_reference(reff, pj, l, "full")
        b, _ = lh.point_cov_reference(reff, pj, l, "schur")
        assert st == lh.OK and (np.diag(a) > 0).all()
        tol, _ = lh.bound(reff, pj, l)
        assert tol < 1e-4 and ch.cov_metric(b, a) <= 2 * tol
        # only j_rho and the line-delay column act: the same with every knot column of Jp removed
        pz = lh.point_jacobian(wf, l)
        pz.Jp[:, :6 * w.K] = 0.0
        z, _ = lh.point_cov_reference(reff, pz, l, "full")
        assert np.array_equal(z, a)
        free, _ = lh.point_cov_reference(ref, lh.point_jacobian(w, l), l, "full")
        assert ch.cov_metric(a, free) > 1e-3
    wl = w.copy(); wl.fix_ld = True; wl.normalize()
    refl = oracle_reference(oracle, wl)
    assert (w.P - 1) not in refl.kp
    l = next(l for l in range(w.L) if lh.anchor_of(w, l)[1] > 0)
    pj = lh.point_jacobian(wl, l)
    a, _ = lh.point_cov_reference(refl, pj, l, "full")
    pz = lh.point_jacobian(wl, l)
    pz.Jp[:, w.P - 1] = 0.0
    assert np.array_equal(lh.point_cov_reference(refl, pz, l, "full")[0], a)
    b, _ = lh.point_cov_reference(refl, pj, l, "schur")
    tol, _ = lh.bound(refl, pj, l)
    assert tol < 1e-4 and ch.cov_metric(b, a) <= 2 * tol
