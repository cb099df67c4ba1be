"""CPU: the NumPy reference of the landmark projections (tests/projection_helpers.py).  The value against the oracle's visual residuals; the
analytic [Jp | j] against central differences of those residuals; the two CPU routes of the 2 x 2 covariance (full inverse of the
un-eliminated system, Schur identity + Cholesky) on the oracle's normal matrix; the status rules; constants; the row iteration."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

EPS = 2.0 ** -53
WINDOWS = (("tiny", "tiny", 7), ("config1", "config1", 1000))


def with_ld_ns(w, n):
    """A copy of w whose line delay truncates to exactly n integer ns."""
    w2 = w.copy()
    w2.ld = (n + (0.5 if n >= 0 else -0.5)) * 1e-9
    assert int(np.int64(w2.ld * 1e9)) == n
    return w2


@pytest.mark.parametrize("name,cfg,seed", WINDOWS, ids=[x[0] for x in WINDOWS])
def test_value_and_jacobian_against_the_visual_residuals(cv, name, cfg, seed):
    """Every visual block v = (l, t_j, row_j, p_j): img_w (proj.xy - p_j) is np_oracle.residuals(w)["vis"][v].  Both sides are the same NumPy
    spline evaluation composed in a different order; the rounding of y is a few eps (|X| + |p_Cq|), through Pi and img_w:
    32 eps img_w (1 + |z|) (|X| + |p_Cq|) / depth.
    Knots and inverse depth: img_w J against np_oracle.fd_jacobian of the block's two rows, h = 1e-6: rounding eps / h + truncation h^2, the flat
    bound 1e-8 of tests/test_lmpoint_reference.py relative to max(1, the block's largest entry).
    Line delay: a step of 1e-6 s moves the integer-ns delay by exactly 1000 ns; the central difference of proj over +-1000 ns has the truncation
    error h^2 / 6 |f'''| with f''' from the five-point stencil of the same NumPy projection; the bound is twice that + 1e-8 max(1, |column|)."""
    import np_oracle
    import lmpoint_helpers as lh
    import projection_helpers as pr
    w = cv.synth.make_window(cfg, seed=seed)
    res = np_oracle.residuals(w)["vis"]
    n_imu = np_oracle.residuals(w)["imu"].size
    cols = list(range(w.P - 1)) + list(range(w.P, w.N))
    fd = np_oracle.fd_jacobian(w, cols)[n_imu:n_imu + 2 * w.V]
    ld_ns = int(np.int64(w.ld * 1e9))
    h = 1e-6
    worst, n_ld = [0.0, 0.0, 0.0], 0
    for v in range(w.V):
        l, t, row = int(w.v_lm[v]), int(w.v_tj[v]), int(w.v_rowj[v])
        proj, r_out, st = pr.project(w, l, t, row)
        assert st == pr.OK and r_out == row
        pj = pr.projection_jacobian(w, l, t, row)
        X = lh.point(w, l)[0]
        tol = 32 * EPS * w.img_w * (1 + np.abs(proj[:2]).max()) * (2 * np.linalg.norm(X) + np.linalg.norm(pj.y)) / proj[2]   # (|p_Cq| <= |X| + |y|)
        e = float(np.abs(w.img_w * (proj[:2] - w.v_pj[v]) - res[v]).max())
        worst[0] = max(worst[0], e)
        assert e <= tol, (v, e, tol)
        Ja = w.img_w * pj.J[:, cols]
        scale = max(1.0, float(np.abs(Ja).max()))
        e = float(np.abs(fd[2 * v:2 * v + 2] - Ja).max() / scale)
        worst[1] = max(worst[1], e)
        assert e <= 1e-8, (v, e)
        # ---- line delay
        f = {k: pr.project(with_ld_ns(w, ld_ns + 1000 * k), l, t, row)[0][:2] for k in (-2, -1, 1, 2)}
        col = pj.Jp[:, w.P - 1]
        if int(w.v_rowi[v]) == 0 and row == 0:
            assert not col.any() and np.array_equal(f[1], f[-1])
            continue
        if not all(np.isfinite(x).all() for x in f.values()):      # a time at the very start or end of the spline: the stencil leaves it
            continue
        n_ld += 1
        x3 = np.abs(f[2] - 2 * f[1] + 2 * f[-1] - f[-2]) / 2.0 / h ** 3
        tol = 2 * h ** 2 / 6 * float(x3.max()) + 1e-8 * max(1.0, float(np.abs(col).max()))
        e = float(np.abs((f[1] - f[-1]) / (2 * h) - col).max())
        worst[2] = max(worst[2], e / tol)
        assert e <= tol, (v, e, tol)
    assert n_ld > w.V // 2
    print(f"{name}: {w.V} blocks ({n_ld} with a line-delay stencil): residual identity {worst[0]:.3g}, knots and inverse depth {worst[1]:.3g} (relative), line delay {worst[2]:.3g} of its bound")


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
    for name, cfg, seed in WINDOWS:
        fx = np.load(os.path.join(golden_dir, f"cov_{cfg}_seed{seed}.npz"))
        w = cv.synth.make_window(cfg, seed=seed)
        w.quat[:] = fx["quat"]; w.pos[:] = fx["pos"]; w.bias[:] = fx["bias"]; w.rho[:] = fx["rho"]; w.ld = float(fx["ld"])
        out[name] = (w, oracle_reference(oracle, w))
    return out


def queries_of(w):
    """Each landmark's own observations, and every landmark into the newest frame at rows 0, 240 and 479."""
    q = [(int(w.v_lm[v]), int(w.v_tj[v]), int(w.v_rowj[v])) for v in range(w.V)]
    t_new = int(max(w.v_tj.max(), w.v_ti.max()))
    return q + [(l, t_new, row) for l in range(w.L) for row in (0, 240, 479)]


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_two_cpu_routes_agree(oracle_refs, name):
    """Full inverse of the un-eliminated system and the Schur identity with numpy.linalg.cholesky within 2 x the GPU tolerance
    4 kappa_s 2^-53 g; the tolerance itself stays below 1e-2 (g reaches 32 on `tiny` and 1.6e3 on `config1`: the flat 1e-4 of the landmark
    points does not hold for this quantity)."""
    import cov_helpers as ch
    import projection_helpers as pr
    w, ref = oracle_refs[name]
    assert (w.P, w.L) == ((103, 12) if name == "tiny" else (211, 50))
    gs, tols, ratios, n_ok = [], [], [], 0
    for i, (l, t, row) in enumerate(queries_of(w)):
        pj = pr.projection_jacobian(w, l, t, row)
        a, sa = pr.proj_cov_reference(ref, pj, l, "full")
        b, sb = pr.proj_cov_reference(ref, pj, l, "schur")
        assert sa == sb, (l, t, row, sa, sb)
        if i < w.V:
            assert sa == pr.OK, (l, t, row, sa)
        if sa != pr.OK:
            continue
        n_ok += 1
        tol, g = pr.bound(ref, pj, l)
        e = ch.cov_metric(b, a)
        gs.append(g); tols.append(tol); ratios.append(e / tol)
        assert np.isfinite(ref.kappa) and tol < 1e-2, (l, t, row, tol)
        assert e <= 2 * tol, (l, t, row, e, tol)
        assert (np.diag(a) > 0).all()
    assert n_ok > w.V
    print(f"{name}: {n_ok} queries, g {min(gs):.3g} .. {max(gs):.3g}, worst bound {max(tols):.3g}, route difference <= {max(ratios):.3g} of the bound")


def test_status_rules(cv, oracle_refs):
    """rho = -1 and a landmark whose blocks name two anchors: status 3 and NaN; a time in the last segment with u > 0 depends on the padding
    knot no factor touches: status 2, +inf diagonal -- at u = 0 it does not; a time outside the spline: status 3; Hll == 0: status 2."""
    import lmpoint_helpers as lh
    import posecov_helpers as ph
    import projection_helpers as pr
    w0, ref = oracle_refs["tiny"]
    t_in = int(w0.v_tj[0])
    w = w0.copy()
    w.rho[2] = -1.0
    p, r, st = pr.project(w, 2, t_in, 0)
    assert st == pr.NONE and r == -1 and np.isnan(p).all() and pr.projection_jacobian(w, 2, t_in, 0) is None
    c, sc = pr.proj_cov_reference(ref, None, 2)
    assert sc == pr.NONE and np.isnan(c).all()
    assert pr.project(w, 3, t_in, 0)[2] == pr.OK
    w = w0.copy()
    v = np.nonzero(w.v_lm == 6)[0]
    assert v.shape[0] >= 2
    w.v_pi[v[-1], 0] += 1e-3
    assert pr.project(w, 6, t_in, 0)[2] == pr.NONE and pr.project(w, 5, t_in, 0)[2] == pr.OK
    # ---- the last segment
    K = w0.K
    assert (np.diag(ref.Hpp)[6 * (K - 1):6 * K] == 0).all(), "the padding knot of `tiny` is touched"
    for u, want in ((0.5, pr.NO_INFO), (0.0, pr.OK)):
        t = ph.time_of(w0, K - 4, u)
        p, _, st = pr.project(w0, 0, t, 0)
        assert st == pr.OK and np.isfinite(p).all()
        pj = pr.projection_jacobian(w0, 0, t, 0)
        assert (K - 1 in pj.knots) == (u > 0)
        for route in ("full", "schur"):
            c, sc = pr.proj_cov_reference(ref, pj, 0, route)
            assert sc == want, (u, sc)
            if want == pr.NO_INFO:
                assert np.isposinf(np.diag(c)).all() and c[0, 1] == 0 and c[1, 0] == 0
    # ---- outside the spline
    for t in (ph.time_of(w0, K - 3, 0.0), int(w0.t0_ns) - 1):
        p, r, st = pr.project(w0, 0, t, 0)
        assert st == pr.NONE and r == -1 and np.isnan(p).all()
    assert pr.project(w0, 0, ph.time_of(w0, K - 3, 0.0) - 1, 0)[2] == pr.OK and pr.project(w0, 0, int(w0.t0_ns), 0)[2] == pr.OK
    w = w0.copy()
    w.ld = 1.0                                   # tau_q far beyond the spline for every row > 0
    assert pr.project(w, 0, t_in, 5)[2] == pr.NONE
    # ---- Hll == 0
    ref0 = lh.joint_reference(ref.Hpp, ref.W, np.where(np.arange(ref.L) == 1, 0.0, ref.Hll), np.ones(ref.P))
    c, sc = pr.proj_cov_reference(ref0, pr.projection_jacobian(w0, 1, t_in, 0), 1)
    assert sc == pr.NO_INFO and np.isposinf(np.diag(c)).all() and c[0, 1] == 0 and c[1, 0] == 0


def test_constants(cv, oracle):
    """fixed_upto = 3 on `tiny`: a query whose two times lie under constant knots alone keeps only its depth term and the free unknowns'
    share -- the covariance equals the one with Jp's knot columns zeroed, and differs from the free window's.  fix_ld = True removes the
    line-delay column."""
    import cov_helpers as ch
    import lmpoint_helpers as lh
    import posecov_helpers as ph
    import projection_helpers as pr
    w = cv.synth.make_window("tiny", seed=7)
    wf = w.copy(); wf.fixed_upto = 3; wf.normalize()
    ref, reff = oracle_reference(oracle, w), oracle_reference(oracle, wf)
    assert not np.isin(np.arange(24), reff.kp).any() and (w.P - 1) in reff.kp
    t = ph.time_of(w, 0, 0.25)                                         # knots 0 .. 3
    under = [l for l in range(w.L) if max(lh.point_jacobian(wf, l).knots) <= 3]
    assert under, "no landmark of `tiny` is anchored under knots 0..3"
    for l in under:
        pj = pr.projection_jacobian(wf, l, t, 7)
        assert max(pj.knots) <= 3 and pj.Jp[:, :24].any()
        a, st = pr.proj_cov_reference(reff, pj, l, "full")
        b, _ = pr.proj_cov_reference(reff, pj, l, "schur")
        assert st == pr.OK and (np.diag(a) > 0).all()
        tol, _ = pr.bound(reff, pj, l)
        assert tol < 1e-2 and ch.cov_metric(b, a) <= 2 * tol
        pz = pr.projection_jacobian(wf, l, t, 7)
        pz.Jp[:, :6 * w.K] = 0.0
        z, _ = pr.proj_cov_reference(reff, pz, l, "full")
        assert np.array_equal(z, a)
        free, _ = pr.proj_cov_reference(ref, pr.projection_jacobian(w, l, t, 7), l, "full")
        assert ch.cov_metric(a, free) > 1e-3
    wl = w.copy(); wl.fix_ld = True; wl.normalize()
    refl = oracle_reference(oracle, wl)
    assert (w.P - 1) not in refl.kp
    l, t = int(w.v_lm[0]), int(w.v_tj[0])
    pj = pr.projection_jacobian(wl, l, t, 200)
    assert pj.Jp[:, w.P - 1].any()
    a, _ = pr.proj_cov_reference(refl, pj, l, "full")
    pz = pr.projection_jacobian(wl, l, t, 200)
    pz.Jp[:, w.P - 1] = 0.0
    assert np.array_equal(pr.proj_cov_reference(refl, pz, l, "full")[0], a)
    b, _ = pr.proj_cov_reference(refl, pj, l, "schur")
    tol, _ = pr.bound(refl, pj, l)
    assert tol < 1e-2 and ch.cov_metric(b, a) <= 2 * tol


def test_row_iteration_reaches_a_fixed_point(oracle_refs):
    """`config1` at the fixture state (ld != 0), every landmark into the newest frame -- the front end's use --, a synthetic pinhole row map
    fy = 460, cy = 240 over 480 rows, first guess rows / 2: three iterations reach a fixed point (a fourth changes nothing), and the final row is
    lrint(fy proj.y + cy) of the returned value.  (The map row -> fy y.y / y.z + cy has the slope fy ld |dy/dt|, about 5e-3 rows per row here:
    the first iteration lands within a row of the fixed point, the second on it, unless the image point sits within that slope of a rounding
    boundary, where no fixed point need exist; none of these queries does.)"""
    import projection_helpers as pr
    w, _ = oracle_refs["config1"]
    assert w.ld != 0.0
    fy, cy, rows = 460.0, 240.0, 480
    moved = 0
    for l, t, _ in queries_of(w)[w.V::3]:
        p3, r3, s3 = pr.project(w, l, t, rows // 2, (fy, cy, rows, 3))
        p4, r4, s4 = pr.project(w, l, t, rows // 2, (fy, cy, rows, 4))
        assert s3 == s4 == pr.OK and r3 == r4 and np.array_equal(p3, p4), (l, t, r3, r4)
        assert r3 == int(min(max(np.rint(fy * p3[1] + cy), 0), rows - 1)), (l, t, r3, p3)
        pg, rg, sg = pr.project(w, l, t, r3)
        assert sg == pr.OK and rg == r3 and np.array_equal(pg, p3)
        moved += r3 != rows // 2
    assert moved > 0
