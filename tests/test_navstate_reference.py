"""CPU: the NumPy reference of the navigation-state covariance (tests/navstate_helpers.py).  The analytic Jacobian against central differences
of the oracle's NumPy spline evaluation; the two CPU routes of the covariance (full inverse, Schur + Cholesky) mapped through J on the oracle's
normal matrix, entry by entry at 2 x the bound 4 kappa_s 2^-53 sqrt(g_a g_b); the zero, +inf and NaN rules."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

FRAME_DT = 100_000_000      # synth.py: frame_dt_ns of every configuration used here
TINY_QUERIES = [(0, 0.0), (1, 0.9), (5, 0.37), (7, 0.999), (8, 0.0)]


@pytest.mark.parametrize("u", [0.0, 0.37, 0.999])
def test_analytic_jacobian_against_central_differences(cv, u):
    """h = 1e-6, bound 1e-8 (the pose reference's): every one of the 15 outputs against every unknown of the four knots, their neighbours and
    all bias states."""
    import np_oracle
    import navstate_helpers as nh
    w = cv.synth.make_window("config1", seed=1003)
    h, worst = 1e-6, 0.0

    def state(x, t, f):
        R, p, v, b = nh.nav_numpy(x, t, f)
        return R, np.concatenate([p, v, b])

    for s, f in ((0, 0), (7, None), (w.K - 4, 3)):
        t = nh.time_of(w, s, u)
        jac = nh.nav_jacobian(w, t, f)
        assert jac.s == s and jac.knots == list(range(s, s + (4 if jac.u > 0 else 3))) and jac.frame == (w.F - 1 if f is None else f)
        R0, _ = state(w, t, f)
        cols = list(range(6 * max(s - 1, 0), 6 * min(s + 5, w.K))) + list(range(6 * w.K, 6 * w.K + 6 * w.F))
        for j in cols:
            xi = np.zeros(w.N); xi[j] = h
            Rp, xp = state(np_oracle.retract(w, xi), t, f)
            Rm, xm = state(np_oracle.retract(w, -xi), t, f)
            fd = np.concatenate([((R0.inv() * Rp).as_rotvec() - (R0.inv() * Rm).as_rotvec()) / (2 * h), (xp - xm) / (2 * h)])
            worst = max(worst, float(np.abs(fd - jac.J[:, j]).max()))
        assert not jac.J[:, [j for j in range(w.P) if j not in cols]].any()
        if jac.u == 0.0:
            assert jac.cv[3] == 0.0 and not jac.J[:, 6 * (s + 3):6 * (s + 4)].any()
    print(f"u {u}: max |J - fd| {worst:.3g}")
    assert worst <= 1e-8


@pytest.fixture(scope="module")
def oracle_refs(cv, oracle, golden_dir):
    """name -> (window at the covariance fixture's state, cov_reference over all P unknowns on the oracle's H); computed once."""
    import cov_helpers as ch
    out = {}
    for name, cfg, seed in (("tiny", "tiny", 7), ("config1", "config1", 1000)):
        fx = np.load(os.path.join(golden_dir, f"cov_{cfg}_seed{seed}.npz"))
        w = cv.synth.make_window(cfg, seed=seed)
        w.quat[:] = fx["quat"]; w.pos[:] = fx["pos"]; w.bias[:] = fx["bias"]; w.rho[:] = fx["rho"]; w.ld = float(fx["ld"])
        H, _, _ = oracle.OracleWindow(w).build_normal()
        P = w.P
        out[name] = (w, ch.cov_reference(H[:P, :P], H[:P, P:], np.diag(H)[P:], ~ch.constant_mask(w), range(P)))
    return out


def queries(name, w):
    """`tiny`: the five in-range queries of the GPU test with frames i mod F; `config1`: every frame time with its own bias state, and the same
    times with the newest."""
    import navstate_helpers as nh
    if name == "tiny":
        return [(nh.time_of(w, s, u), i % w.F) for i, (s, u) in enumerate(TINY_QUERIES)]
    frames = [int(w.t0_ns + f * FRAME_DT) for f in range(w.F)]
    return [(t, f) for f, t in enumerate(frames)] + [(t, None) for t in frames]


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_two_cpu_routes_agree_through_J(oracle_refs, name):
    """Full inverse and Schur + Cholesky, each mapped through J, entry by entry within 2 x the GPU tolerance 4 kappa_s 2^-53 sqrt(g_a g_b); the
    tolerance itself stays below 1e-4 among pose and bias rows and below 1e-3 where a velocity row is involved."""
    import cov_helpers as ch
    import navstate_helpers as nh
    w, ref = oracle_refs[name]
    gp, gb, gv, bv, err = 0.0, 0.0, 0.0, 0.0, 0.0
    for t, f in queries(name, w):
        jac = nh.nav_jacobian(w, t, f)
        a, sa = nh.nav_cov_reference(ref, jac, w.K, "full")
        b, sb = nh.nav_cov_reference(ref, jac, w.K, "schur")
        assert sa == sb == nh.OK, (t, f, sa, sb)
        g = nh.row_amplification(jac.J, ref.cov_full)
        tol, cap = nh.entry_bounds(ch.bound(ref.kappa), g)
        e = nh.entry_errors(b, a)
        gp, gb, gv = max(gp, g[nh.POSE].max()), max(gb, g[9:].max()), max(gv, g[nh.VEL].max())
        bv, err = max(bv, tol.max()), max(err, e.max())
        assert (tol < cap).all(), (t, f, tol.max())
        assert (e <= 2 * tol).all(), (t, f, float((e / tol).max()))
    print(f"{name}: kappa_s {ref.kappa:.3g}, g pose <= {gp:.3g}, bias {gb:.3g}, velocity <= {gv:.3g}, largest bound {bv:.3g}, route difference <= {err:.3g}")
    assert abs(gb - 1.0) <= 4 * ch.EPS                 # one-hot rows: sqrt(Sigma_kk)^2 / Sigma_kk


def test_zero_inf_and_nan_rules(cv, oracle, oracle_refs):
    import cov_helpers as ch
    import navstate_helpers as nh
    w, ref = oracle_refs["tiny"]
    assert w.K == 12 and ref.untouched[6 * 11:6 * 12].all()
    cov, st = nh.nav_cov_reference(ref, nh.nav_jacobian(w, nh.time_of(w, 8, 0.5), 0), w.K)      # depends on the untouched last knot
    assert st == nh.UNTOUCHED and np.isposinf(np.diag(cov)).all() and not cov[~np.eye(15, dtype=bool)].any()
    cov, st = nh.nav_cov_reference(ref, nh.nav_jacobian(w, nh.time_of(w, 8, 0.0), 0), w.K)      # u = 0: it does not
    assert st == nh.OK and np.isfinite(cov).all() and (np.diag(cov) > 0).all()
    for t in (w.t0_ns - 1, w.t0_ns + (w.K - 3) * w.dt_ns):
        assert nh.nav_jacobian(w, t) is None
        cov, st = nh.nav_cov_reference(ref, None, w.K)
        assert st == nh.OUTSIDE and np.isnan(cov).all()
    wf = cv.synth.make_window("tiny", seed=7)
    wf.fixed_upto = 3
    wf.lock_bg = 1
    wf.normalize()
    H, _, _ = oracle.OracleWindow(wf).build_normal()
    P = wf.P
    reff = ch.cov_reference(H[:P, :P], H[:P, P:], np.diag(H)[P:], ~ch.constant_mask(wf), range(P))
    cov, st = nh.nav_cov_reference(reff, nh.nav_jacobian(wf, nh.time_of(wf, 0, 0.0)), wf.K)    # knots 0..2 constant, bg locked: only ba is left
    assert st == nh.OK and not cov[:12].any() and not cov[:, :12].any() and (np.diag(cov)[12:] > 0).all()
    cov, st = nh.nav_cov_reference(reff, nh.nav_jacobian(wf, nh.time_of(wf, 1, 0.5)), wf.K)    # knots 1..4: only knot 4 contributes
    d = np.diag(cov)
    assert st == nh.OK and (d[:9] > 0).all() and not cov[9:12].any() and not cov[:, 9:12].any() and (d[12:] > 0).all()
