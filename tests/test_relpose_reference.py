"""CPU: the NumPy reference of the relative-pose covariance (tests/relpose_helpers.py).  The analytic Jacobian against central differences of
the oracle's NumPy spline evaluation; the two CPU routes of the covariance (full inverse, Schur + Cholesky) mapped through J_rel on the
oracle's normal matrix, entry by entry at 2 x the bound 4 kappa_s 2^-53 sqrt(g_a g_b); the zero, +inf and NaN rules."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

EXT = (np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9]), np.array([0.05, -0.02, 0.1]))
# (s, u) -> (s, u): overlapping spans, disjoint spans, the same segment, b before a (disjoint and overlapping)
FD_PAIRS = [((2, 0.3), (4, 0.75)), ((1, 0.9), (9, 0.37)), ((5, 0.37), (5, 0.87)), ((9, 0.5), (2, 0.25)), ((4, 0.0), (3, 0.6)), ((0, 0.0), (3, 0.0))]
TINY_PAIRS = [((0, 0.0), (1, 0.9)), ((1, 0.9), (5, 0.37)), ((0, 0.0), (8, 0.0)), ((7, 0.5), (2, 0.25)), ((3, 0.2), (4, 0.2)), ((4, 0.5), (6, 0.5))]
FRAME_DT = 100_000_000      # synth.py: frame_dt_ns of every configuration used here


@pytest.mark.parametrize("ext", [False, True], ids=["body", "extrinsic"])
def test_analytic_jacobian_against_central_differences(cv, ext):
    """h = 1e-6, bound 1e-8 (the pose reference's): the six outputs against every unknown of the knots of both poses and their neighbours."""
    import np_oracle
    import relpose_helpers as rh
    w = cv.synth.make_window("config1", seed=1003)
    q_SI, p_SI = EXT if ext else (None, None)
    h, worst = 1e-6, 0.0
    for (sa, ua), (sb, ub) in FD_PAIRS:
        ta, tb = rh.time_of(w, sa, ua), rh.time_of(w, sb, ub)
        jac = rh.rel_jacobian(w, ta, tb, q_SI, p_SI)
        assert jac.a.s == sa and jac.b.s == sb
        R0, p0 = rh.rel_numpy(w, ta, tb, q_SI, p_SI)
        assert (R0.inv() * rh.Rot.from_matrix(jac.R_ab)).magnitude() <= 1e-12 and np.abs(p0 - jac.p_ab).max() <= 1e-12 * max(1.0, np.abs(p0).max())
        cols = sorted(set(j for s in (sa, sb) for j in range(6 * max(s - 1, 0), 6 * min(s + 5, w.K))))
        for j in cols:
            xi = np.zeros(w.N); xi[j] = h
            Rp, pp = rh.rel_numpy(np_oracle.retract(w, xi), ta, tb, q_SI, p_SI)
            Rm, pm = rh.rel_numpy(np_oracle.retract(w, -xi), ta, tb, q_SI, p_SI)
            fd = np.concatenate([((R0.inv() * Rp).as_rotvec() - (R0.inv() * Rm).as_rotvec()) / (2 * h), (pp - pm) / (2 * h)])
            worst = max(worst, float(np.abs(fd - jac.J[:, j]).max()))
        assert not jac.J[:, [j for j in range(w.P) if j not in cols]].any()
    print(f"{'extrinsic' if ext else 'body'}: max |J - fd| {worst:.3g}")
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
    """`tiny`: the six in-range pairs of the GPU test, body, and the first four with the extrinsic; `config1`: the consecutive frame pairs (body
    and with the window's camera extrinsic), (0, F - 1), (F - 1, 0), (3, 7) and the same-segment pair (body and with the synthetic extrinsic)."""
    import relpose_helpers as rh
    if name == "tiny":
        ts = [(rh.time_of(w, *a), rh.time_of(w, *b)) for a, b in TINY_PAIRS]
        return [(ta, tb, None, None) for ta, tb in ts] + [(ta, tb) + EXT for ta, tb in ts[:4]]
    fr = [int(w.t0_ns + f * FRAME_DT) for f in range(w.F)]
    out = [(fr[f], fr[f + 1], None, None) for f in range(w.F - 1)] + [(fr[f], fr[f + 1], w.q_CI, w.p_CI) for f in range(w.F - 1)]
    out += [(fr[0], fr[-1], None, None), (fr[-1], fr[0], None, None), (fr[3], fr[7], None, None)]
    same = (rh.time_of(w, 5, 0.37), rh.time_of(w, 5, 0.87))
    return out + [same + (None, None), same + EXT]


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_two_cpu_routes_agree_through_J(oracle_refs, name):
    """Full inverse and Schur + Cholesky, each mapped through J_rel, entry by entry within 2 x the GPU tolerance 4 kappa_s 2^-53 sqrt(g_a g_b);
    the tolerance itself stays below the cap 1e-3."""
    import cov_helpers as ch
    import relpose_helpers as rh
    w, ref = oracle_refs[name]
    gmax, bmax, err = 0.0, 0.0, 0.0
    for ta, tb, q, p in queries(name, w):
        jac = rh.rel_jacobian(w, ta, tb, q, p)
        a, sa = rh.rel_cov_reference(ref, jac, "full")
        b, sb = rh.rel_cov_reference(ref, jac, "schur")
        assert sa == sb == rh.OK, (ta, tb, sa, sb)
        g = rh.row_amplification(jac.J, ref.cov_full)
        tol = rh.entry_bounds(ch.bound(ref.kappa), g)
        e = rh.entry_errors(b, a)
        gmax, bmax, err = max(gmax, g.max()), max(bmax, tol.max()), max(err, e.max())
        assert (tol < rh.CAP).all(), (ta, tb, tol.max())
        assert (e <= 2 * tol).all(), (ta, tb, float((e / tol).max()))
    print(f"{name}: kappa_s {ref.kappa:.3g}, g <= {gmax:.3g}, largest bound {bmax:.3g}, route difference <= {err:.3g}")


def test_zero_inf_and_nan_rules(cv, oracle, oracle_refs):
    import cov_helpers as ch
    import relpose_helpers as rh
    w, ref = oracle_refs["tiny"]
    assert w.K == 12 and ref.untouched[6 * 11:6 * 12].all()
    inside, needs11 = rh.time_of(w, 1, 0.9), rh.time_of(w, 8, 0.5)       # (8, 0.5) depends on the untouched last knot
    for ta, tb in ((needs11, inside), (inside, needs11)):
        cov, st = rh.rel_cov_reference(ref, rh.rel_jacobian(w, ta, tb))
        assert st == rh.UNTOUCHED and np.isposinf(np.diag(cov)).all() and not cov[rh.OFF].any()
    cov, st = rh.rel_cov_reference(ref, rh.rel_jacobian(w, inside, rh.time_of(w, 8, 0.0)))      # u = 0: it does not
    assert st == rh.OK and np.isfinite(cov).all() and (np.diag(cov) > 0).all()
    for ta, tb in ((w.t0_ns - 1, inside), (inside, w.t0_ns + (w.K - 3) * w.dt_ns), (needs11, w.t0_ns - 1)):      # the last: 3 takes precedence over 2
        jac = rh.rel_jacobian(w, ta, tb)
        assert jac is None
        cov, st = rh.rel_cov_reference(ref, jac)
        assert st == rh.OUTSIDE and np.isnan(cov).all()
    wf = cv.synth.make_window("tiny", seed=7)
    wf.fixed_upto = 3
    wf.normalize()
    H, _, _ = oracle.OracleWindow(wf).build_normal()
    P = wf.P
    reff = ch.cov_reference(H[:P, :P], H[:P, P:], np.diag(H)[P:], ~ch.constant_mask(wf), range(P))
    cov, st = rh.rel_cov_reference(reff, rh.rel_jacobian(wf, rh.time_of(wf, 0, 0.0), rh.time_of(wf, 1, 0.0)))    # knots 0..3: constant
    assert st == rh.OK and not cov.any()
    cov, st = rh.rel_cov_reference(reff, rh.rel_jacobian(wf, rh.time_of(wf, 0, 0.0), rh.time_of(wf, 1, 0.5)))    # only knot 4 contributes
    assert st == rh.OK and (np.diag(cov) > 0).all()
    jac = rh.rel_jacobian(wf, rh.time_of(wf, 2, 0.4), rh.time_of(wf, 2, 0.4))                                    # t_a == t_b: J vanishes up to rounding
    assert np.abs(jac.J).max() <= 1e-14 and np.abs(jac.p_ab).max() == 0.0
