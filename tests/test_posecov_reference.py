"""CPU: the NumPy reference of the pose covariance (tests/posecov_helpers.py).  The analytic Jacobian against central differences of the
oracle's NumPy spline evaluation; the two CPU routes of the covariance (full inverse, Schur + Cholesky) mapped through J on the oracle's
normal matrix; the zero and +inf rules."""
import os
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

FRAME_DT = 100_000_000      # synth.py: frame_dt_ns of every configuration used here
TINY_QUERIES = [(0, 0.0), (1, 0.9), (5, 0.37), (7, 0.999), (8, 0.0)]


def config1_times(w):
    """All frame times plus the row times t + row * ld for rows 0 and 479 (the time exactly as the factors take it: integer-ns line delay)."""
    ld_ns = int(w.ld * 1e9)
    frames = [int(w.t0_ns + f * FRAME_DT) for f in range(w.F)]
    return frames + [t + row * ld_ns for t in frames for row in (0, 479)]


@pytest.mark.parametrize("cam", [False, True], ids=["body", "camera"])
@pytest.mark.parametrize("u", [0.0, 0.37, 0.999])
def test_analytic_jacobian_against_central_differences(cv, u, cam):
    """h = 1e-6: rounding eps / h + truncation h^2 is about 1.1e-10 for O(1) quantities; the bound 1e-8 leaves two orders of margin."""
    import np_oracle
    import posecov_helpers as ph
    w = cv.synth.make_window("config1", seed=1003)
    ext = (w.q_CI, w.p_CI) if cam else (None, None)
    h, worst = 1e-6, 0.0
    for s in (0, 7, w.K - 4):
        t = ph.time_of(w, s, u)
        jac = ph.pose_jacobian(w, t, *ext)
        assert jac.s == s and jac.knots == list(range(s, s + (4 if jac.u > 0 else 3)))
        R0, p0 = ph.pose_numpy(w, t, *ext)
        cols = list(range(6 * max(s - 1, 0), 6 * min(s + 5, w.K)))      # the four knots and their neighbours (no dependence)
        for j in cols:
            xi = np.zeros(w.N); xi[j] = h
            Rp, pp = ph.pose_numpy(np_oracle.retract(w, xi), t, *ext)
            Rm, pm = ph.pose_numpy(np_oracle.retract(w, -xi), t, *ext)
            fd = np.concatenate([((R0.inv() * Rp).as_rotvec() - (R0.inv() * Rm).as_rotvec()) / (2 * h), (pp - pm) / (2 * h)])
            worst = max(worst, float(np.abs(fd - jac.J[:, j]).max()))
        assert not jac.J[:, [j for j in range(w.P) if j not in cols]].any()
    print(f"u {u}, {'camera' if cam else 'body'}: max |J - fd| {worst:.3g}")
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


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_two_cpu_routes_agree_through_J(oracle_refs, name):
    """Full inverse and Schur + Cholesky, each mapped through J, within 2 x the GPU tolerance 4 kappa_s 2^-53 g; the tolerance itself stays
    below 1e-4 (the smallest modelling error the covariance tests are built to catch)."""
    import cov_helpers as ch
    import posecov_helpers as ph
    w, ref = oracle_refs[name]
    times = [ph.time_of(w, s, u) for s, u in TINY_QUERIES] if name == "tiny" else config1_times(w)
    exts = [(None, None)] if name == "tiny" else [(None, None), (w.q_CI, w.p_CI)]
    gs, tols, errs = [], [], []
    for ext in exts:
        for t in times:
            jac = ph.pose_jacobian(w, t, *ext)
            a, sa = ph.pose_cov_reference(ref, jac, "full")
            b, sb = ph.pose_cov_reference(ref, jac, "schur")
            assert sa == sb == ph.OK, (t, sa, sb)
            g = ph.amplification(jac.J, ref.cov_full)
            tol = ch.bound(ref.kappa) * g
            e = ch.cov_metric(b, a)
            gs.append(g); tols.append(tol); errs.append(e)
            assert tol < 1e-4, (t, tol)
            assert e <= 2 * tol, (t, e, tol)
    print(f"{name}: g {min(gs):.3g} .. {max(gs):.3g}, bound {min(tols):.3g} .. {max(tols):.3g}, route difference <= {max(errs):.3g}")


def test_zero_and_inf_rules(cv, oracle, oracle_refs):
    import cov_helpers as ch
    import posecov_helpers as ph
    w, ref = oracle_refs["tiny"]
    assert w.K == 12 and ref.untouched[6 * 11:6 * 12].all()
    cov, st = ph.pose_cov_reference(ref, ph.pose_jacobian(w, ph.time_of(w, 8, 0.5)))       # depends on the untouched last knot
    assert st == ph.UNTOUCHED and np.isinf(np.diag(cov)).all() and not cov[~np.eye(6, dtype=bool)].any()
    cov, st = ph.pose_cov_reference(ref, ph.pose_jacobian(w, ph.time_of(w, 8, 0.0)))       # u = 0: it does not
    assert st == ph.OK and np.isfinite(cov).all() and (np.diag(cov) > 0).all()
    for t in (w.t0_ns - 1, w.t0_ns + (w.K - 3) * w.dt_ns):
        cov, st = ph.pose_cov_reference(ref, ph.pose_jacobian(w, t))
        assert st == ph.OUTSIDE and np.isnan(cov).all()
    wf = cv.synth.make_window("tiny", seed=7)
    wf.fixed_upto = 3
    wf.normalize()
    H, _, _ = oracle.OracleWindow(wf).build_normal()
    P = wf.P
    reff = ch.cov_reference(H[:P, :P], H[:P, P:], np.diag(H)[P:], ~ch.constant_mask(wf), range(P))
    cov, st = ph.pose_cov_reference(reff, ph.pose_jacobian(wf, ph.time_of(wf, 0, 0.0)))    # knots 0..2, all constant
    assert st == ph.OK and not cov.any()
    cov, st = ph.pose_cov_reference(reff, ph.pose_jacobian(wf, ph.time_of(wf, 1, 0.5)))    # knots 1..4: only knot 4 contributes
    assert st == ph.OK and (np.diag(cov) > 0).all()
