"""CPU: the NumPy reference of the leave-one-out IMU gate (tests/imugate_helpers.py) on the oracle's normal matrix.  The quantities of the
formulation's table; C_loo = (I - A)^-1 - I against the brute-force route -- H minus the sample's own J^T J, inverted -- and r_loo against
the Gauss-Newton step of the downdated system; the tolerance hat_bound itself; statuses, locked biases, constants, samples at u = 0."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

EPS = 2.0 ** -53
# smallest / largest redundancy at the covariance fixtures' states: over the samples the formulation was checked on (every sample of `tiny`,
# every 5th of `config1`), and re-measured here over ALL samples (the last sample of `config1`, which no 5th sample is, has the smallest)
TABLE = {"tiny": (1, 0.4795, 0.8972), "config1": (5, 0.7734, 0.9589)}
TABLE_ALL = {"tiny": (0.4795, 0.8972), "config1": (0.7585, 0.9602)}


def oracle_reference(oracle, w):
    from test_projection_reference import oracle_reference as o
    return o(oracle, w)


def fixture_window(cv, golden_dir, cfg, seed):
    fx = np.load(os.path.join(golden_dir, f"cov_{cfg}_seed{seed}.npz"))
    w = cv.synth.make_window(cfg, seed=seed)
    w.quat[:] = fx["quat"]; w.pos[:] = fx["pos"]; w.bias[:] = fx["bias"]; w.rho[:] = fx["rho"]; w.ld = float(fx["ld"])
    return w


@pytest.fixture(scope="module")
def refs(cv, oracle, golden_dir):
    """name -> (window at the covariance fixture's state, the joint reference on the oracle's H, the per-sample references); computed once."""
    import imugate_helpers as ig
    out = {}
    for name, cfg, seed in (("tiny", "tiny", 7), ("config1", "config1", 1000)):
        w = fixture_window(cv, golden_dir, cfg, seed)
        ref = oracle_reference(oracle, w)
        out[name] = (w, ref, [ig.sample_reference(w, ref, m) for m in range(w.M)])
    return out


@pytest.fixture(scope="module")
def long_window(cv, oracle):
    """`config1` seed 1400 with F 16, L 60, M 750 (K 34) after the oracle's solve(4), and its joint reference."""
    w = cv.synth.make_window("config1", seed=1400, F=16, L=60, M=750)
    oracle.OracleWindow(w).solve(4)
    return w, oracle_reference(oracle, w)


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_formulation_table(refs, name):
    """I - A positive definite for every sample, the redundancies of TABLE (on its samples) and TABLE_ALL within 1e-3; on `config1` (converged) the mean deleted chi2 over
    all samples is 6 within (0.8, 1.25) and the post-fit form r^T (I - A) r -- what ctvio_visual_gate's chi2 would read with S = I -- lies
    below it."""
    import imugate_helpers as ig
    w, ref, R = refs[name]
    assert w.M == (80 if name == "tiny" else 500)
    assert all(b.status == ig.OK for b in R)
    red = np.array([b.redundancy for b in R])
    chi = np.array([b.chi2 for b in R])
    post = np.array([b.res @ (np.eye(6) - b.A) @ b.res for b in R])
    print(f"{name}: kappa_s {ref.kappa:.3g}, redundancy in [{red.min():.4f}, {red.max():.4f}], mean deleted chi2 {chi.mean():.4g}, post-fit form {post.mean():.4g}")
    assert red.min() > 0
    step, lo, hi = TABLE[name]
    assert abs(red[::step].min() - lo) < 1e-3 and abs(red[::step].max() - hi) < 1e-3, (red[::step].min(), red[::step].max())
    lo, hi = TABLE_ALL[name]
    assert abs(red.min() - lo) < 1e-3 and abs(red.max() - hi) < 1e-3, (red.min(), red.max())
    assert post.mean() < chi.mean()
    if name == "config1":
        assert 0.8 < chi.mean() / 6 < 1.25, chi.mean()


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_woodbury_against_the_downdated_system(refs, name):
    """Every sample of `tiny`, every tenth of `config1`: (I - A)^-1 - I = J (H - J^T J)^-1 J^T in imugate_helpers.cov_error within the sum of
    the two routes' bounds: (hat_bound + 64 * 2^-53) / redundancy for the Woodbury route, cov_helpers.bound(kappa of the downdated system)
    |C|_2 / |C + I|_2 for the other."""
    import cov_helpers as ch
    import imugate_helpers as ig
    w, ref, R = refs[name]
    worst, worst_cm = 0.0, 0.0
    for b in (R if name == "tiny" else R[::10]):
        C, tol_bf, kappa, _ = ig.brute_force(w, ref, b)
        assert np.isfinite(kappa)
        tol = (b.tol + ig.STEP) / b.redundancy + tol_bf * float(np.linalg.norm(C, 2) / np.linalg.norm(C + np.eye(6), 2))
        e = ig.cov_error(b.cov, C)
        assert tol < 1e-3 and e <= tol, (name, b.m, e, tol, b.redundancy)
        worst, worst_cm = max(worst, e / tol), max(worst_cm, ch.cov_metric(b.cov, C))
    print(f"{name}: Woodbury against the downdated inverse: worst {worst:.3g} of the bound, cov_metric {worst_cm:.3g}")


def test_r_loo_is_the_gauss_newton_step_without_the_sample(cv, oracle):
    """`config1` seed 1003 after the oracle's solve(15) (g = 0 up to the solve's tolerance): with the sample taken out of H and g, the
    Gauss-Newton step delta = -(H - J^T J)^-1 (g - J^T r) moves the sample's residual to r + J delta = (I + C_loo) r - J (H - J^T J)^-1 g."""
    import imugate_helpers as ig
    w = cv.synth.make_window("config1", seed=1003)
    ow = oracle.OracleWindow(w)
    ow.solve(15)
    ref = oracle_reference(oracle, w)
    _, g, _ = ow.build_normal()
    gk = np.concatenate([g[:w.P][ref.kp], g[w.P:][ref.kl]])
    chi = []
    for m in range(0, w.M, 25):
        b = ig.sample_reference(w, ref, m)
        assert b.status == ig.OK
        C, tol_bf, _, Sig = ig.brute_force(w, ref, b)
        delta = -Sig @ (gk - b.J.T @ b.res)
        r_gn = b.res + b.J @ delta
        r_loo = (np.eye(6) + b.cov) @ b.res
        rest = b.J @ (Sig @ gk)
        tol = ((b.tol + ig.STEP) / b.redundancy ** 2 + tol_bf * float(np.linalg.norm(C, 2))) * float(np.linalg.norm(b.res)) + 64 * EPS * float(np.abs(r_gn).max())
        assert np.abs(r_gn - (r_loo - rest)).max() <= tol, (m, np.abs(r_gn - (r_loo - rest)).max(), tol)
        assert np.linalg.norm(rest) <= 1e-3 * np.linalg.norm(b.res), (m, rest)       # (the state is a minimum: g plays no part)
        assert abs(b.chi2 - r_loo @ np.linalg.solve(b.cov + np.eye(6), r_loo)) <= 1e-9 * b.chi2
        chi.append(b.chi2)
    print(f"config1 seed 1003 after solve(15): mean deleted chi2 over {len(chi)} samples {np.mean(chi):.3g}")


def test_the_tolerance_itself(refs, long_window):
    """hat_bound = cov_helpers.bound(kappa_s) |A|_2 (norm-wise, no row amplification: see imugate_helpers).  Two NumPy routes to A -- the
    joint Jacobi-scaled inverse and the Cholesky factor of the reduced system -- agree within it; a 1e-11 relative perturbation of J -- the
    agreement tests/test_ratesjac_host.py holds the device Jacobian to -- moves A by less than 1e-2 of it; it is below 1e-4 on every tested
    window."""
    import imugate_helpers as ig
    rng = np.random.default_rng(11)
    lw, lref = long_window
    assert lw.K == 34
    cases = [(n, refs[n][0], refs[n][1], refs[n][2][::(1 if n == "tiny" else 10)]) for n in ("tiny", "config1")]
    cases.append(("long k34", lw, lref, [ig.sample_reference(lw, lref, m) for m in range(0, lw.M, 10)]))
    for name, w, ref, R in cases:
        worst_routes, worst_pert, worst_tol = 0.0, 0.0, 0.0
        for b in R:
            assert b.status == ig.OK and 0 < b.tol < 1e-4, (name, b.m, b.tol)
            Jp = b.J[:, :ref.kp.shape[0]]
            Y = np.linalg.solve(ref.Lc, Jp.T)
            e = float(np.linalg.norm(Y.T @ Y - b.A, 2))
            assert e <= b.tol, (name, b.m, e, b.tol)
            Jn = b.J * (1.0 + 1e-11 * rng.uniform(-1, 1, b.J.shape))
            d = float(np.linalg.norm(Jn @ ref.Sig @ Jn.T - b.J @ ref.Sig @ b.J.T, 2))
            assert d <= 1e-2 * b.tol, (name, b.m, d, b.tol)
            worst_routes, worst_pert, worst_tol = max(worst_routes, e / b.tol), max(worst_pert, d / b.tol), max(worst_tol, b.tol)
        print(f"{name}: hat_bound <= {worst_tol:.3g}; the two routes differ by {worst_routes:.3g} of it, a 1e-11 perturbation of J moves A by {worst_pert:.3g} of it")


def test_statuses(cv, oracle, refs):
    """A sample given a bias state of its own (F + 1 states, no bias-chain link): nothing else predicts it, the reference redundancy is zero
    up to rounding -- below min_redundancy / 10 -- and the status 4; its neighbours keep theirs.  Locked biases: the bias rows contribute
    nothing.  Every unknown constant: A = 0, redundancy 1, a zero C_loo, chi2 = |r|^2.  Samples at u = 0 (`tiny` has eight): knot s + 3
    does not enter.  Zero IMU weights with an otherwise untouched bias state: status 2."""
    import imugate_helpers as ig
    w0, _, R0 = refs["tiny"]
    m = w0.M // 2
    w = w0.copy()
    w.bias = np.vstack([w.bias, w.bias[w.imu_bias[m]]])
    w.imu_bias[m] = w0.F
    assert w.F == w0.F + 1
    ref = oracle_reference(oracle, w)
    R = [ig.sample_reference(w, ref, k) for k in range(m - 2, m + 3)]
    b = R[2]
    print(f"a bias state of its own: redundancy {b.redundancy:.3g}; neighbours {R[1].redundancy:.3g}, {R[3].redundancy:.3g}")
    assert b.status == ig.WEAK and b.redundancy < 0.01 / 10 and np.isposinf(np.diag(b.cov)).all() and b.chi2 == 0.0
    assert all(x.status == ig.OK and x.redundancy > 0.4 for x in R[:2] + R[3:])
    fs = ig.frame_reference(w, R)
    assert fs[w0.F].tolist()[0] == 0 and np.isnan(fs[w0.F, 1]) and fs[w0.F, 2] == 0.0 and fs[w0.F, 3] == b.redundancy
    # locked biases
    w = w0.copy(); w.lock_bg = True; w.lock_ba = True
    ref = oracle_reference(oracle, w)
    for k in range(0, w.M, 9):
        b = ig.sample_reference(w, ref, k)
        assert b.status == ig.OK and b.redundancy >= R0[k].redundancy - 1e-12      # (fewer unknowns: the rest predicts better)
    # every unknown constant
    w = w0.copy(); w.lock_bg = True; w.lock_ba = True; w.fix_ld = True; w.fixed_upto = w.K - 1
    ref = oracle_reference(oracle, w)
    assert ref.kp.shape[0] == 0
    b = ig.sample_reference(w, ref, 3)
    assert b.status == ig.OK and not b.A.any() and b.redundancy == 1.0 and not b.cov.any() and b.chi2 == pytest.approx(b.res @ b.res, rel=1e-15)
    # u = 0
    u0 = [k for k in range(w0.M) if (int(w0.imu_t[k]) - int(w0.t0_ns)) % int(w0.dt_ns) == 0]
    assert len(u0) == 8
    for k in u0:
        J6, jac = ig.sample_jacobian(w0, k)
        assert jac.u == 0.0 and len(jac.knots) == 3 and not J6[:, 6 * (jac.s + 3):6 * (jac.s + 4)].any() and R0[k].status == ig.OK
    # zero weights: the added bias state is touched by nothing
    w = w0.copy()
    w.bias = np.vstack([w.bias, w.bias[w.imu_bias[m]]])
    w.imu_bias[m] = w0.F
    w.imu_w = np.zeros(6)
    H = oracle.OracleWindow(w).build_normal()[0]      # (without IMU information the system is singular: the status needs the diagonal alone)
    assert not np.diag(H)[6 * w.K + 6 * w0.F:6 * w.K + 6 * w0.F + 6].any()
    b = ig.sample_reference(w, SimpleNamespace(Hpp=H[:w.P, :w.P]), m)
    assert b.status == ig.NO_INFO and b.redundancy == 0.0 and b.chi2 == 0.0 and np.isposinf(np.diag(b.cov)).all() and not b.res.any()
