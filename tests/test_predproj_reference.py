"""CPU: the NumPy reference of ctvio_predict_landmarks (tests/predproj_helpers.py) against itself and against the helpers of the entries it
composes: the analytic [Jp | j] against central differences of its own value map, Phi and N against imuprop_helpers.propagate, the
covariance without the landmark's terms against A P_e A^T, one sample at row 0 against projection_helpers, the two covariance routes, the
status rules."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

WINDOWS = (("tiny", "tiny", 7), ("config1", "config1", 1000))


def samples(w, m, seed, t_start=None):
    from test_gpu_imu_predict import draw
    return draw(w, m, seed, t_start=t_start)


def half_turn(w, m=21, seed=8):
    """A draw whose gyro readings turn the body by pi about its y axis over the samples: the camera ends up looking away from the scene."""
    t, gyro, acc = samples(w, m, seed)
    gyro[:] = np.array([0.0, np.pi / ((int(t[-1]) - int(t[0])) * 1e-9), 0.0])
    return t, gyro, acc


def with_ld_ns(w, n):
    from test_projection_reference import with_ld_ns as f
    return f(w, n)


@pytest.mark.parametrize("name,cfg,seed", WINDOWS, ids=[x[0] for x in WINDOWS])
def test_jacobian_against_central_differences(cv, name, cfg, seed):
    """[Jp | j] against central differences of predict() under np_oracle.retract, over every unknown the value depends on: the knots of the
    anchor time and of the start time, the six biases of the chosen state, rho, h = 1e-6 and the flat 1e-8 relative to max(1, largest entry)
    of tests/test_projection_reference.py; the line delay over +-1000 ns with that test's five-point truncation bound.  The propagation part
    alone, A Phi against central differences over the start state's tangent: 1e-9 max(1, |A Phi|), as tests/test_imuprop_reference.py."""
    import imuprop_helpers as ih
    import np_oracle
    import predproj_helpers as pp
    w = cv.synth.make_window(cfg, seed=seed)
    if w.ld == 0.0:
        w.ld = 2.0e-5                      # the read-out is not degenerate
    t, gyro, acc = samples(w, 21, 5)
    frame = w.F - 1
    h = 1e-6
    ld_ns = int(np.int64(w.ld * 1e9))
    worst = [0.0, 0.0, 0.0]
    for l, row in ((0, 0), (w.L // 2, 240), (w.L - 1, 479)):
        pj = pp.prediction_jacobian(w, l, frame, t, gyro, acc, row)
        assert pj is not None
        f = lambda x: pp.predict(x, l, frame, t, gyro, acc, row)[0][:2]
        cols = sorted({6 * k + c for k in list(pj.knots_a) + list(pj.knots_q) for c in range(6)} | {6 * w.K + 6 * frame + c for c in range(6)} | {w.P + l})
        scale = max(1.0, float(np.abs(pj.J).max()))
        for u in cols:
            xi = np.zeros(w.N); xi[u] = h
            fd = (f(np_oracle.retract(w, xi)) - f(np_oracle.retract(w, -xi))) / (2 * h)
            e = float(np.abs(fd - pj.J[:, u]).max() / scale)
            worst[0] = max(worst[0], e)
            assert e <= 1e-8, (l, row, u, e)
        # ---- every other column is zero, the line delay apart
        rest = np.ones(w.P + w.L, bool); rest[cols] = False; rest[w.P - 1] = False
        assert not pj.J[:, rest].any()
        # ---- line delay
        fl = {k: pp.predict(with_ld_ns(w, ld_ns + 1000 * k), l, frame, t, gyro, acc, row)[0][:2] for k in (-2, -1, 1, 2)}
        col = pj.Jp[:, w.P - 1]
        x3 = np.abs(fl[2] - 2 * fl[1] + 2 * fl[-1] - fl[-2]) / 2.0 / h ** 3
        tol = 2 * h ** 2 / 6 * float(x3.max()) + 1e-8 * max(1.0, float(np.abs(col).max()))
        e = float(np.abs((fl[1] - fl[-1]) / (2 * h) - col).max())
        worst[1] = max(worst[1], e / tol)
        assert e <= tol, (l, row, e, tol)
        # ---- the propagation part: d(proj) / d(start state)
        x0 = pp.start_state(w, int(t[0]), frame)
        M = pj.A @ pj.Phi

        def g(d):
            xs, _ = ih.propagate(ih.boxplus(x0, d), None, t, gyro, acc, w.gravity, cov=False)
            return pp.predict_from(w, l, xs[-1], gyro[-1] - xs[-1][3], row)[0][:2]
        for k in range(15):
            d = np.zeros(15); d[k] = h
            e = float(np.abs((g(d) - g(-d)) / (2 * h) - M[:, k]).max())
            worst[2] = max(worst[2], e / max(1.0, np.abs(M).max()))
            assert e <= 1e-9 * max(1.0, np.abs(M).max()), (l, row, k, e)
    print(f"{name}: knots, biases, rho {worst[0]:.3g} (relative), line delay {worst[1]:.3g} of its bound, A Phi {worst[2]:.3g}")


def test_transition_reproduces_the_recurrence(cv):
    """Phi P0 Phi^T + N equals imuprop_helpers.propagate's last P for a random P0, within 64 max(d, 15 m 2^-53), d the float64-vs-longdouble
    difference that helper measures on the same inputs; the end state is propagate's to the bit."""
    import imuprop_helpers as ih
    import predproj_helpers as pp
    w = cv.synth.make_window("tiny", seed=7)
    rng = np.random.default_rng(3)
    for m in (1, 2, 21):
        t, gyro, acc = samples(w, m, 20 + m)
        x0 = pp.start_state(w, int(t[0]), None)
        A = rng.normal(0, 1e-2, (15, 15))
        P0 = A @ A.T
        xe, Phi, N = pp.transition(x0, t, gyro, acc, w.gravity)
        xs, Ps = ih.propagate(x0, P0, t, gyro, acc, w.gravity)
        _, Pl = ih.propagate(x0, P0, t, gyro, acc, w.gravity, dtype=np.longdouble)
        assert all(np.array_equal(a, b) for a, b in zip(xe, xs[-1]))
        d = ih.entry_metric(Ps[-1], Pl[-1])
        e = ih.entry_metric(Phi @ P0 @ Phi.T + N, Pl[-1])
        print(f"m {m}: float64 vs longdouble {d:.3g}, Phi P0 Phi^T + N {e:.3g}")
        assert e <= 64 * max(d, 15 * m * 2.0 ** -53), (m, e, d)
        if m == 1:
            assert np.array_equal(Phi, np.eye(15)) and not N.any()


@pytest.fixture(scope="module")
def oracle_refs(cv, oracle, golden_dir):
    from test_projection_reference import oracle_reference
    out = {}
    for name, cfg, seed in WINDOWS:
        fx = np.load(os.path.join(golden_dir, f"cov_{cfg}_seed{seed}.npz"))
        w = cv.synth.make_window(cfg, seed=seed)
        w.quat[:] = fx["quat"]; w.pos[:] = fx["pos"]; w.bias[:] = fx["bias"]; w.rho[:] = fx["rho"]; w.ld = float(fx["ld"])
        out[name] = (w, oracle_reference(oracle, w))
    return out


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_ties_to_imu_predict_and_the_two_routes_agree(oracle_refs, name):
    """With the landmark's terms removed (anchor block, read-out column and j zero) the covariance is A P_e A^T with P_e the covariance
    ctvio_imu_predict reports: imuprop_helpers.propagate from P0 = J_nav Sigma J_nav^T.  The full and the Schur route agree within twice the
    state part of the GPU bound."""
    import cov_helpers as ch
    import imuprop_helpers as ih
    import posecov_helpers as ph
    import predproj_helpers as pp
    w, ref = oracle_refs[name]
    t, gyro, acc = samples(w, 21, 9)
    n_ok = 0
    for l in range(0, w.L, max(1, w.L // 6)):
        pj = pp.prediction_jacobian(w, l, None, t, gyro, acc, 240)
        a, sa = pp.pred_cov_reference(ref, pj, l, w.K, "full")
        b, sb = pp.pred_cov_reference(ref, pj, l, w.K, "schur")
        assert sa == sb
        if sa != pp.OK:
            continue
        n_ok += 1
        g = ph.amplification(pp.kept_jacobian(ref, pj, l), ref.Sig)
        tol = ch.bound(ref.kappa) * g
        assert tol < 1e-2 and ch.cov_metric(b, a) <= 2 * tol, (l, ch.cov_metric(b, a), tol)
        assert (np.diag(a) > 0).all() and (np.diag(pj.ANA) > 0).all()
        Sig = ref.Sig[:ref.kp.shape[0], :ref.kp.shape[0]]
        Jn = pj.nav.J[:, ref.kp]
        P0 = Jn @ Sig @ Jn.T
        _, Ps = ih.propagate(pp.start_state(w, int(t[0]), None), P0, t, gyro, acc, w.gravity)
        want = pj.A @ Ps[-1] @ pj.A.T
        Jq = pj.Jn[:, ref.kp]
        got = Jq @ Sig @ Jq.T + pj.ANA
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (l, got, want)
    assert n_ok >= 3


def test_one_sample_at_row_zero_is_the_projection(cv):
    """m = 1, row 0: the end state is the start state, delta = 0, Phi = I, N = 0: value and [Jp | j] are projection_helpers' at (imu_t[0], 0)."""
    import predproj_helpers as pp
    import projection_helpers as pr
    w = cv.synth.make_window("config1", seed=1000)
    t, gyro, acc = samples(w, 1, 4, t_start=int(w.t0_ns) + 7 * int(w.dt_ns) + 12_345_678)
    for l in range(0, w.L, 7):
        pj = pp.prediction_jacobian(w, l, None, t, gyro, acc, 0)
        qj = pr.projection_jacobian(w, l, int(t[0]), 0)
        assert pj is not None and qj is not None and not pj.ANA.any()
        assert np.allclose(pj.proj, qj.proj, rtol=1e-12, atol=1e-13)
        s = max(1.0, np.abs(qj.J).max())
        assert np.abs(pj.J - qj.J).max() <= 1e-11 * s, (l, np.abs(pj.J - qj.J).max())
        assert not pj.J[:, 6 * w.K:w.P - 1].any()          # no bias dependence without a step and a read-out


def test_status_rules(cv, oracle_refs):
    """A start time outside the spline, rho <= 0 and a point behind the camera: status 3; an untouched knot under the start time (the last
    segment at u = 0.5) and Hll == 0: status 2; otherwise 0."""
    import lmpoint_helpers as lh
    import posecov_helpers as ph
    import predproj_helpers as pp
    w0, ref = oracle_refs["tiny"]
    K = w0.K
    t, gyro, acc = samples(w0, 5, 2)
    assert pp.predict(w0, 0, None, t, gyro, acc, 0)[2] == pp.OK
    for ts in (int(w0.t0_ns) - 1, ph.time_of(w0, K - 3, 0.0)):
        to, go, ao = samples(w0, 5, 2, t_start=ts)
        p, r, st = pp.predict(w0, 0, None, to, go, ao, 0)
        assert st == pp.NONE and r == -1 and np.isnan(p).all() and pp.prediction_jacobian(w0, 0, None, to, go, ao, 0) is None
    w = w0.copy(); w.rho[2] = -1.0
    assert pp.predict(w, 2, None, t, gyro, acc, 0)[2] == pp.NONE and pp.predict(w, 3, None, t, gyro, acc, 0)[2] == pp.OK
    c, sc = pp.pred_cov_reference(ref, None, 2, K)
    assert sc == pp.NONE and np.isnan(c).all()
    tb, gb, ab = half_turn(w0)                                     # the body turned half round: every landmark behind the camera
    assert all(pp.predict(w0, l, None, tb, gb, ab, 0)[2] == pp.NONE for l in range(w0.L))
    assert (np.diag(ref.Hpp)[6 * (K - 1):6 * K] == 0).all(), "the padding knot of `tiny` is touched"
    for u, want in ((0.5, pp.NO_INFO), (0.0, pp.OK)):
        tu, gu, au = samples(w0, 3, 6, t_start=ph.time_of(w0, K - 4, u))
        pj = pp.prediction_jacobian(w0, 0, None, tu, gu, au, 0)
        assert pj is not None and (K - 1 in pj.knots_q) == (u > 0)
        for route in ("full", "schur"):
            c, sc = pp.pred_cov_reference(ref, pj, 0, K, route)
            assert sc == want, (u, sc)
            if want == pp.NO_INFO:
                assert np.isposinf(np.diag(c)).all() and c[0, 1] == 0 and c[1, 0] == 0
    ref0 = lh.joint_reference(ref.Hpp, ref.W, np.where(np.arange(ref.L) == 1, 0.0, ref.Hll), np.ones(ref.P))
    c, sc = pp.pred_cov_reference(ref0, pp.prediction_jacobian(w0, 1, None, t, gyro, acc, 0), 1, K)
    assert sc == pp.NO_INFO and np.isposinf(np.diag(c)).all()
