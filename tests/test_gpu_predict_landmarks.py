"""GPU (-m gpu): ctvio_predict_landmarks_batch / ctvio_predict_landmarks (csrc/kernels_prop.hpp: k_imu_transition; csrc/kernels_cov.hpp:
k_cov_pred_jac, k_cov_solve tiles of kind TILE_PRED) against the NumPy reference of tests/predproj_helpers.py.  The joint covariance of (trajectory,
inverse depths) is formed from the DEVICE's own ctvio_linearize output of the same state (tests/test_gpu_landmark_points.device_reference, for
the reason given there).  Samples are drawn as tests/test_gpu_imu_predict.draw draws them: 200 Hz from the newest frame time, one 7 ms gap.

Per point, in this order: the status; proj3 at projection_helpers.value_atol; cov4 symmetric to the bit with a positive diagonal and
cov_metric <= cov_helpers.bound(kappa_s) g + 64 max(d, 15 m 2^-53) share -- g the amplification of [Jp | j] over the joint covariance, d the
float64-vs-longdouble difference of the helper's Phi and N, share the part of A N A^T in the block: the bounds of
tests/test_gpu_project_landmarks.py and tests/test_gpu_imu_predict.py, no new constant; chi2 against the extended-precision value from the
returned bits at 16 kappa_2 2^-53."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import query_harness as qh  # noqa: E402
from query_harness import device_joint_reference as device_reference  # noqa: E402,F401

EPS = 2.0 ** -53
ROW_MODEL = (460.0, 240.0, 480, 3)
FIELDS = ("state", "proj", "cov", "chi2", "row", "status")


def draw(w, m, seed, t_start=None):
    from test_gpu_imu_predict import draw as d
    return d(w, m, seed, t_start=t_start)


def cat(preds):
    """The concatenated samples of a list of predictions (frame, t, gyro, acc)."""
    return tuple(np.concatenate([p[k] for p in preds]) for k in (1, 2, 3))


def references(w, ref, preds, pts, row_model=None, noise=None):
    """Per point (prediction index, landmark, row): the helper's value, final row and value status, the Jacobian, the reference covariance, its
    status and bound.  preds: (frame, t, gyro, acc) per prediction."""
    import imuprop_helpers as ih
    import predproj_helpers as pp
    nz = ih.DEFAULT_NOISE if noise is None else noise
    ends, ds = [], []
    for frame, t, gyro, acc in preds:
        ends.append(pp.end_of(w, frame, t, gyro, acc))
        x0 = pp.start_state(w, int(t[0]), frame)
        ds.append(pp.recurrence_d((x0, t, gyro, acc, w.gravity, nz)) if x0 is not None and len(t) > 1 else 0.0)
    out = []
    for k, l, row in pts:
        frame, t, gyro, acc = preds[k]
        proj, r, sv = pp.predict_from(w, l, ends[k][0], ends[k][1], row, row_model)
        pj = pp.prediction_jacobian(w, l, frame, t, gyro, acc, r, nz) if sv == pp.OK else None
        c, sc = pp.pred_cov_reference(ref, pj, l, w.K)
        tol, g, share = pp.bound(ref, pj, l, ds[k], len(t)) if sc == pp.OK else (0.0, 0.0, 0.0)
        out.append(SimpleNamespace(k=k, l=l, proj=proj, row=r, sv=sv, pj=pj, cov=c, sc=sc, tol=tol, g=g, share=share))
    return out


def gate_points(R):
    return np.array([(r.proj[:2] + 2e-3 * np.array([np.cos(i), np.sin(i)])) if r.sv == 0 else np.zeros(2) for i, r in enumerate(R)])


def check(w, R, out, what, idx=None, obs=None):
    """out (Solver.predict_landmarks) against the references R[idx]; returns the worst (error / bound, bound, g, share)."""
    import cov_helpers as ch
    import projection_helpers as pr
    idx = list(range(len(R))) if idx is None else list(idx)
    n = len(idx)
    assert out.proj.shape == (n, 3) and out.status.shape == (n,) and out.row.shape == (n,)
    assert out.cov is None or out.cov.shape == (n, 2, 2)
    worst = (0.0, 0.0, 0.0, 0.0)
    for i, k in enumerate(idx):
        r = R[k]
        want = r.sc if out.cov is not None else r.sv
        assert out.status[i] == want, (what, k, out.status[i], want)                                         # 1. the status
        if want == pr.NONE:
            assert np.isnan(out.proj[i]).all() and out.row[i] == -1, (what, k)
            assert out.cov is None or np.isnan(out.cov[i]).all(), (what, k)
            assert out.chi2 is None or np.isnan(out.chi2[i]), (what, k)
            continue
        txy, tz = pr.value_atol(w, r.proj)                                                                  # 2. the value
        assert out.row[i] == r.row, (what, k, out.row[i], r.row)
        assert (np.abs(out.proj[i, :2] - r.proj[:2]) <= txy).all(), (what, k, out.proj[i], r.proj, txy)
        assert abs(out.proj[i, 2] - r.proj[2]) <= 1e-12 * abs(r.proj[2]) + tz, (what, k, out.proj[i], r.proj)
        if out.cov is None:
            continue
        c = out.cov[i]
        if want == pr.NO_INFO:
            assert np.isposinf(np.diag(c)).all() and c[0, 1] == 0 and c[1, 0] == 0, (what, k)
            assert out.chi2 is None or out.chi2[i] == 0.0, (what, k)
            continue
        assert np.isfinite(c).all() and c[0, 1] == c[1, 0] and (np.diag(c) > 0).all(), (what, k, c)         # 3. the covariance
        e = ch.cov_metric(c, r.cov)
        if e > 0.5 * r.tol:
            print(f"  {what} point {k}: error {e:.3g}, bound {r.tol:.3g}, g {r.g:.3g}, share {r.share:.3g}")
        worst = max(worst, (e / r.tol, r.tol, r.g, r.share))
        assert e <= r.tol, (what, k, e, r.tol)
        if out.chi2 is not None:                                                                            # 4. the gate
            val, k2 = pr.chi2_reference(out.proj[i], c, obs[i], w.img_w)
            assert abs(out.chi2[i] - val) <= 16 * k2 * EPS * val, (what, k, out.chi2[i], val, k2)
    print(f"{what}: {n} points, worst error {worst[0]:.3g} of its bound {worst[1]:.3g} (g {worst[2]:.3g}, noise share {worst[3]:.3g})")
    return worst


def cols(pts):
    a = np.array(pts, np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32)


def take(out, idx):
    return SimpleNamespace(state=out.state, proj=out.proj[idx], cov=None if out.cov is None else out.cov[idx],
                           chi2=None if out.chi2 is None else out.chi2[idx], row=out.row[idx], status=out.status[idx])


def same(a, b, fields=FIELDS):
    return qh.same_bits(a, b, fields)


def batch_call(s, win, preds, pts, **kw):
    """preds with frame None throughout: frame == NULL; otherwise every frame is given."""
    pi, l, row = cols(pts)
    fr = [p[0] for p in preds]
    return s.predict_landmarks_batch(win, None if all(f is None for f in fr) else fr, [len(p[1]) for p in preds], *cat(preds), pi, l, row, **kw)


def test_tiny_initial_state(cv):
    """Case 1: `tiny` seed 7 at the initial state (P = 103, L = 12): predictions of 1, 2 and 21 samples with bias states 0, F // 2 and the
    newest, every landmark under each; then calls of 1, 8, 9 and 17 points -- one tile, a full tile, a full tile plus one, a third tile with a
    tail -- through both entries, with and without gate, values only.  state16 equals imu_predict(last_only) bit for bit."""
    w = cv.synth.make_window("tiny", seed=7)
    assert (w.P, w.L) == (103, 12)
    ms, frames = [1, 2, 21], [0, w.F // 2, w.F - 1]
    preds = [(f,) + draw(w, m, 70 + i) for i, (m, f) in enumerate(zip(ms, frames))]
    pts = [(k, l, (37 * l + 101 * k) % 480) for k in range(3) for l in range(w.L)]
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = device_reference(s, 0, w)
        R = references(w, ref, preds, pts)
        assert all(r.sv == 0 for r in R), [r.sv for r in R]
        obs = gate_points(R)
        out = batch_call(s, [0, 0, 0], preds, pts, obs=obs)
        check(w, R, out, "tiny, all", obs=obs)
        ls, _, lst = s.imu_predict_batch([0, 0, 0], frames, ms, *cat(preds), last_only=True, cov=False)
        assert not lst.any() and np.array_equal(out.state, ls)
        ls, _, _ = s.imu_predict_batch([0, 0, 0], frames, ms, *cat(preds), last_only=True)
        assert np.array_equal(out.state, ls)
        # ---- the single-window entry: prediction 2, 17 points (landmarks repeat, the rows differ)
        p2 = [(2, k % w.L, (53 * k + 7) % 480) for k in range(17)]
        R2 = references(w, ref, preds, p2)
        obs2 = gate_points(R2)
        f, t, gyro, acc = preds[2]
        for n, first in ((1, 3), (8, 0), (9, 8), (17, 0)):
            idx = range(first, first + n)
            q = [p2[k] for k in idx]
            _, l, row = cols(q)
            a = s.predict_landmarks(0, None, t, gyro, acc, l, row, obs=obs2[first:first + n])
            check(w, R2, a, f"tiny, {n} points, single entry", idx, obs2[first:first + n])
            b = batch_call(s, [0, 0, 0], preds, q)
            check(w, R2, b, f"tiny, {n} points, batch entry, no gate", idx)
            v = s.predict_landmarks(0, w.F - 1, t, gyro, acc, l, row, cov=False)
            check(w, R2, v, f"tiny, {n} points, values only", idx)
            assert np.array_equal(a.state[0], out.state[2]) and np.array_equal(v.state[0], out.state[2]) and np.array_equal(b.state, out.state)
            assert np.array_equal(a.proj, b.proj) and np.array_equal(a.proj, v.proj) and np.array_equal(a.row, v.row)


@pytest.fixture(scope="module")
def config1_solved(cv):
    """`config1` seed 1000 after a 15-iteration solve on an open handle: (solver, the window at the solved state, the device reference, one
    21-sample prediction from the newest frame time)."""
    for s, w in qh.solved_window(cv, "config1", 1000, 15):
        yield s, w, device_reference(s, 0, w), (None,) + draw(w, 21, 1000)


def test_config1_solved(config1_solved):
    """Case 2: solved `config1` (P = 211, L = 50, a free line delay != 0): the next frame -- every landmark at row 240 and at its iterated row."""
    s, w, ref, pred = config1_solved
    assert (w.P, w.L) == (211, 50) and w.ld != 0.0 and not w.fix_ld
    pts = [(0, l, 240) for l in range(w.L)]
    _, t, gyro, acc = pred
    for rm, what in ((None, "config1 solved, row 240"), (ROW_MODEL, "config1 solved, row model")):
        R = references(w, ref, [pred], pts, rm)
        assert all(r.sv == 0 for r in R)
        assert rm is None or sum(r.row != 240 for r in R) > w.L // 2
        obs = gate_points(R)
        _, l, row = cols(pts)
        out = s.predict_landmarks(0, None, t, gyro, acc, l, row, obs=obs, row_model=rm)
        check(w, R, out, what, obs=obs)
        vals = s.predict_landmarks(0, None, t, gyro, acc, l, row, cov=False, row_model=rm)
        check(w, R, vals, what + ", values only")
        assert np.array_equal(vals.proj, out.proj) and np.array_equal(vals.row, out.row) and np.array_equal(vals.state, out.state)


def test_one_sample_at_row_zero_is_project_landmarks(config1_solved):
    """Case 2, cross-check: m = 1, row 0 against ctvio_project_landmarks at the same time -- other code, so not to the bit: the values within
    the value tolerance, the covariances within the sum of both bounds."""
    import cov_helpers as ch
    import projection_helpers as pr
    from test_gpu_imu_predict import newest
    from test_gpu_project_landmarks import references as proj_refs
    s, w, ref, _ = config1_solved
    t, gyro, acc = draw(w, 1, 5)
    assert int(t[0]) == newest(w)
    pts = [(0, l, 0) for l in range(w.L)]
    R = references(w, ref, [(None, t, gyro, acc)], pts)
    Rp = proj_refs(w, ref, [(l, int(t[0]), 0) for l in range(w.L)])
    _, l, row = cols(pts)
    a = s.predict_landmarks(0, None, t, gyro, acc, l, row)
    b = s.project_landmarks(0, l, np.full(w.L, int(t[0]), np.int64), row)
    assert np.array_equal(a.status, b.status) and not a.status.any()
    worst = 0.0
    for i in range(w.L):
        txy, tz = pr.value_atol(w, b.proj[i])
        assert (np.abs(a.proj[i, :2] - b.proj[i, :2]) <= txy).all() and abs(a.proj[i, 2] - b.proj[i, 2]) <= 1e-12 * b.proj[i, 2] + tz
        e = ch.cov_metric(a.cov[i], b.cov[i])
        worst = max(worst, e / (R[i].tol + Rp[i].tol))
        assert e <= R[i].tol + Rp[i].tol, (i, e, R[i].tol, Rp[i].tol)
    print(f"m = 1, row 0 against project_landmarks: worst {worst:.3g} of the sum of both bounds")


def run_variant(cv, x, preds, pts, what, noise=None):
    with cv.Solver() as s:
        s.set_windows([x.copy()])
        R = references(x, device_reference(s, 0, x), preds, pts, noise=noise)
        obs = gate_points(R)
        vals = batch_call(s, [0] * len(preds), preds, pts, cov=False, noise=noise)
        full = batch_call(s, [0] * len(preds), preds, pts, obs=obs, noise=noise)
    check(x, R, vals, what + ", values only")
    check(x, R, full, what, obs=obs)
    assert np.array_equal(vals.proj, full.proj, equal_nan=True) and np.array_equal(vals.row, full.row) and np.array_equal(vals.state, full.state, equal_nan=True)
    return R, vals, full


def test_constants_and_statuses(cv):
    """Case 3 on `tiny`: fixed_upto, lock_bg / lock_ba and fix_ld variants (values unchanged to the bit); all sigmas zero gives the state part
    alone; a start time outside the spline, rho <= 0 and a point behind the camera give status 3; an untouched knot under the start time and
    Hll == 0 give status 2."""
    import posecov_helpers as ph
    import predproj_helpers as pp
    from test_predproj_reference import half_turn
    w = cv.synth.make_window("tiny", seed=7)
    K = w.K
    nf = w.F - 1
    preds = [(nf,) + draw(w, 21, 31), (1,) + draw(w, 5, 32, t_start=ph.time_of(w, K - 4, 0.5)), (nf,) + draw(w, 3, 33, t_start=ph.time_of(w, K - 3, 0.0)),
             (nf,) + draw(w, 3, 34, t_start=int(w.t0_ns) - 1), (nf,) + half_turn(w), (0,) + draw(w, 4, 35, t_start=ph.time_of(w, K - 4, 0.0))]
    pts = [(0, l, (37 * l) % 480) for l in range(w.L)] + [(k, l, 0) for k in range(1, 6) for l in (0, 5)]
    R0, v0, f0 = run_variant(cv, w, preds, pts, "tiny, free")
    st = {k: [r.sc for r in R0 if r.k == k] for k in range(6)}
    assert st[1] == [pp.NO_INFO] * 2 and st[2] == [pp.NONE] * 2 and st[3] == [pp.NONE] * 2 and st[4] == [pp.NONE] * 2 and st[0] == [0] * w.L
    assert np.isnan(f0.state[2]).all() and np.isnan(f0.state[3]).all() and np.isfinite(f0.state[[0, 1, 4, 5]]).all()
    mine = np.array([p[0] == 1 for p in pts])
    assert (f0.status[mine] == 2).all() and (v0.status[mine] == 0).all()
    wr = w.copy(); wr.rho[2] = -1.0
    _, v1, f1 = run_variant(cv, wr, preds, pts, "tiny, rho = -1 on landmark 2")
    bad = np.array([p[1] == 2 for p in pts])
    assert (v1.status[bad] == 3).all() and (f1.status[bad] == 3).all() and np.isnan(f1.cov[bad]).all()
    assert np.array_equal(v1.proj[~bad], v0.proj[~bad], equal_nan=True)
    for what, mod in (("fixed_upto = 3", dict(fixed_upto=3)), ("lock_bg, lock_ba", dict(lock_bg=1, lock_ba=1)), ("fix_ld", dict(fix_ld=True))):
        x = w.copy()
        for a, b in mod.items():
            setattr(x, a, b)
        x.normalize()
        _, v, f = run_variant(cv, x, preds, pts, "tiny, " + what)
        assert np.array_equal(v.proj, v0.proj, equal_nan=True) and np.array_equal(v.state, v0.state, equal_nan=True)
    # ---- all sigmas zero: N = 0, the state part alone -- smaller than with noise, by A N A^T to rounding
    Rz, _, fz = run_variant(cv, w, preds, pts, "tiny, zero sigmas", noise=(0.0, 0.0, 0.0, 0.0))
    for i in range(w.L):
        assert not Rz[i].pj.ANA.any() and Rz[i].share == 0.0
        d = f0.cov[i] - fz.cov[i]
        assert np.abs(d - R0[i].pj.ANA).max() <= (R0[i].tol + Rz[i].tol) * np.abs(np.diag(f0.cov[i])).max()


def test_no_landmark_information(cv):
    """Case 3, Hll == 0: with img_w = 0 the visual blocks weigh nothing, every Hll is zero and every computable point has status 2: the value
    is the free window's to the bit, +inf on the diagonal, 0 elsewhere."""
    w = cv.synth.make_window("tiny", seed=7)
    f, t, gyro, acc = (None,) + draw(w, 5, 36)
    l, row = np.arange(w.L, dtype=np.int32), np.zeros(w.L, np.int32)
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        v0 = s.predict_landmarks(0, f, t, gyro, acc, l, row, cov=False)
    wz = w.copy(); wz.img_w = 0.0
    with cv.Solver() as s:
        s.set_windows([wz])
        assert not s.linearize(0)[2].any()
        o = s.predict_landmarks(0, f, t, gyro, acc, l, row)
    assert not v0.status.any() and (o.status == 2).all() and np.array_equal(o.proj, v0.proj)
    assert np.isposinf(o.cov[:, 0, 0]).all() and np.isposinf(o.cov[:, 1, 1]).all() and not o.cov[:, 0, 1].any() and not o.cov[:, 1, 0].any()


def mixed_setup(cv):
    """The four windows of test_gpu_covariance's mixed batch: one prediction per window from its newest frame time (1, 5, 21, 21 samples),
    every landmark of the three windows with landmarks under its window's prediction and every third also at another row, interleaved."""
    from test_gpu_covariance import mixed_batch
    ws, _ = mixed_batch(cv)
    ms = [21, 5, 21, 1]
    preds = [([0, w.F - 1, w.F // 2, w.F - 1][i],) + draw(w, ms[i], 600 + i) for i, w in enumerate(ws)]
    pts = []
    for i, w in enumerate(ws):
        pts += [(i, l, (53 * l + 7) % 480) for l in range(w.L)] + [(i, l, 11 * l % 480) for l in range(0, w.L, 3)]
    order = np.random.default_rng(5).permutation(len(pts))
    return ws, list(range(len(ws))), preds, [pts[k] for k in order]


@pytest.fixture(scope="module")
def mixed(cv):
    from test_gpu_covariance import DET
    ws, win, preds, pts = mixed_setup(cv)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        refs = [device_reference(s, i, w) if w.L else None for i, w in enumerate(ws)]
        R = [None] * len(pts)
        for i, w in enumerate(ws):
            idx = [k for k, p in enumerate(pts) if p[0] == i]
            for k, r in zip(idx, references(w, refs[i], [preds[i]], [(0, pts[k][1], pts[k][2]) for k in idx]) if idx else []):
                R[k] = r
        obs = gate_points(R)
        out = batch_call(s, win, preds, pts, obs=obs)
    return ws, win, preds, pts, R, obs, out


def test_mixed_batch_against_reference(mixed):
    """Case 4: one call over the mixed batch (`tiny`, `config1`, the K = 34 / P = 301 window, an IMU-only window), the points of three windows
    interleaved; the IMU-only window has a prediction and no point."""
    ws, win, preds, pts, R, obs, out = mixed
    assert ws[3].L == 0 and not any(p[0] == 3 for p in pts) and np.isfinite(out.state).all()
    for i, w in enumerate(ws):
        idx = np.array([k for k, p in enumerate(pts) if p[0] == i], int)
        if idx.shape[0]:
            check(w, R, take(out, idx), f"mixed window {i} (P {w.P}, L {w.L})", idx, obs[idx])


def test_mixed_batch_bits(cv, mixed, monkeypatch):
    """Case 4, bitwise under the order-fixed linearisation: a second call; the single-window entry per window; points and predictions
    permuted; values only against the covariance call; a call without the gate; CTVIO_POISON=1."""
    from test_gpu_covariance import DET
    ws, win, preds, pts, R, obs, out = mixed
    n = len(pts)
    pf = ("proj", "cov", "chi2", "row", "status")

    def run(s):
        assert same(batch_call(s, win, preds, pts, obs=obs), out)
        for i, w in enumerate(ws):
            idx = np.array([k for k, p in enumerate(pts) if p[0] == i], int)
            if idx.shape[0]:
                f, t, gyro, acc = preds[i]
                _, l, row = cols([pts[k] for k in idx])
                o = s.predict_landmarks(i, f, t, gyro, acc, l, row, obs=obs[idx])
                assert same(o, take(out, idx), pf) and np.array_equal(o.state[0], out.state[i]), i
        sh = np.random.default_rng(9).permutation(n)
        pp_ = [3, 1, 0, 2]                                     # the caller's order of the predictions
        inv = {old: new for new, old in enumerate(pp_)}
        o = batch_call(s, [win[k] for k in pp_], [preds[k] for k in pp_], [(inv[pts[k][0]], pts[k][1], pts[k][2]) for k in sh], obs=obs[sh])
        assert same(o, take(out, sh), pf) and np.array_equal(o.state, out.state[pp_])
        v = batch_call(s, win, preds, pts, cov=False)
        assert np.array_equal(v.proj, out.proj, equal_nan=True) and np.array_equal(v.row, out.row) and np.array_equal(v.state, out.state)
        nog = batch_call(s, win, preds, pts)
        assert nog.chi2 is None and np.array_equal(nog.cov, out.cov, equal_nan=True) and np.array_equal(nog.proj, out.proj, equal_nan=True)
        half = np.arange(0, n, 2)
        assert same(batch_call(s, win, preds, [pts[k] for k in half], obs=obs[half]), take(out, half), pf)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        run(s)
    monkeypatch.setenv("CTVIO_POISON", "1")
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        run(s)


def test_leaves_the_solve_alone(cv, mixed):
    """Case 5: state bits, graph captures and a following solve are unchanged by the calls; the timing slots of both calls."""
    ws, win, preds, pts, R, obs, out = mixed

    def calls(s, b):
        o1 = batch_call(s, win, preds, pts, obs=obs)
        assert np.isfinite(o1.cov[o1.status == 0]).all() and np.isfinite(o1.proj[o1.status != 3]).all()
        ms, launches = s.last_timing()
        assert launches[:4].tolist() == [1, 1, 1, 1] and ms[7] >= ms[1] > 0 and ms[2] > 0 and ms[3] > 0
        o2 = batch_call(s, win, preds, pts, cov=False)
        ms, launches = s.last_timing()
        assert launches[:4].tolist() == [0, 0, 1, 1] and ms[7] >= ms[2] > 0 and ms[3] > 0
        assert np.array_equal(o2.proj, o1.proj, equal_nan=True) and np.array_equal(o2.row, o1.row) and np.array_equal(o2.state, o1.state)
    qh.check_leaves_the_solve_alone(cv, ws, calls)


def test_refusals_leave_the_handle_usable(cv):
    """Case 6: CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for every case of the header (a landmark index for the IMU-only window
    among them); empty calls are fine; the handle solves afterwards like a fresh one."""
    import ctypes as C
    from test_gpu_covariance import DET, mixed_batch
    p = cv.capi._p
    ws, _ = mixed_batch(cv)
    w = ws[0]
    assert ws[3].L == 0
    t, gyro, acc = draw(w, 4, 1)
    t3, gyro3, acc3 = draw(ws[3], 4, 2)
    tt, gg, aa = np.concatenate([t, t3]), np.concatenate([gyro, gyro3]), np.concatenate([acc, acc3])
    win = np.array([0, 3], np.int32); fr = np.array([0, 0], np.int32); m = np.array([4, 4], np.int32)
    pred = np.array([0, 0], np.int32); lm = np.array([0, 1], np.int32); row = np.array([0, 5], np.int32)
    obs = np.zeros((2, 2)); x16 = np.zeros((2, 16)); proj = np.zeros((2, 3)); cov = np.zeros((2, 4)); chi = np.zeros(2)
    ro = np.zeros(2, np.int32); st = np.zeros(2, np.int32)
    nz = cv.capi.ImuNoise(4e-3, 8e-2, 2e-6, 4e-5)
    outs = (p(x16), p(proj), p(cov), p(chi), p(ro), p(st))
    with cv.Solver(**DET) as s:
        lib, h = s._lib, s._h

        def batch(n_pred=2, a_win=win, a_fr=fr, a_m=m, a_t=tt, a_g=gg, a_a=aa, a_nz=nz, n_pts=2, a_pred=pred, a_lm=lm, a_row=row, a_rm=None, a_obs=obs, o=outs):
            q = lambda x: None if x is None else p(x)
            return lib.ctvio_predict_landmarks_batch(h, n_pred, q(a_win), q(a_fr), q(a_m), q(a_t), q(a_g), q(a_a), C.byref(a_nz) if a_nz is not None else None,
                                                     n_pts, q(a_pred), q(a_lm), q(a_row), C.byref(a_rm) if a_rm is not None else None, q(a_obs), *o)

        def single(wid=0, n_pts=2, a_lm=lm, o=outs):
            return lib.ctvio_predict_landmarks(h, wid, -1, 4, p(t), p(gyro), p(acc), C.byref(nz), n_pts, p(a_lm), p(row), None, p(obs), *o)
        assert batch() == 4 and single() == 4                                                        # before the upload
        s.set_windows([x.copy() for x in ws])
        assert batch() == 0 and single() == 0
        assert single(wid=4) == 1 and single(wid=-1) == 1                                            # window id
        assert batch(a_win=np.array([0, 4], np.int32)) == 1
        assert batch(a_fr=np.array([0, ws[3].F], np.int32)) == 1                                     # bias state
        assert batch(n_pred=-1) == 1 and batch(n_pts=-1) == 1                                        # counts
        for name in ("a_win", "a_m", "a_t", "a_g", "a_a", "a_nz", "a_pred", "a_lm", "a_row"):        # null inputs
            assert batch(**{name: None}) == 1, name
        assert batch(a_m=np.array([0, 4], np.int32)) == 1 and batch(a_m=np.array([4097, 4], np.int32)) == 1
        bt = tt.copy(); bt[2] = bt[1]
        assert batch(a_t=bt) == 1                                                                    # times not strictly increasing
        bg = gg.copy(); bg[5, 1] = np.nan
        ba = aa.copy(); ba[0, 0] = np.inf
        assert batch(a_g=bg) == 1 and batch(a_a=ba) == 1                                             # a non-finite measurement
        for bad in (cv.capi.ImuNoise(-1e-3, 8e-2, 2e-6, 4e-5), cv.capi.ImuNoise(4e-3, np.inf, 2e-6, 4e-5), cv.capi.ImuNoise(4e-3, 8e-2, np.nan, 4e-5)):
            assert batch(a_nz=bad) == 1
        assert batch(a_pred=np.array([0, 2], np.int32)) == 1 and batch(a_pred=np.array([-1, 0], np.int32)) == 1
        assert batch(a_lm=np.array([0, w.L], np.int32)) == 1 and batch(a_lm=np.array([-1, 0], np.int32)) == 1
        assert batch(a_pred=np.array([0, 1], np.int32)) == 1                                         # a landmark of the IMU-only window
        assert single(a_lm=np.array([0, w.L], np.int32)) == 1
        assert batch(o=(None, None, None, None, p(ro), p(st))) == 1                                  # all of state16 / proj3 / cov4 / chi2 null
        assert batch(a_obs=None) == 1                                                                # chi2 without obs2
        bo = obs.copy(); bo[1, 0] = np.inf
        assert batch(a_obs=bo) == 1
        for fy, cy, rows, its in ((460.0, 240.0, 480, 0), (460.0, 240.0, 480, 9), (460.0, 240.0, 0, 3), (np.nan, 240.0, 480, 3), (460.0, np.inf, 480, 3)):
            assert batch(a_rm=cv.capi.RowModel(fy, cy, rows, its)) == 1
        assert batch(n_pred=0) == 0 and batch(n_pts=0) == 0                                          # empty calls
        assert batch(o=(p(x16), None, None, None, None, None), a_obs=None) == 0                      # the states alone
        assert batch(o=(None, None, p(cov), None, None, None), a_obs=None) == 0                      # the covariances alone
        assert batch(a_rm=cv.capi.RowModel(460.0, 240.0, 480, 3)) == 0
        o = s.predict_landmarks_batch(win, fr, m, tt, gg, aa, pred, lm, row, obs=obs, row_model=ROW_MODEL)
        assert np.array_equal(o.state, x16) and np.array_equal(o.proj, proj) and np.array_equal(o.cov.ravel(), cov.ravel())
        assert np.array_equal(o.chi2, chi) and np.array_equal(o.row, ro) and np.array_equal(o.status, st)
        b = [x.copy() for x in ws]
        s.set_windows(b)
        sm = s.solve(6)
    with cv.Solver(**DET) as f:
        fb = [x.copy() for x in ws]
        f.set_windows(fb)
        assert f.solve(6) == sm
    assert all(np.array_equal(x.pos, y.pos) and np.array_equal(x.quat, y.quat) for x, y in zip(b, fb))
