"""GPU (-m gpu): ctvio_project_landmarks_batch / ctvio_project_landmarks (csrc/kernels_cov.hpp: k_cov_proj_jac, k_cov_solve tiles of kind TILE_PROJ) against
the NumPy reference of tests/projection_helpers.py: the joint covariance of (trajectory, inverse depths) by the Jacobi-scaled inverse of the
un-eliminated system, formed from the DEVICE's own ctvio_linearize output of the same state (as tests/test_gpu_landmark_points.py, and for its
reason), mapped through the NumPy Jacobian [Jp | j].

Per query, in this order: the status; proj3 (xy: |d| <= point_atol / depth_q (1 + |z|inf) + 1e-12 |z|, depth: rtol 1e-12, atol point_atol); cov4
symmetric to the bit with a positive diagonal and cov_metric <= 4 kappa_s 2^-53 g, g = posecov_helpers.amplification of [Jp | j] over the joint
covariance, the bound itself below 1e-2; chi2 against the extended-precision value from the returned proj3 / cov4 / obs2 at relative
16 kappa_2(Cov + I / img_w^2) 2^-53."""
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
# A query into its landmark's own anchor time predicts the anchor observation itself: the anchor's and the query's knot terms cancel and j is
# zero, so only the line-delay term (row_q - row_i) is left -- and with fix_ld nothing: the covariance is zero by construction, and both the
# device and the reference return rounding residue of the cancelled Jacobians ((1e-11 |J|)^2 Sigma at most: the rtol of test_projjac_host.py).
# Such a query is recognised on the REFERENCE (its covariance below CANCELLED times the size it would have without cancellation) and the
# device's block is held to the same ceiling instead of the relative bound; only the fix_ld variant may contain any.
CANCELLED = 1e-18


def frames_of(w):
    return sorted({int(t) for t in np.concatenate([w.v_ti, w.v_tj])})


def references(w, ref, Q, row_model=None):
    """Per query (l, t, row): the helper's value, final row and value status, the Jacobian, the reference covariance, its status, bound and g."""
    import projection_helpers as pr
    out = []
    for l, t, row in Q:
        proj, r, sv = pr.project(w, l, t, row, row_model)
        pj = pr.projection_jacobian(w, l, t, r) if sv == pr.OK else None
        c, sc = pr.proj_cov_reference(ref, pj, l)
        tol, g = pr.bound(ref, pj, l) if sc == pr.OK else (0.0, 0.0)
        s2 = 0.0
        if sc == pr.OK:      # the size the covariance would have without cancellation between the anchor's and the query's terms
            sd = np.sqrt(np.clip(np.diag(ref.Sig), 0.0, None))[:ref.kp.shape[0]]
            s2 = float((((np.abs(pj.Ja) + np.abs(pj.Jq))[:, ref.kp] @ sd) ** 2).max())
        out.append(SimpleNamespace(l=l, proj=proj, row=r, sv=sv, pj=pj, cov=c, sc=sc, tol=tol, g=g, s2=s2,
                                   cancelled=bool(sc == pr.OK and np.abs(c).max() <= CANCELLED * s2)))
    return out


def gate_points(R):
    """Candidate points for the gate: the helper's prediction moved by a millirad-sized offset that changes with the query."""
    return np.array([(r.proj[:2] + 2e-3 * np.array([np.cos(i), np.sin(i)])) if r.sv == 0 else np.zeros(2) for i, r in enumerate(R)])


def check(w, R, out, what, idx=None, obs=None, allow_cancelled=False):
    """out (Solver.project_landmarks) against the references R[idx]; returns the worst (error / bound, bound, g)."""
    import cov_helpers as ch
    import projection_helpers as pr
    idx = list(range(len(R))) if idx is None else list(idx)
    n = len(idx)
    assert out.proj.shape == (n, 3) and out.status.shape == (n,) and out.row.shape == (n,)
    assert out.cov is None or out.cov.shape == (n, 2, 2)
    worst, n_cancelled = (0.0, 0.0, 0.0), 0
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
        if r.cancelled:
            assert np.isfinite(c).all() and c[0, 1] == c[1, 0] and (np.diag(c) >= 0).all() and np.abs(c).max() <= CANCELLED * r.s2, (what, k, c, r.s2)
            n_cancelled += 1
            continue
        assert np.isfinite(c).all() and c[0, 1] == c[1, 0] and (np.diag(c) > 0).all(), (what, k, c)         # 3. the covariance
        e = ch.cov_metric(c, r.cov)
        print(f"  {what} query {k}: error {e:.3g}, bound {r.tol:.3g}, g {r.g:.3g}") if e > 0.5 * r.tol else None
        assert r.tol < 1e-2, (what, k, r.tol)
        assert e <= r.tol, (what, k, e, r.tol)
        worst = max(worst, (e / r.tol, r.tol, r.g))
        if out.chi2 is not None:                                                                            # 4. the gate
            val, k2 = pr.chi2_reference(out.proj[i], c, obs[i], w.img_w)
            assert abs(out.chi2[i] - val) <= 16 * k2 * EPS * val, (what, k, out.chi2[i], val, k2)
    print(f"{what}: {n} queries ({n_cancelled} with a covariance that is zero by construction), worst error {worst[0]:.3g} of its bound "
          f"{worst[1]:.3g} (g {worst[2]:.3g})")
    assert allow_cancelled or n_cancelled == 0, (what, n_cancelled)
    return worst


def cols(Q):
    a = np.array(Q, np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.int32), np.ascontiguousarray(a[:, 1]), a[:, 2].astype(np.int32)


def tiny_queries(w):
    """Every landmark into every frame time, the rows spread over the image."""
    return [(l, t, (37 * l + 101 * f) % 480) for f, t in enumerate(frames_of(w)) for l in range(w.L)]


def test_tiny_initial_state(cv):
    """`tiny` seed 7 at the initial state (P = 103, L = 12, ld == 0): every landmark into every frame time in one call, then calls of 1, 8, 9 and
    17 queries: one tile, exactly one full tile, a full tile plus one, a third tile with a tail -- through both entries."""
    w = cv.synth.make_window("tiny", seed=7)
    assert (w.P, w.L) == (103, 12) and w.ld == 0.0
    Q = tiny_queries(w)
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        R = references(w, device_reference(s, 0, w), Q)
        obs = gate_points(R)
        assert sum(r.sc == 0 for r in R) >= len(Q) // 2
        check(w, R, s.project_landmarks(0, *cols(Q), obs=obs), "tiny, all", obs=obs)
        for n, first in ((1, 3), (8, 0), (9, 8), (17, 5)):
            idx = range(first, first + n)
            q = [Q[k] for k in idx]
            check(w, R, s.project_landmarks(0, *cols(q), obs=obs[first:first + n]), f"tiny, {n} queries", idx, obs[first:first + n])
            check(w, R, s.project_landmarks_batch([0] * n, *cols(q)), f"tiny, {n} queries, batch entry, no gate", idx)
            check(w, R, s.project_landmarks(0, *cols(q), cov=False), f"tiny, {n} queries, values only", idx)


def config1_queries(w):
    """Each block's own observation, then every landmark into the newest frame at row 240."""
    t_new = frames_of(w)[-1]
    return [(int(w.v_lm[v]), int(w.v_tj[v]), int(w.v_rowj[v])) for v in range(w.V)] + [(l, t_new, 240) for l in range(w.L)]


@pytest.fixture(scope="module")
def config1_solved(cv):
    """`config1` seed 1000 after a 15-iteration solve on an open handle: (solver, the window at the solved state, the device reference, the
    queries, their references)."""
    for s, w in qh.solved_window(cv, "config1", 1000, 15):
        ref = device_reference(s, 0, w)
        Q = config1_queries(w)
        yield s, w, ref, Q, references(w, ref, Q)


def test_config1_solved(config1_solved):
    """`config1` seed 1000, solved (P = 211, L = 50, a free line delay != 0, rows up to 845): each block's own observation gated with the observed
    point, and the newest frame."""
    s, w, ref, Q, R = config1_solved
    assert (w.P, w.L) == (211, 50) and w.ld != 0.0 and not w.fix_ld and int(w.v_rowj.max()) > 0
    obs = gate_points(R)
    obs[:w.V] = w.v_pj
    out = s.project_landmarks(0, *cols(Q), obs=obs)
    assert not out.status[:w.V].any(), out.status[:w.V]
    check(w, R, out, "config1 solved", obs=obs)


def test_cross_checks_against_the_entries_that_exist(config1_solved):
    """The depth equals ctvio_shift_anchor_batch's (row_times = 1) at rtol 1e-12; the block-coincident predictions reproduce the image sums of
    ctvio_residual_summary, sum |img_w (proj - p_j)| over all blocks, at rtol 1e-10."""
    s, w, ref, Q, R = config1_solved
    l, t, row = cols(Q)
    out = s.project_landmarks(0, l, t, row, cov=False)
    ok = out.status == 0
    assert ok[:w.V].all()
    depth, flag = s.shift_anchor([0] * len(Q), l, t, row, row_times=1)
    assert np.allclose(out.proj[ok, 2], depth[ok], rtol=1e-12, atol=0.0), np.abs(out.proj[ok, 2] / depth[ok] - 1).max()
    sums, cnt = s.residual_summary(0)["image"]
    mine = np.abs(w.img_w * (out.proj[:w.V, :2] - w.v_pj)).sum(axis=0)
    print(f"image sums: {mine} vs {sums}")
    assert cnt == w.V and np.allclose(mine, sums, rtol=1e-10, atol=0.0)


def status_queries(cv, w):
    """tiny_queries plus: the last segment at u = 0.5 (the padding knot no factor touches: status 2) and at u = 0 (status 0 or whatever the
    reference says), the first time past the spline and the last before it (status 3)."""
    import posecov_helpers as ph
    K = w.K
    return tiny_queries(w) + [(0, ph.time_of(w, K - 4, 0.5), 0), (0, ph.time_of(w, K - 4, 0.0), 0), (1, ph.time_of(w, K - 3, 0.0), 0), (1, int(w.t0_ns) - 1, 0)]


def run_variant(cv, x, Q, what, allow_cancelled=False):
    with cv.Solver() as s:
        s.set_windows([x.copy()])
        R = references(x, device_reference(s, 0, x), Q)
        obs = gate_points(R)
        vals = s.project_landmarks(0, *cols(Q), cov=False)
        full = s.project_landmarks(0, *cols(Q), obs=obs)
    check(x, R, vals, what + ", values only")
    check(x, R, full, what, obs=obs, allow_cancelled=allow_cancelled)
    assert np.array_equal(vals.proj, full.proj, equal_nan=True) and np.array_equal(vals.row, full.row)
    return R, vals, full


def test_constants_and_statuses(cv):
    """The `tiny` variants of the CPU test: the free window with the last-segment and outside-the-spline queries; rho = -1 on landmark 2 and two
    anchors on landmark 6 (status 3, the other queries' values unchanged to the bit); fixed_upto = 3 and fix_ld (values unchanged to the bit,
    every covariance at the bound; with fix_ld a query on a row > 0 differs from the free one far beyond the bound)."""
    import cov_helpers as ch
    import projection_helpers as pr
    w = cv.synth.make_window("tiny", seed=7)
    Q = status_queries(cv, w)
    nq = len(Q)
    R0, v0, f0 = run_variant(cv, w, Q, "tiny, free")
    assert [r.sc for r in R0[-4:]][0] == pr.NO_INFO and [r.sc for r in R0[-2:]] == [pr.NONE, pr.NONE]
    assert f0.status[nq - 4] == 2 and v0.status[nq - 4] == 0
    wr = w.copy(); wr.rho[2] = -1.0
    _, v1, f1 = run_variant(cv, wr, Q, "tiny, rho = -1 on landmark 2")
    wa = w.copy()
    v = np.nonzero(wa.v_lm == 6)[0]
    assert v.shape[0] >= 2
    wa.v_pi[v[-1], 0] += 1e-3
    _, v2, f2 = run_variant(cv, wa, Q, "tiny, landmark 6 with two anchors")
    for bad, vals, full in ((2, v1, f1), (6, v2, f2)):
        mine = np.array([q[0] == bad for q in Q])
        assert (vals.status[mine] == 3).all() and (full.status[mine] == 3).all() and np.isnan(full.cov[mine]).all()
        assert np.array_equal(vals.proj[~mine], v0.proj[~mine], equal_nan=True) and np.array_equal(full.proj[~mine], v0.proj[~mine], equal_nan=True)
    wf = w.copy(); wf.fixed_upto = 3; wf.normalize()
    wl = w.copy(); wl.fix_ld = True; wl.normalize()
    _, v3, f3 = run_variant(cv, wf, Q, "tiny, fixed_upto = 3")
    R4, v4, f4 = run_variant(cv, wl, Q, "tiny, fix_ld", allow_cancelled=True)
    assert np.array_equal(v3.proj, v0.proj, equal_nan=True) and np.array_equal(v4.proj, v0.proj, equal_nan=True)
    k = max((k for k in range(nq) if f0.status[k] == 0 and f4.status[k] == 0), key=lambda k: Q[k][2])
    d = ch.cov_metric(f4.cov[k], f0.cov[k])
    print(f"fix_ld vs free line delay, query {k} (row {Q[k][2]}): {d:.3g} (bounds {R0[k].tol:.3g}, {R4[k].tol:.3g})")
    assert Q[k][2] > 400 and d > 2 * (R0[k].tol + R4[k].tol)   # more than the rounding of both results can explain


def mixed_queries(ws):
    """Per window with landmarks: every landmark into its newest frame, the rows spread; every third landmark also into its first observation."""
    win, Q = [], []
    for i, w in enumerate(ws):
        if not w.L:
            continue
        t_new = frames_of(w)[-1]
        q = [(l, t_new, (53 * l + 7) % 480) for l in range(w.L)]
        q += [(int(w.v_lm[v]), int(w.v_tj[v]), int(w.v_rowj[v])) for v in range(0, w.V, max(1, w.V // 16))]
        win += [i] * len(q); Q += q
    return np.array(win, np.int32), Q


@pytest.fixture(scope="module")
def mixed(cv):
    """The four windows of test_gpu_covariance's mixed batch, order-fixed linearisation; interleaved queries over the three windows with
    landmarks; the references and the batch call's output -- computed once."""
    from test_gpu_covariance import DET, mixed_batch
    ws, _ = mixed_batch(cv)
    win, Q = mixed_queries(ws)
    order = np.random.default_rng(5).permutation(len(Q))           # the caller's order: windows interleaved
    win, Q = win[order], [Q[k] for k in order]
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        refs = [device_reference(s, i, w) if w.L else None for i, w in enumerate(ws)]
        R = [references(ws[i], refs[i], [q])[0] for i, q in zip(win, Q)]
        obs = gate_points(R)
        out = s.project_landmarks_batch(win, *cols(Q), obs=obs)
    return ws, win, Q, R, obs, out


def take(out, idx):
    return SimpleNamespace(proj=out.proj[idx], cov=None if out.cov is None else out.cov[idx], chi2=None if out.chi2 is None else out.chi2[idx],
                           row=out.row[idx], status=out.status[idx])


def same(a, b):
    return qh.same_bits(a, b, ("proj", "cov", "chi2", "row", "status"))


def test_mixed_batch_against_reference(mixed):
    """One call over the mixed batch, the queries of three windows interleaved; the L = 0 window takes no query and breaks nothing."""
    ws, win, Q, R, obs, out = mixed
    assert ws[3].L == 0 and not (win == 3).any()
    for i, w in enumerate(ws):
        idx = np.nonzero(win == i)[0]
        if idx.shape[0]:
            check(w, R, take(out, idx), f"mixed window {i} (P {w.P}, L {w.L})", idx, obs[idx])


def test_mixed_batch_bits(cv, mixed):
    """The batch call's bits from: the single-window entry per window, a second batch call, a shuffled query order, a call without the gate, a
    call with proj3 alone."""
    from test_gpu_covariance import DET
    p = cv.capi._p
    ws, win, Q, R, obs, out = mixed
    l, t, row = cols(Q)
    n = len(Q)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        for i in range(len(ws)):
            idx = np.nonzero(win == i)[0]
            if idx.shape[0]:
                assert same(s.project_landmarks(i, l[idx], t[idx], row[idx], obs=obs[idx]), take(out, idx)), i
        assert same(s.project_landmarks_batch(win, l, t, row, obs=obs), out)
        sh = np.random.default_rng(9).permutation(n)
        assert same(s.project_landmarks_batch(win[sh], l[sh], t[sh], row[sh], obs=obs[sh]), take(out, sh))
        nog = s.project_landmarks_batch(win, l, t, row)
        assert nog.chi2 is None and np.array_equal(nog.cov, out.cov, equal_nan=True) and np.array_equal(nog.proj, out.proj, equal_nan=True)
        proj = np.zeros((n, 3))
        assert s._lib.ctvio_project_landmarks_batch(s._h, n, p(win), p(l), p(t), p(row), None, None, p(proj), None, None, None, None) == 0
        assert np.array_equal(proj, out.proj, equal_nan=True)
        half = np.arange(0, n, 2)
        assert same(s.project_landmarks_batch(win[half], l[half], t[half], row[half], obs=obs[half]), take(out, half))


def test_row_model(cv, config1_solved):
    """Solved `config1`, a pinhole row map over 480 rows, first guess rows / 2, every landmark into the newest frame and into its own
    observations: row_out equals the helper's, the values and covariances are the helper's at that row.  A query whose first guess lies
    inside the spline and whose iterated row leaves it: status 3."""
    import projection_helpers as pr
    s, w, ref, Q, _ = config1_solved
    q = [(l, t, 240) for l, t, _ in Q[::4]]
    R = references(w, ref, q, ROW_MODEL)
    assert sum(r.sv == 0 and r.row != 240 for r in R) > len(q) // 2
    check(w, R, s.project_landmarks(0, *cols(q), row_model=ROW_MODEL), "config1 solved, row model")
    check(w, R, s.project_landmarks(0, *cols(q), row_model=ROW_MODEL, cov=False), "config1 solved, row model, values only")
    ld_ns = int(np.int64(w.ld * 1e9))
    assert ld_ns > 0
    t_edge = int(w.t0_ns) + (w.K - 3) * int(w.dt_ns) - 100 * ld_ns      # rows below 100 are inside the spline, the others outside
    edge = [(l, t_edge, 0) for l in range(w.L)]
    Re = references(w, ref, edge, ROW_MODEL)
    plain = [pr.project(w, l, t, r)[2] for l, t, r in edge]
    left = [k for k, r in enumerate(Re) if r.sv == pr.NONE and plain[k] == pr.OK]
    assert left, "no landmark leaves the spline under the row iteration"
    out = s.project_landmarks(0, *cols(edge), row_model=ROW_MODEL)
    check(w, Re, out, "config1 solved, row model at the end of the spline")
    assert (out.status[left] == 3).all() and (out.row[left] == -1).all()


def test_leaves_the_solve_alone(cv, mixed):
    """State bits, graph captures and a following solve are unchanged by the calls; ctvio_covariance_batch on the same handle gives identical bits
    before and after them; the timing slots of both calls."""
    from test_gpu_covariance import mixed_batch
    ws, win, Q, R, obs, out = mixed
    _, sels = mixed_batch(cv)
    l, t, row = cols(Q)

    def calls(s, b):
        o1 = s.project_landmarks_batch(win, l, t, row, obs=obs)
        assert np.isfinite(o1.cov[o1.status == 0]).all() and np.isfinite(o1.proj[o1.status != 3]).all()
        ms, launches = s.last_timing()
        assert launches[:3].tolist() == [1, 1, 1] and ms[7] >= ms[1] > 0 and ms[2] > 0
        o2 = s.project_landmarks_batch(win, l, t, row, cov=False)
        ms, launches = s.last_timing()
        assert launches[:3].tolist() == [0, 0, 1] and ms[7] >= ms[2] > 0
        assert np.array_equal(o2.proj, o1.proj, equal_nan=True) and np.array_equal(o2.row, o1.row)
    qh.check_leaves_the_solve_alone(cv, ws, calls, sels)


def test_refusals_leave_the_handle_usable(cv):
    """CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for every case of the header; n == 0 is fine; the handle solves afterwards like a
    fresh one."""
    import ctypes as C
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    t_in = frames_of(w)[1]
    lm = np.array([0, 1], np.int32); t = np.array([t_in, t_in], np.int64); row = np.array([0, 5], np.int32); win = np.zeros(2, np.int32)
    obs = np.zeros((2, 2)); proj = np.zeros((2, 3)); cov = np.zeros((2, 4)); chi = np.zeros(2); ro = np.zeros(2, np.int32); st = np.zeros(2, np.int32)
    rm = cv.capi.RowModel(460.0, 240.0, 480, 3)
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        single = lambda n, a_lm, a_t, a_row, a_rm, a_obs, *o: lib.ctvio_project_landmarks(h, 0, n, a_lm, a_t, a_row, a_rm, a_obs, *o)
        batch = lambda n, a_win, a_lm, a_t, a_row, a_rm, a_obs, *o: lib.ctvio_project_landmarks_batch(h, n, a_win, a_lm, a_t, a_row, a_rm, a_obs, *o)
        outs = (p(proj), p(cov), p(chi), p(ro), p(st))
        assert single(2, p(lm), p(t), p(row), None, p(obs), *outs) == 4
        assert batch(2, p(win), p(lm), p(t), p(row), None, p(obs), *outs) == 4
        with pytest.raises(cv.capi.CtvioError):
            s.project_landmarks(0, lm, t, row)
        s.set_windows([w.copy()])
        assert lib.ctvio_project_landmarks(h, 1, 2, p(lm), p(t), p(row), None, p(obs), *outs) == 1          # window id
        assert lib.ctvio_project_landmarks(h, -1, 2, p(lm), p(t), p(row), None, p(obs), *outs) == 1
        assert batch(2, p(np.array([0, 1], np.int32)), p(lm), p(t), p(row), None, p(obs), *outs) == 1
        assert single(2, p(np.array([0, w.L], np.int32)), p(t), p(row), None, p(obs), *outs) == 1           # landmark index
        assert single(2, p(np.array([-1, 0], np.int32)), p(t), p(row), None, p(obs), *outs) == 1
        assert single(-1, p(lm), p(t), p(row), None, p(obs), *outs) == 1                                     # n < 0
        assert single(2, None, p(t), p(row), None, p(obs), *outs) == 1                                       # null inputs
        assert single(2, p(lm), None, p(row), None, p(obs), *outs) == 1
        assert single(2, p(lm), p(t), None, None, p(obs), *outs) == 1
        assert batch(2, None, p(lm), p(t), p(row), None, p(obs), *outs) == 1
        assert single(2, p(lm), p(t), p(row), None, p(obs), None, None, None, None, None) == 1               # every output null
        assert single(2, p(lm), p(t), p(row), None, None, *outs) == 1                                        # chi2 without obs2
        bad = obs.copy(); bad[1, 0] = np.inf
        assert single(2, p(lm), p(t), p(row), None, p(bad), *outs) == 1                                      # a non-finite candidate
        for fy, cy, rows, its in ((460.0, 240.0, 480, 0), (460.0, 240.0, 480, 9), (460.0, 240.0, 0, 3), (np.nan, 240.0, 480, 3), (460.0, np.inf, 480, 3)):
            assert single(2, p(lm), p(t), p(row), C.byref(cv.capi.RowModel(fy, cy, rows, its)), p(obs), *outs) == 1
        with pytest.raises(cv.capi.CtvioError, match="invalid"):
            s.project_landmarks(3, lm, t, row)
        assert single(0, None, None, None, None, None, None, None, None, None, None) == 0                   # n == 0
        assert batch(0, None, None, None, None, None, None, None, None, None, None, None) == 0
        assert single(2, p(lm), p(t), p(row), None, None, None, None, None, None, p(st)) == 0                # the statuses alone
        assert single(2, p(lm), p(t), p(row), None, None, None, p(cov), None, None, None) == 0               # the covariances alone
        assert single(2, p(lm), p(t), p(row), C.byref(rm), p(obs), *outs) == 0
        o = s.project_landmarks(0, lm, t, row, obs=obs, row_model=rm)
        assert np.array_equal(o.proj, proj) and np.array_equal(o.cov.ravel(), cov.ravel()) and np.array_equal(o.chi2, chi)
        assert np.array_equal(o.row, ro) and np.array_equal(o.status, st)
        qh.check_usable_after(cv, w, s)


def test_adaptor_project_landmarks_matches_python(cv, tmp_path):
    """tests/project_landmarks_demo.cpp through the C++ adaptor: predictions, covariances, gates and statuses of every block's own observation
    equal the Python call on the same window at the demo's solved state, bit for bit."""
    w0 = cv.synth.make_window("config1", seed=1005)
    K, F, L, V = w0.K, w0.F, w0.L, w0.V
    wa, rest = qh.run_demo(qh.build_demo("project_landmarks_demo", tmp_path), w0, tmp_path, 15)
    assert rest[0] == 1 and rest[1] == V
    proj_cpp = rest[2:2 + 3 * V].reshape(V, 3)
    cov_cpp = rest[2 + 3 * V:2 + 7 * V].reshape(V, 2, 2)
    chi_cpp = rest[2 + 7 * V:2 + 8 * V]
    st_cpp = rest[2 + 8 * V:2 + 9 * V]
    rest = rest[2 + 9 * V:]
    assert rest[0] == 1 and rest[1] == V
    only_cpp = rest[2:2 + 3 * V].reshape(V, 3)
    with cv.Solver() as s:
        s.set_windows([wa])
        o = s.project_landmarks(0, wa.v_lm, wa.v_tj, wa.v_rowj, obs=wa.v_pj)
    assert not o.status.any() and not st_cpp.any()
    print(f"adaptor vs Python: predictions {np.max(np.abs(proj_cpp - o.proj)):.3g}, covariances {np.max(np.abs(cov_cpp - o.cov)):.3g}, "
          f"gates {np.max(np.abs(chi_cpp - o.chi2)):.3g} (absolute)")
    assert np.array_equal(proj_cpp, o.proj) and np.array_equal(only_cpp, o.proj) and np.array_equal(cov_cpp, o.cov) and np.array_equal(chi_cpp, o.chi2)
