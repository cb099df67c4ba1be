"""GPU (-m gpu): ctvio_nav_state_batch / ctvio_nav_state (csrc/kernels_cov.hpp: k_cov_nav_jac, k_cov_solve tiles of kind TILE_NAV) against the NumPy
reference: cov_helpers.cov_reference on the DEVICE's own ctvio_linearize output of the same state with all P unknowns selected (as
tests/test_gpu_pose_covariance.py, and for its reason), mapped through the NumPy Jacobian of tests/navstate_helpers.py.

Tolerance, entry by entry: |Pi_ab - ref_ab| / sqrt(ref_aa ref_bb) <= 4 kappa_s 2^-53 sqrt(g_a g_b); 4 kappa_s 2^-53 is the covariance tests' own
bound and g_a = (sum_k |J_ak| sqrt(Sigma_kk))^2 / Pi_aa the amplification of row a through J (an error of tol sqrt(Sigma_kk Sigma_ll) per entry of
Sigma becomes at most tol s_a s_b in Pi_ab).  The velocity rows cancel between neighbouring knots, so their g is larger than the pose rows'
(about 14 on `tiny`, 144 on `config1`); the bias rows are one-hot, g = 1.  Every check asserts that its bound stays below 1e-4 for entries
among pose and bias rows -- the size of the leftover-damping error the covariance tests exist to catch -- and below 1e-3 for entries that
involve a velocity row, whose own errors (a wrong derivative coefficient, a missing 1 / dt, a knot offset) are O(1)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

FRAME_DT = 100_000_000      # synth.py: frame_dt_ns of every configuration used here
OFF = ~np.eye(15, dtype=bool)


def check(w, ref, times, frames, state, cov, st, what, expect=None):
    """Every query of one window (w: the window at the device's state) against the reference: the status, the rule of that status, the state
    values against the oracle's NumPy spline evaluation, and for status 0 every entry of the covariance at its bound.  Returns the largest
    (error / bound, error, bound) over the entries."""
    import cov_helpers as ch
    import navstate_helpers as nh
    from scipy.spatial.transform import Rotation as Rot
    n = len(times)
    assert state.shape == (n, 16) and cov.shape == (n, 15, 15) and st.shape == (n,)
    worst = (0.0, 0.0, 0.0)
    for i, t in enumerate(times):
        f = None if frames is None else int(frames[i])
        jac = nh.nav_jacobian(w, t, f)
        r, rs = nh.nav_cov_reference(ref, jac, w.K)
        assert st[i] == rs, (what, i, t, st[i], rs)
        if expect is not None:
            assert st[i] == expect[i], (what, i, t, st[i], expect[i])
        c = cov[i]
        if rs == nh.OUTSIDE:
            assert np.isnan(c).all() and np.isnan(state[i]).all(), (what, i)
            continue
        R, p, v, b = nh.nav_numpy(w, t, f)
        x = state[i]
        assert np.abs(x[0:3] - p).max() <= 1e-12 * max(1.0, np.abs(p).max()) and np.abs(x[7:10] - v).max() <= 1e-12 * max(1.0, np.abs(v).max()), (what, i)
        assert (Rot.from_quat(x[3:7]).inv() * R).magnitude() <= 1e-12 and np.array_equal(x[10:16], b), (what, i)
        if rs == nh.UNTOUCHED:
            assert np.isposinf(np.diag(c)).all() and not c[OFF].any(), (what, i)
            continue
        assert np.isfinite(c).all() and np.array_equal(c, c.T), (what, i)
        if not r.any():                            # only constant unknowns: the exact zero matrix
            assert not c.any(), (what, i)
            continue
        assert (np.diag(c)[np.diag(r) > 0] > 0).all(), (what, i)
        g = nh.row_amplification(jac.J, ref.cov_full)
        tol, cap = nh.entry_bounds(ch.bound(ref.kappa), g)
        e = nh.entry_errors(c, r)
        k = np.unravel_index(np.argmax(e / tol), e.shape)
        print(f"{what} query {i} (s {jac.s}, u {jac.u:.3g}, frame {jac.frame}): kappa_s {ref.kappa:.3g}, g pose {g[:6].max():.3g} velocity {g[6:9].max():.3g} "
              f"bias {g[9:].max():.3g}, bound pose/bias {tol[np.ix_([0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14], [0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14])].max():.3g} "
              f"velocity {tol.max():.3g}, worst entry {k}: error {e[k]:.3g} at bound {tol[k]:.3g}")
        assert np.isfinite(ref.kappa) and (tol < cap).all(), (what, i, float(tol.max()))
        assert (e <= tol).all(), (what, i, k, float(e[k]), float(tol[k]))
        worst = max(worst, (float(e[k] / tol[k]), float(e[k]), float(tol[k])))
    return worst


def test_tiny_initial_state(cv):
    """Case 1: `tiny` seed 7 at the initial state (P = 103, four 32-row blocks, bias rows at 72..101, the last knot untouched): statuses 0, 0, 0,
    0, 0, 2, 3, 3 with frames i mod F; frame = NULL equals frame F - 1."""
    import navstate_helpers as nh
    w = cv.synth.make_window("tiny", seed=7)
    assert (w.K, w.P, w.F) == (12, 103, 5)
    times = [nh.time_of(w, s, u) for s, u in ((0, 0.0), (1, 0.9), (5, 0.37), (7, 0.999), (8, 0.0), (8, 0.5))]
    times += [w.t0_ns - 1, w.t0_ns + (w.K - 3) * w.dt_ns]           # before t0; the end of the spline
    frames = [i % w.F for i in range(len(times))]
    import query_harness as qh
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = qh.device_reference(s, 0, w)
        state, cov, st = s.nav_state(0, times, frames)
        state_n, cov_n, st_n = s.nav_state(0, times)
        state_l, cov_l, st_l = s.nav_state(0, times, [w.F - 1] * len(times))
    expect = [0, 0, 0, 0, 0, 2, 3, 3]
    assert st.tolist() == expect and st_n.tolist() == expect
    check(w, ref, times, frames, state, cov, st, "tiny", expect=expect)
    check(w, ref, times, None, state_n, cov_n, st_n, "tiny, newest frame", expect=expect)
    assert np.array_equal(state_n, state_l, equal_nan=True) and np.array_equal(cov_n, cov_l, equal_nan=True) and np.array_equal(st_n, st_l)
    assert np.isposinf(np.diag(cov[5])).all() and not cov[5][OFF].any() and np.isfinite(state[5]).all()
    assert np.isnan(cov[6:]).all() and np.isnan(state[6:]).all()
    for c in cov[:5]:
        assert np.isfinite(c).all() and np.array_equal(c, c.T) and (np.diag(c) > 0).all()


@pytest.fixture(scope="module")
def config1_solved(cv):
    """`config1` seed 1000 after a 15-iteration solve on an open handle: (solver, the window at the solved state, the device reference)."""
    import query_harness as qh
    for s, w in qh.solved_window(cv, "config1", 1000, 15):
        yield s, w, qh.device_reference(s, 0, w)


def test_config1_solved_frames(config1_solved):
    """Case 2: `config1` seed 1000, solved (P = 211): every frame time with its own bias state and the same times with the newest -- 22 queries
    in one call (a call takes a frame array or NULL, so the second eleven name F - 1); the call with frame = NULL gives their states and is checked like them."""
    s, w, ref = config1_solved
    assert w.P == 211 and w.F == 11
    times = [int(w.t0_ns + f * FRAME_DT) for f in range(w.F)]
    frames = list(range(w.F))
    both_t, both_f = times + times, frames + [w.F - 1] * w.F
    state, cov, st = s.nav_state(0, both_t, both_f)
    assert state.shape == (22, 16) and not st.any(), st
    e = check(w, ref, both_t, both_f, state, cov, st, "config1 solved")
    state_n, cov_n, st_n = s.nav_state(0, times)
    assert np.array_equal(state_n, state[11:]) and np.array_equal(st_n, st[11:])
    check(w, ref, times, None, state_n, cov_n, st_n, "config1 solved, frame NULL")
    print(f"config1 solved: worst error / bound {e[0]:.3g} (error {e[1]:.3g} at bound {e[2]:.3g})")


def test_constants(cv):
    """Case 3: `tiny` with fixed_upto = 3 and lock_bg = 1: at (0, 0) the pose, velocity and bg rows and columns are exact zeros and the ba block
    is positive; at (1, 0.5) only knot 4 contributes and the result equals the reference."""
    import navstate_helpers as nh
    w = cv.synth.make_window("tiny", seed=7)
    w.fixed_upto = 3; w.lock_bg = 1
    w.normalize()
    times = [nh.time_of(w, 0, 0.0), nh.time_of(w, 1, 0.5)]
    frames = [1, 2]
    import query_harness as qh
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = qh.device_reference(s, 0, w)
        state, cov, st = s.nav_state(0, times, frames)
    assert st.tolist() == [0, 0]
    assert not cov[0][:12].any() and not cov[0][:, :12].any() and (np.diag(cov[0])[12:] > 0).all()
    d = np.diag(cov[1])
    assert (d[:9] > 0).all() and not cov[1][9:12].any() and not cov[1][:, 9:12].any() and (d[12:] > 0).all()
    check(w, ref, times, frames, state, cov, st, "tiny, constants")


def mixed_queries(ws):
    """Three queries per window of the mixed batch, interleaved across the windows: (win, t_ns, frame); the bias states 0, F / 2 and F - 1.
    The times are (1, 0.3), (K / 2, 0) and (K / 3, 0.75), not the pose test's (K - 5, 0.75): at the batch's INITIAL state the position
    variance grows along the window, away from the prior, while the velocity variance does not, so the amplification g of the velocity rows
    grows with the segment -- on the oracle's H of the 34-knot window (kappa_s 1.5e10) from 6 at segment 1 through 81 at (11, 0.75) and 148
    at (17, 0.75) to 382 at (29, 0.75), where the BOUND itself is 2.6e-3 and says nothing any more.  The cap of 1e-3 on the bound holds
    there for g < 149; (K / 3, 0.75) keeps a factor of 1.8 below it on that window and more on the others.  Late segments at a solved
    state, where kappa_s is smaller, are case 2's."""
    import navstate_helpers as nh
    per = [[nh.time_of(w, 1, 0.3), nh.time_of(w, w.K // 2, 0.0), nh.time_of(w, w.K // 3, 0.75)] for w in ws]
    perf = [[0, w.F // 2, w.F - 1] for w in ws]
    win = [i for j in range(3) for i in range(len(ws))]
    t = [per[i][j] for j in range(3) for i in range(len(ws))]
    f = [perf[i][j] for j in range(3) for i in range(len(ws))]
    return np.array(win, np.int32), np.array(t, np.int64), np.array(f, np.int32)


@pytest.fixture(scope="module")
def mixed(cv):
    """The four windows of test_gpu_covariance's mixed batch (`tiny`, `config1`, the F = 16 window on the envelope panel path, the IMU-only
    predict window with locked biases and L = 0), order-fixed linearisation; the queries, the device references and the plain call's outputs --
    computed once."""
    import query_harness as qh
    from test_gpu_covariance import DET, mixed_batch
    ws, _ = mixed_batch(cv)
    win, t, f = mixed_queries(ws)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        refs = [qh.device_reference(s, i, w) for i, w in enumerate(ws)]
        out = s.nav_state_batch(win, t, f)
    return ws, win, t, f, refs, out


def test_mixed_batch_against_reference(mixed):
    """Case 4: one call over the four windows, every query at the bound."""
    ws, win, t, f, refs, (state, cov, st) = mixed
    for i, w in enumerate(ws):
        idx = np.nonzero(win == i)[0]
        check(w, refs[i], [int(x) for x in t[idx]], f[idx], state[idx], cov[idx], st[idx], f"mixed window {i} (P {w.P})")


def test_mixed_batch_bits(cv, mixed):
    """Case 4: the bits of a query depend on its window, time and frame alone: the single-window entry, a second call, the reversed order, and
    calls with other counts per window give the batch call's bits."""
    import query_harness as qh
    ws, win, t, f, _, out = mixed
    with cv.Solver(**qh.DET) as s:
        s.set_windows([w.copy() for w in ws])
        qh.check_batch_bits(s.nav_state, s.nav_state_batch, win, (t, f), out, len(ws))


def test_cross_checks(config1_solved):
    """Case 5, on `config1`: J_np Sigma_30 J_np^T with Sigma_30 = ctvio_covariance of the query's 24 knot unknowns and 6 bias unknowns; the pose
    block against ctvio_pose_covariance; the values against ctvio_spline_eval and get_state; cov=False gives the same state bits."""
    import cov_helpers as ch
    import navstate_helpers as nh
    import posecov_helpers as ph
    s, w, ref = config1_solved
    fr = 4
    t = nh.time_of(w, w.K // 2, 0.37)
    jac = nh.nav_jacobian(w, t, fr)
    sel = list(range(6 * jac.s, 6 * jac.s + 24)) + list(range(6 * w.K + 6 * fr, 6 * w.K + 6 * fr + 6))
    state, cov, st = s.nav_state(0, [t], [fr])
    blk, _, sing = s.covariance(0, sel)
    assert st[0] == 0 and sing == 0
    via = jac.J[:, sel] @ blk @ jac.J[:, sel].T
    g = nh.row_amplification(jac.J, ref.cov_full)
    tol, cap = nh.entry_bounds(ch.bound(ref.kappa), g)
    e = nh.entry_errors(cov[0], via)
    print(f"nav entry vs J Sigma_30 J^T: worst error / bound {(e / tol).max():.3g}, error {e.max():.3g}")
    assert (tol < cap).all() and (e <= tol).all()
    pc, pst = s.pose_covariance(0, [t])
    ptol = ch.bound(ref.kappa) * ph.amplification(jac.J[:6], ref.cov_full)
    pe = ch.cov_metric(cov[0][:6, :6], pc[0])
    print(f"pose block vs ctvio_pose_covariance: {pe:.3g} at bound {ptol:.3g}")
    assert pst[0] == 0 and ptol < 1e-4 and pe <= ptol
    times = [int(w.t0_ns + f * FRAME_DT) for f in range(w.F)] + [t]
    frames = list(range(w.F)) + [fr]
    st16, _, stat = s.nav_state(0, times, frames)
    pose, vel, _, _ = s.spline_eval(0, times)
    x = np.concatenate([pose, vel], 1)
    assert not stat.any() and (np.abs(st16[:, :10] - x) <= 1e-12 * np.maximum(1.0, np.abs(x))).all()
    assert np.array_equal(st16[:, 10:], s.get_state(0).bias[frames])
    st16v, covv, statv = s.nav_state(0, times, frames, cov=False)
    assert covv is None and np.array_equal(st16v, st16) and np.array_equal(statv, stat)
    ms, launches = s.last_timing()
    assert launches[:3].tolist() == [0, 0, 1] and ms[7] >= ms[2] > 0


def test_leaves_the_solve_alone(cv, mixed):
    """Case 6: state bits, graph captures and a following solve are unchanged by the call; ctvio_covariance_batch on the same handle gives
    identical bits before and after it; last_timing reports one launch of each of the three kernels."""
    import query_harness as qh
    from test_gpu_covariance import mixed_batch
    ws, win, t, f, _, _ = mixed
    _, sels = mixed_batch(cv)

    def calls(s, b):
        o1 = s.nav_state_batch(win, t, f)
        assert np.isfinite(o1[1][o1[2] == 0]).all() and np.isfinite(o1[0]).all()
        ms, launches = s.last_timing()
        assert launches[:3].tolist() == [1, 1, 1] and ms[7] >= ms[1] > 0 and not ms[3:7].any()
        s.nav_state_batch(win, t, cov=False)
    qh.check_leaves_the_solve_alone(cv, ws, calls, sels)


def test_refusals_leave_the_handle_usable(cv):
    """Case 7: CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a window id out of range, a frame outside [0, F), a negative n, a NULL win
    / t_ns with n > 0, all three outputs NULL with n > 0; n == 0 is fine; the handle solves afterwards like a fresh one."""
    import query_harness as qh
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    t = np.array([w.t0_ns + 1], np.int64); win = np.zeros(1, np.int32); fr = np.zeros(1, np.int32)
    x = np.zeros(16); cov = np.zeros(225); st = np.zeros(1, np.int32)
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        assert lib.ctvio_nav_state_batch(h, 1, p(win), p(t), None, p(x), p(cov), p(st)) == 4
        assert lib.ctvio_nav_state(h, 0, 1, p(t), None, p(x), p(cov), p(st)) == 4
        s.set_windows([w.copy()])
        bad = np.array([1], np.int32)
        assert lib.ctvio_nav_state_batch(h, 1, p(bad), p(t), None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_nav_state(h, 1, 1, p(t), None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_nav_state(h, -1, 1, p(t), None, p(x), p(cov), p(st)) == 1
        for f in (-1, w.F):
            badf = np.array([f], np.int32)
            assert lib.ctvio_nav_state_batch(h, 1, p(win), p(t), p(badf), p(x), p(cov), p(st)) == 1
            assert lib.ctvio_nav_state(h, 0, 1, p(t), p(badf), p(x), p(cov), p(st)) == 1
            assert lib.ctvio_nav_state(h, 0, 1, p(t), p(badf), p(x), None, p(st)) == 1
        assert lib.ctvio_nav_state_batch(h, -1, p(win), p(t), None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_nav_state(h, 0, -1, p(t), None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_nav_state_batch(h, 1, None, p(t), None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_nav_state_batch(h, 1, p(win), None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_nav_state(h, 0, 1, None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_nav_state_batch(h, 1, p(win), p(t), None, None, None, None) == 1
        assert lib.ctvio_nav_state(h, 0, 1, p(t), p(fr), None, None, None) == 1
        with pytest.raises(cv.capi.CtvioError, match="invalid"):
            s.nav_state_batch([3], t)
        assert lib.ctvio_nav_state_batch(h, 0, None, None, None, None, None, None) == 0
        assert lib.ctvio_nav_state(h, 0, 0, None, None, None, None, None) == 0
        x0, c0, s0 = s.nav_state(0, [])
        assert x0.shape == (0, 16) and c0.shape == (0, 15, 15) and s0.shape == (0,)
        x1, c1, s1 = s.nav_state(0, t)
        assert s1[0] == 0
        assert lib.ctvio_nav_state(h, 0, 1, p(t), None, None, p(cov), None) == 0                   # each output alone
        assert np.array_equal(cov, c1[0].ravel())
        assert lib.ctvio_nav_state(h, 0, 1, p(t), None, p(x), None, None) == 0
        assert np.array_equal(x, x1[0])
        assert lib.ctvio_nav_state(h, 0, 1, p(t), None, None, None, p(st)) == 0 and st[0] == 0
        qh.check_usable_after(cv, w, s)


def test_adaptor_nav_state_matches_python(cv, tmp_path):
    """Case 8: tests/nav_state_demo.cpp through the C++ adaptor: the states and covariances at five times, with the newest bias state and with
    bias state 1, equal the Python call on the same window at the demo's solved state, bit for bit."""
    import query_harness as qh
    w0 = cv.synth.make_window("config1", seed=1005)
    K, F = w0.K, w0.F
    n = 5
    wa, rest = qh.run_demo(qh.build_demo("nav_state_demo", tmp_path), w0, tmp_path, 15, n)
    got = []
    for _ in range(2):
        assert rest[0] == 1 and rest[1] == n
        got.append((rest[2:2 + 16 * n].reshape(n, 16), rest[2 + 16 * n:2 + 241 * n].reshape(n, 15, 15)))
        rest = rest[2 + 241 * n:]
    assert rest[0] == 0                               # a time outside the spline: reported, not thrown
    times = [int(w0.t0_ns + (i + 1) * (K - 4) * w0.dt_ns // (n + 1)) for i in range(n)]
    with cv.Solver() as s:
        s.set_windows([wa])
        new = s.nav_state(0, times)
        one = s.nav_state(0, times, [1] * n)
    for (x_cpp, c_cpp), (x, c, st) in zip(got, (new, one)):
        assert not st.any()
        assert np.array_equal(x_cpp, x) and np.array_equal(c_cpp, c)
    assert np.array_equal(got[0][0][:, 10:], np.tile(wa.bias[F - 1], (n, 1))) and np.array_equal(got[1][0][:, 10:], np.tile(wa.bias[1], (n, 1)))
