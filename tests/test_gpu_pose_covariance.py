"""GPU (-m gpu): ctvio_pose_covariance_batch / ctvio_pose_covariance (csrc/kernels_cov.hpp: k_cov_pose_jac, k_cov_solve tiles of kind TILE_POSE) against
the NumPy reference: cov_helpers.cov_reference on the DEVICE's own ctvio_linearize output of the same state with all P unknowns selected (as
tests/test_gpu_covariance.py, and for its reason), mapped through the NumPy Jacobian of tests/posecov_helpers.py.

Tolerance everywhere: 4 kappa_s 2^-53 g on cov_helpers.cov_metric of the 6 x 6 (|a - b| / sqrt(b_ii b_jj)); 4 kappa_s 2^-53 is the covariance
tests' own bound and g = max_a (sum_k |J_ak| sqrt(Sigma_kk))^2 / Pi_aa the amplification through J (an error of tol sqrt(Sigma_kk Sigma_ll) per
entry of Sigma becomes at most tol s_a s_b in Pi).  Every check asserts that its bound stays below 1e-4, the size of the smallest modelling error
the covariance tests are built to catch (leftover damping at radius 1e4)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import query_harness as qh  # noqa: E402
from query_harness import device_reference  # noqa: E402,F401

FRAME_DT = 100_000_000      # synth.py: frame_dt_ns of every configuration used here


def check(w, ref, times, cov, st, ext, what, expect=None):
    """Every query of one window (w: the window at the device's state) against the reference: the status, the rule of that status, and for
    status 0 the error at the bound.  Returns the largest (error, bound, g)."""
    import cov_helpers as ch
    import posecov_helpers as ph
    assert cov.shape == (len(times), 6, 6) and st.shape == (len(times),)
    worst = (0.0, 0.0, 0.0)
    for i, t in enumerate(times):
        jac = ph.pose_jacobian(w, t, *ext)
        r, rs = ph.pose_cov_reference(ref, jac)
        assert st[i] == rs, (what, i, t, st[i], rs)
        if expect is not None:
            assert st[i] == expect[i], (what, i, t, st[i], expect[i])
        c = cov[i]
        if rs == ph.OUTSIDE:
            assert np.isnan(c).all(), (what, i)
            continue
        if rs == ph.UNTOUCHED:
            assert np.isposinf(np.diag(c)).all() and not c[~np.eye(6, dtype=bool)].any(), (what, i)
            continue
        assert np.isfinite(c).all() and np.array_equal(c, c.T), (what, i)
        if not r.any():                            # only constant knots: the exact zero matrix
            assert not c.any(), (what, i)
            continue
        assert (np.diag(c) > 0).all(), (what, i)
        g = ph.amplification(jac.J, ref.cov_full)
        tol = ch.bound(ref.kappa) * g
        e = ch.cov_metric(c, r)
        print(f"{what} query {i} (s {jac.s}, u {jac.u:.3g}): kappa_s {ref.kappa:.3g}, g {g:.3g}, bound {tol:.3g}, error {e:.3g}")
        assert np.isfinite(ref.kappa) and tol < 1e-4, (what, i, tol)
        assert e <= tol, (what, i, e, tol)
        worst = max(worst, (e, tol, g))
    return worst


def test_tiny_initial_state(cv):
    """Case 1: `tiny` seed 7 at the initial state (P = 103, four 32-row blocks, the last knot untouched): statuses 0, 0, 0, 0, 0, 2, 3, 3."""
    import posecov_helpers as ph
    w = cv.synth.make_window("tiny", seed=7)
    assert (w.K, w.P) == (12, 103)
    times = [ph.time_of(w, s, u) for s, u in ((0, 0.0), (1, 0.9), (5, 0.37), (7, 0.999), (8, 0.0), (8, 0.5))]
    times += [w.t0_ns - 1, w.t0_ns + (w.K - 3) * w.dt_ns]           # before t0; the end of the spline
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = device_reference(s, 0, w)
        cov, st = s.pose_covariance(0, times)
    assert st.tolist() == [0, 0, 0, 0, 0, 2, 3, 3]
    check(w, ref, times, cov, st, (None, None), "tiny", expect=[0, 0, 0, 0, 0, 2, 3, 3])
    assert np.isposinf(np.diag(cov[5])).all() and not cov[5][~np.eye(6, dtype=bool)].any()
    assert np.isnan(cov[6:]).all()
    for c in cov[:5]:
        assert np.isfinite(c).all() and np.array_equal(c, c.T) and (np.diag(c) > 0).all()


@pytest.fixture(scope="module")
def config1_solved(cv):
    """`config1` seed 1000 after a 15-iteration solve on an open handle: (solver, the window at the solved state, the device reference)."""
    for s, w in qh.solved_window(cv, "config1", 1000, 15):
        yield s, w, device_reference(s, 0, w)


def config1_times(w):
    """All frame times plus the row times t + row * ld (the time as the factors take it: integer-ns line delay) for rows 0, 240 and 479."""
    ld_ns = int(w.ld * 1e9)
    frames = [int(w.t0_ns + f * FRAME_DT) for f in range(w.F)]
    return frames + [t + row * ld_ns for t in frames for row in (0, 240, 479)]


@pytest.mark.parametrize("cam", [False, True], ids=["body", "camera"])
def test_config1_solved_frames_and_rows(config1_solved, cam):
    """Case 2: `config1` seed 1000, solved (P = 211): every frame time and the row times of rows 0, 240, 479 -- 44 queries in one call, far
    past what 64 selected unknowns reach (two and a half frames); the body pose and the window's camera extrinsic."""
    s, w, ref = config1_solved
    assert w.P == 211 and w.F == 11
    times = config1_times(w)
    assert len(times) == 44 and w.ld != 0.0
    ext = (w.q_CI, w.p_CI) if cam else (None, None)
    cov, st = s.pose_covariance(0, times, *ext)
    assert not st.any(), st
    e, tol, g = check(w, ref, times, cov, st, ext, "config1 solved, " + ("camera" if cam else "body"))
    print(f"config1 solved ({'camera' if cam else 'body'}): worst error {e:.3g} at bound {tol:.3g} (g {g:.3g})")


def test_constant_knots(cv):
    """Case 3: `tiny` with fixed_upto = 3: (0, 0) depends on constant knots alone -- the exact zero matrix, status 0; at (1, 0.5) only knot 4
    contributes and the result equals the reference."""
    import posecov_helpers as ph
    w = cv.synth.make_window("tiny", seed=7)
    w.fixed_upto = 3
    w.normalize()
    times = [ph.time_of(w, 0, 0.0), ph.time_of(w, 1, 0.5)]
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = device_reference(s, 0, w)
        cov, st = s.pose_covariance(0, times)
        covc, stc = s.pose_covariance(0, times, w.q_CI, w.p_CI)
    assert st.tolist() == [0, 0] and stc.tolist() == [0, 0]
    assert not cov[0].any() and not covc[0].any()
    assert (np.diag(cov[1]) > 0).all()
    check(w, ref, times, cov, st, (None, None), "tiny, constants")
    check(w, ref, times, covc, stc, (w.q_CI, w.p_CI), "tiny, constants, camera")


def mixed_queries(ws):
    """Three queries per window of the mixed batch, interleaved across the windows: (win, t_ns)."""
    import posecov_helpers as ph
    per = [[ph.time_of(w, 1, 0.3), ph.time_of(w, w.K // 2, 0.0), ph.time_of(w, w.K - 5, 0.75)] for w in ws]
    win = [i for j in range(3) for i in range(len(ws))]
    t = [per[i][j] for j in range(3) for i in range(len(ws))]
    return np.array(win, np.int32), np.array(t, np.int64)


@pytest.fixture(scope="module")
def mixed(cv):
    """The four windows of test_gpu_covariance's mixed batch (`tiny`, `config1`, the F = 16 window on the envelope panel path, the IMU-only
    predict window with L = 0), order-fixed linearisation; the queries, the device references and the plain call's outputs -- computed once."""
    from test_gpu_covariance import DET, mixed_batch
    ws, _ = mixed_batch(cv)
    win, t = mixed_queries(ws)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        refs = [device_reference(s, i, w) for i, w in enumerate(ws)]
        out = s.pose_covariance_batch(win, t)
    return ws, win, t, refs, out


def test_mixed_batch_against_reference(mixed):
    """Case 4: one call over the four windows, every query at the bound."""
    ws, win, t, refs, (cov, st) = mixed
    for i, w in enumerate(ws):
        idx = np.nonzero(win == i)[0]
        check(w, refs[i], [int(x) for x in t[idx]], cov[idx], st[idx], (None, None), f"mixed window {i} (P {w.P})")


def test_mixed_batch_bits(cv, mixed):
    """Case 4: the bits of a query depend on its window and time alone: the single-window entry, a second call, the reversed order, and calls
    with other counts per window (other tile partners) give the batch call's bits."""
    ws, win, t, _, out = mixed
    with cv.Solver(**qh.DET) as s:
        s.set_windows([w.copy() for w in ws])
        qh.check_batch_bits(s.pose_covariance, s.pose_covariance_batch, win, (t,), out, len(ws))


def test_cross_check_against_the_selected_block(config1_solved):
    """Case 5: for one `config1` query, J_np Sigma_24 J_np^T with Sigma_24 = ctvio_covariance of its 24 unknowns agrees with the new entry."""
    import cov_helpers as ch
    import posecov_helpers as ph
    s, w, ref = config1_solved
    t = ph.time_of(w, w.K // 2, 0.37)
    jac = ph.pose_jacobian(w, t)
    sel = list(range(6 * jac.s, 6 * jac.s + 24))
    cov, st = s.pose_covariance(0, [t])
    blk, _, sing = s.covariance(0, sel)
    assert st[0] == 0 and sing == 0
    via = jac.J[:, sel] @ blk @ jac.J[:, sel].T
    tol = ch.bound(ref.kappa) * ph.amplification(jac.J, ref.cov_full)
    e = ch.cov_metric(cov[0], via)
    print(f"pose entry vs J Sigma_24 J^T: {e:.3g} at bound {tol:.3g}")
    assert tol < 1e-4 and e <= tol


def test_leaves_the_solve_alone(cv, mixed):
    """Case 6: state bits, graph captures and a following solve are unchanged by the call; ctvio_covariance_batch on the same handle gives
    identical bits before and after it."""
    from test_gpu_covariance import mixed_batch
    ws, win, t, _, _ = mixed
    _, sels = mixed_batch(cv)

    def calls(s, b):
        o1 = s.pose_covariance_batch(win, t)
        o2 = s.pose_covariance_batch(win, t, ws[1].q_CI, ws[1].p_CI)
        assert np.isfinite(o1[0][o1[1] == 0]).all() and np.isfinite(o2[0][o2[1] == 0]).all()
        ms, launches = s.last_timing()
        assert launches[:3].tolist() == [1, 1, 1] and ms[7] >= ms[1] > 0
    qh.check_leaves_the_solve_alone(cv, ws, calls, sels)


def test_refusals_leave_the_handle_usable(cv):
    """Case 7: CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a window id out of range, a negative n, a NULL win / t_ns / cov36 with
    n > 0, exactly one of q_SI / p_SI NULL; n == 0 is fine; the handle solves afterwards like a fresh one."""
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    t = np.array([w.t0_ns + 1], np.int64); win = np.zeros(1, np.int32); cov = np.zeros(36); st = np.zeros(1, np.int32)
    q = np.array([0.0, 0.0, 0.0, 1.0]); pp = np.zeros(3)
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        assert lib.ctvio_pose_covariance_batch(h, 1, p(win), p(t), None, None, p(cov), p(st)) == 4
        assert lib.ctvio_pose_covariance(h, 0, 1, p(t), None, None, p(cov), p(st)) == 4
        s.set_windows([w.copy()])
        bad = np.array([1], np.int32)
        assert lib.ctvio_pose_covariance_batch(h, 1, p(bad), p(t), None, None, p(cov), p(st)) == 1
        assert lib.ctvio_pose_covariance(h, 1, 1, p(t), None, None, p(cov), p(st)) == 1
        assert lib.ctvio_pose_covariance(h, -1, 1, p(t), None, None, p(cov), p(st)) == 1
        assert lib.ctvio_pose_covariance_batch(h, -1, p(win), p(t), None, None, p(cov), p(st)) == 1
        assert lib.ctvio_pose_covariance(h, 0, -1, p(t), None, None, p(cov), p(st)) == 1
        assert lib.ctvio_pose_covariance_batch(h, 1, None, p(t), None, None, p(cov), p(st)) == 1
        assert lib.ctvio_pose_covariance_batch(h, 1, p(win), None, None, None, p(cov), p(st)) == 1
        assert lib.ctvio_pose_covariance_batch(h, 1, p(win), p(t), None, None, None, p(st)) == 1
        assert lib.ctvio_pose_covariance(h, 0, 1, None, None, None, p(cov), p(st)) == 1
        assert lib.ctvio_pose_covariance(h, 0, 1, p(t), None, None, None, p(st)) == 1
        assert lib.ctvio_pose_covariance_batch(h, 1, p(win), p(t), p(q), None, p(cov), p(st)) == 1
        assert lib.ctvio_pose_covariance(h, 0, 1, p(t), None, p(pp), p(cov), p(st)) == 1
        with pytest.raises(cv.capi.CtvioError, match="invalid"):
            s.pose_covariance_batch([3], t)
        assert lib.ctvio_pose_covariance_batch(h, 0, None, None, None, None, None, None) == 0
        assert lib.ctvio_pose_covariance(h, 0, 0, None, None, None, None, None) == 0
        c0, s0 = s.pose_covariance(0, [])
        assert c0.shape == (0, 6, 6) and s0.shape == (0,)
        assert lib.ctvio_pose_covariance(h, 0, 1, p(t), p(q), p(pp), p(cov), None) == 0          # status may be NULL
        c1, s1 = s.pose_covariance(0, t)
        assert s1[0] == 0 and np.array_equal(c1[0].ravel(), cov)                                   # (identity extrinsic: the body pose's bits)
        qh.check_usable_after(cv, w, s)


def test_adaptor_pose_covariance_matches_python(cv, tmp_path):
    """Case 8: tests/pose_covariance_demo.cpp through the C++ adaptor: the body and camera pose covariances at five times equal the Python
    call on the same window at the demo's solved state, bit for bit."""
    w0 = cv.synth.make_window("config1", seed=1005)
    K, F, L = w0.K, w0.F, w0.L
    n = 5
    wa, rest = qh.run_demo(qh.build_demo("pose_covariance_demo", tmp_path), w0, tmp_path, 15, n)
    assert rest[0] == 1 and rest[1] == n
    body_cpp = rest[2:2 + 36 * n].reshape(n, 6, 6)
    rest = rest[2 + 36 * n:]
    assert rest[0] == 1 and rest[1] == n
    cam_cpp = rest[2:2 + 36 * n].reshape(n, 6, 6)
    assert rest[2 + 36 * n] == 0                      # a time outside the spline: reported, not thrown
    times = [int(w0.t0_ns + (i + 1) * (K - 4) * w0.dt_ns // (n + 1)) for i in range(n)]
    with cv.Solver() as s:
        s.set_windows([wa])
        body, st = s.pose_covariance(0, times)
        cam, stc = s.pose_covariance(0, times, wa.q_CI, wa.p_CI)
    assert not st.any() and not stc.any()
    scale = np.sqrt(np.einsum("ni,nj->nij", np.einsum("nii->ni", body), np.einsum("nii->ni", body)))
    print(f"adaptor vs Python: body {np.max(np.abs(body_cpp - body) / scale):.3g}, camera {np.max(np.abs(cam_cpp - cam)):.3g} (absolute)")
    assert np.array_equal(body_cpp, body) and np.array_equal(cam_cpp, cam)
