"""GPU (-m gpu): ctvio_relative_pose_batch / ctvio_relative_pose (csrc/kernels_cov.hpp: k_cov_rel_jac, k_cov_solve tiles of kind TILE_REL) against the
NumPy reference: cov_helpers.cov_reference on the DEVICE's own ctvio_linearize output of the same state with all P unknowns selected (as
tests/test_gpu_pose_covariance.py, and for its reason), mapped through the NumPy J_rel of tests/relpose_helpers.py.

Tolerance, entry by entry: |c_ab - r_ab| / sqrt(r_aa r_bb) <= 4 kappa_s 2^-53 sqrt(g_a g_b); 4 kappa_s 2^-53 is the covariance tests' own bound and
g_a = (sum_k |J_ak| sqrt(Sigma_kk))^2 / Pi_aa the amplification of row a through J_rel (an error of tol sqrt(Sigma_kk Sigma_ll) per entry of Sigma
becomes at most tol s_a s_b in Pi_ab).  Relative poses cancel between neighbouring knots, so g is larger than for absolute poses; every check
asserts that its bound stays below the cap 1e-3 for every tested query -- the errors this test exists to catch are O(1) to O(0.1): a wrong sign,
R_ab for R_ab^T, the wrong frame for dp, a missing overlap sum.

Measured on an MI355X over cases 1 to 5: worst error 1.1e-6 at its bound 1.8e-5 (`tiny`, initial state); largest bound 6.1e-4 (DESIGN.md
section 6 has every case)."""
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
EXT = (np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9]), np.array([0.05, -0.02, 0.1]))
BODY = (None, None)


def check(w, ref, pairs, ext, rel, cov, st, what, expect=None):
    """Every query of one window (w: the window at the device's state; pairs: (t_a, t_b)) against the reference: the status, the rule of that
    status, the value against the oracle's NumPy spline evaluation, and for status 0 every entry of the covariance at its bound.  Returns the
    largest (error / bound, error, bound) over the entries."""
    import cov_helpers as ch
    import relpose_helpers as rh
    from scipy.spatial.transform import Rotation as Rot
    n = len(pairs)
    assert rel.shape == (n, 7) and cov.shape == (n, 6, 6) and st.shape == (n,)
    worst = (0.0, 0.0, 0.0)
    for i, (ta, tb) in enumerate(pairs):
        jac = rh.rel_jacobian(w, ta, tb, *ext)
        r, rs = rh.rel_cov_reference(ref, jac)
        assert st[i] == rs, (what, i, ta, tb, st[i], rs)
        if expect is not None:
            assert st[i] == expect[i], (what, i, st[i], expect[i])
        c = cov[i]
        if rs == rh.OUTSIDE:
            assert np.isnan(c).all() and np.isnan(rel[i]).all(), (what, i)
            continue
        R, p = rh.rel_numpy(w, ta, tb, *ext)
        assert abs(np.linalg.norm(rel[i, 3:]) - 1.0) <= 1e-15, (what, i)
        assert np.abs(rel[i, :3] - p).max() <= 1e-12 * max(1.0, np.abs(p).max()) and (Rot.from_quat(rel[i, 3:]).inv() * R).magnitude() <= 1e-12, (what, i)
        if rs == rh.UNTOUCHED:
            assert np.isposinf(np.diag(c)).all() and not c[rh.OFF].any(), (what, i)
            continue
        assert np.isfinite(c).all() and np.array_equal(c, c.T), (what, i)
        if not r.any():                            # only constant unknowns: the exact zero matrix
            assert not c.any(), (what, i)
            continue
        assert (np.diag(c)[np.diag(r) > 0] > 0).all(), (what, i)
        g = rh.row_amplification(jac.J, ref.cov_full)
        tol = rh.entry_bounds(ch.bound(ref.kappa), g)
        e = rh.entry_errors(c, r)
        k = np.unravel_index(np.argmax(e / tol), e.shape)
        print(f"{what} query {i} (a: s {jac.a.s}, u {jac.a.u:.3g}; b: s {jac.b.s}, u {jac.b.u:.3g}): kappa_s {ref.kappa:.3g}, g <= {g.max():.3g}, "
              f"bound <= {tol.max():.3g}, worst entry {k}: error {e[k]:.3g} at bound {tol[k]:.3g}")
        assert np.isfinite(ref.kappa) and (tol < rh.CAP).all(), (what, i, float(tol.max()))
        assert (e <= tol).all(), (what, i, k, float(e[k]), float(tol[k]))
        worst = max(worst, (float(e[k] / tol[k]), float(e[k]), float(tol[k])))
    print(f"{what}: worst error / bound {worst[0]:.3g} (error {worst[1]:.3g} at bound {worst[2]:.3g})")
    return worst


def test_tiny_initial_state(cv):
    """Case 1: `tiny` seed 7 at the initial state (P = 103, knot 11 untouched): six in-range pairs (overlapping spans with u = 0 on a, adjacent
    disjoint spans, the widest with both u = 0, b before a, neighbouring segments, spans two knots apart), an untouched knot on either side,
    a time outside on either side, and the precedence of 3 over 2; the first four again with an extrinsic."""
    import relpose_helpers as rh
    w = cv.synth.make_window("tiny", seed=7)
    assert (w.K, w.P) == (12, 103)
    T = lambda s, u: rh.time_of(w, s, u)
    before, end = w.t0_ns - 1, w.t0_ns + (w.K - 3) * w.dt_ns
    pairs = [(T(0, 0.0), T(1, 0.9)), (T(1, 0.9), T(5, 0.37)), (T(0, 0.0), T(8, 0.0)), (T(7, 0.5), T(2, 0.25)), (T(3, 0.2), T(4, 0.2)),
             (T(4, 0.5), T(6, 0.5)), (T(8, 0.5), T(1, 0.9)), (T(1, 0.9), T(8, 0.5)), (before, T(1, 0.9)), (T(1, 0.9), end), (T(8, 0.5), before)]
    expect = [0, 0, 0, 0, 0, 0, 2, 2, 3, 3, 3]
    ta, tb = [a for a, _ in pairs], [b for _, b in pairs]
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = device_reference(s, 0, w)
        rel, cov, st = s.relative_pose(0, ta, tb)
        rel_e, cov_e, st_e = s.relative_pose(0, ta[:4], tb[:4], *EXT)
    assert st.tolist() == expect and st_e.tolist() == expect[:4]
    check(w, ref, pairs, BODY, rel, cov, st, "tiny", expect=expect)
    check(w, ref, pairs[:4], EXT, rel_e, cov_e, st_e, "tiny, extrinsic", expect=expect[:4])
    for i in (6, 7):
        assert np.isposinf(np.diag(cov[i])).all() and not cov[i][rh.OFF].any() and np.isfinite(rel[i]).all()
    assert np.isnan(cov[8:]).all() and np.isnan(rel[8:]).all()
    for c in cov[:6]:
        assert np.isfinite(c).all() and np.array_equal(c, c.T) and (np.diag(c) > 0).all()


@pytest.fixture(scope="module")
def config1_solved(cv):
    """`config1` seed 1000 after a 15-iteration solve on an open handle: (solver, the window at the solved state, the device reference)."""
    for s, w in qh.solved_window(cv, "config1", 1000, 15):
        yield s, w, device_reference(s, 0, w)


def test_config1_solved_frame_pairs(config1_solved):
    """Case 2: `config1` seed 1000, solved (P = 211, frames 0.1 s apart): the ten consecutive frame pairs, body and with the window's own camera
    extrinsic; (0, F - 1), (F - 1, 0) and (3, 7); the same-segment pair (5, 0.37) -> (5, 0.87), body and with the synthetic extrinsic."""
    import relpose_helpers as rh
    s, w, ref = config1_solved
    assert w.P == 211 and w.F == 11
    fr = [int(w.t0_ns + f * FRAME_DT) for f in range(w.F)]
    cons = [(fr[f], fr[f + 1]) for f in range(w.F - 1)]
    wide = [(fr[0], fr[-1]), (fr[-1], fr[0]), (fr[3], fr[7])]
    same = [(rh.time_of(w, 5, 0.37), rh.time_of(w, 5, 0.87))]
    for pairs, ext, what in ((cons + wide + same, BODY, "config1 solved"), (cons, (w.q_CI, w.p_CI), "config1 solved, camera"),
                             (same, EXT, "config1 solved, same segment, extrinsic")):
        rel, cov, st = s.relative_pose(0, [a for a, _ in pairs], [b for _, b in pairs], *ext)
        assert not st.any(), (what, st)
        check(w, ref, pairs, ext, rel, cov, st, what)


def test_constants(cv):
    """Case 3: `tiny` with fixed_upto = 3: (0, 0) -> (1, 0) depends on constant knots alone: the exact zero matrix with status 0; at (0, 0) ->
    (1, 0.5) only knot 4 contributes and the result equals the reference."""
    import relpose_helpers as rh
    w = cv.synth.make_window("tiny", seed=7)
    w.fixed_upto = 3
    w.normalize()
    pairs = [(rh.time_of(w, 0, 0.0), rh.time_of(w, 1, 0.0)), (rh.time_of(w, 0, 0.0), rh.time_of(w, 1, 0.5))]
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = device_reference(s, 0, w)
        rel, cov, st = s.relative_pose(0, [a for a, _ in pairs], [b for _, b in pairs])
    assert st.tolist() == [0, 0]
    assert not cov[0].any() and np.isfinite(rel).all()
    assert (np.diag(cov[1]) > 0).all()
    check(w, ref, pairs, BODY, rel, cov, st, "tiny, constants")


def mixed_queries(ws):
    """Three pairs per window of the mixed batch, interleaved across the windows: (win, t_a, t_b).  On the IMU-only window (knots 0..3
    constant) the first pair sees knot 4 alone on its a-side."""
    import relpose_helpers as rh
    per = [[(rh.time_of(w, 1, 0.3), rh.time_of(w, w.K // 2, 0.0)), (rh.time_of(w, w.K // 2, 0.0), rh.time_of(w, w.K // 3, 0.75)),
            (rh.time_of(w, 4, 0.5), rh.time_of(w, 6, 0.5))] for w in ws]
    win = [i for j in range(3) for i in range(len(ws))]
    ta = [per[i][j][0] for j in range(3) for i in range(len(ws))]
    tb = [per[i][j][1] for j in range(3) for i in range(len(ws))]
    return np.array(win, np.int32), np.array(ta, np.int64), np.array(tb, np.int64)


@pytest.fixture(scope="module")
def mixed(cv):
    """The four windows of test_gpu_covariance's mixed batch (`tiny`, `config1`, the F = 16 window on the envelope panel path, the IMU-only
    predict window with locked biases and L = 0), order-fixed linearisation; the queries, the device references and the plain call's outputs --
    computed once."""
    from test_gpu_covariance import DET, mixed_batch
    ws, _ = mixed_batch(cv)
    win, ta, tb = mixed_queries(ws)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        refs = [device_reference(s, i, w) for i, w in enumerate(ws)]
        out = s.relative_pose_batch(win, ta, tb)
    return ws, win, ta, tb, refs, out


def test_mixed_batch_against_reference(mixed):
    """Case 4: one call over the four windows, every query at the bound."""
    ws, win, ta, tb, refs, (rel, cov, st) = mixed
    for i, w in enumerate(ws):
        idx = np.nonzero(win == i)[0]
        pairs = [(int(a), int(b)) for a, b in zip(ta[idx], tb[idx])]
        check(w, refs[i], pairs, BODY, rel[idx], cov[idx], st[idx], f"mixed window {i} (P {w.P})", expect=[0, 0, 0])


def test_mixed_batch_bits(cv, mixed):
    """Case 4: the bits of a query depend on its window and its two times alone: the single-window entry, a second call, the reversed order, and
    calls with other counts per window (another tile partner, or none) give the batch call's bits."""
    ws, win, ta, tb, _, out = mixed
    with cv.Solver(**qh.DET) as s:
        s.set_windows([w.copy() for w in ws])
        qh.check_batch_bits(s.relative_pose, s.relative_pose_batch, win, (ta, tb), out, len(ws))


def test_cross_checks(config1_solved):
    """Case 5, on `config1` solved: J_np Sigma_n J_np^T with Sigma_n = ctvio_covariance of the pair's knot unknowns (at most 48); cov=False gives
    the same rel7 bits with one kernel; t_a == t_b gives the identity and a covariance that vanishes up to the rounding of R_a^T R_a."""
    import cov_helpers as ch
    import relpose_helpers as rh
    from scipy.spatial.transform import Rotation as Rot
    s, w, ref = config1_solved
    pairs = [(rh.time_of(w, w.K // 2, 0.37), rh.time_of(w, w.K // 2 + 2, 0.6)), (rh.time_of(w, 3, 0.2), rh.time_of(w, w.K - 5, 0.0))]
    for ext in (BODY, EXT):
        for ta, tb in pairs:
            jac = rh.rel_jacobian(w, ta, tb, *ext)
            sel = [j for k in jac.knots for j in range(6 * k, 6 * k + 6)]
            assert len(sel) <= 48
            rel, cov, st = s.relative_pose(0, [ta], [tb], *ext)
            blk, _, sing = s.covariance(0, sel)
            assert st[0] == 0 and sing == 0
            via = jac.J[:, sel] @ blk @ jac.J[:, sel].T
            tol = rh.entry_bounds(ch.bound(ref.kappa), rh.row_amplification(jac.J, ref.cov_full))
            e = rh.entry_errors(cov[0], via)
            print(f"relative entry vs J Sigma_{len(sel)} J^T: worst error / bound {(e / tol).max():.3g}, error {e.max():.3g}, bound <= {tol.max():.3g}")
            assert (tol < rh.CAP).all() and (e <= tol).all()
    fr = [int(w.t0_ns + f * FRAME_DT) for f in range(w.F)]
    ta, tb = fr[:-1] + [w.t0_ns - 1], fr[1:] + [fr[0]]
    rel, cov, st = s.relative_pose(0, ta, tb)
    relv, covv, stv = s.relative_pose(0, ta, tb, cov=False)
    assert covv is None and np.array_equal(relv, rel, equal_nan=True) and np.array_equal(stv, st) and set(stv.tolist()) <= {0, 3}
    ms, launches = s.last_timing()
    assert launches[:3].tolist() == [0, 0, 1] and ms[7] >= ms[2] > 0
    for ext in (BODY, EXT):
        ts = [rh.time_of(w, 6, 0.0), rh.time_of(w, 6, 0.4)]
        rel, cov, st = s.relative_pose(0, ts, ts, *ext)
        pc, pst = s.pose_covariance(0, ts, *ext)
        assert not st.any() and not pst.any()
        for i, t in enumerate(ts):
            _, p = rh.ph.pose_numpy(w, t, *ext)
            assert np.abs(Rot.from_quat(rel[i, 3:]).as_matrix() - np.eye(3)).max() <= 1e-15
            assert np.abs(rel[i, :3]).max() <= 1e-15 * max(1.0, np.abs(p).max())
            ratio = np.diag(cov[i]).max() / np.diag(pc[i]).max()
            print(f"t_a == t_b (u {0.4 * i:.1f}, {'extrinsic' if ext[0] is not None else 'body'}): largest diagonal / the pose's {ratio:.3g}")
            assert (np.diag(cov[i]) >= 0).all() and ratio <= 1e-24


def test_leaves_the_solve_alone(cv, mixed):
    """Case 6: state bits, graph captures and a following solve are unchanged by the call; ctvio_covariance_batch on the same handle gives
    identical bits before and after it; last_timing reports one launch of each of the three kernels."""
    from test_gpu_covariance import mixed_batch
    ws, win, ta, tb, _, _ = mixed
    _, sels = mixed_batch(cv)

    def calls(s, b):
        o1 = s.relative_pose_batch(win, ta, tb)
        assert np.isfinite(o1[1][o1[2] == 0]).all() and np.isfinite(o1[0]).all()
        ms, launches = s.last_timing()
        assert launches[:3].tolist() == [1, 1, 1] and ms[7] >= ms[1] > 0 and not ms[3:7].any()
        s.relative_pose_batch(win, ta, tb, cov=False)
    qh.check_leaves_the_solve_alone(cv, ws, calls, sels)


def test_refusals_leave_the_handle_usable(cv):
    """Case 7: CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a window id out of range, a negative n, a NULL win / t_a_ns / t_b_ns with
    n > 0, both outputs and status NULL with n > 0, exactly one of q_SI and p_SI NULL, a zero quaternion; n == 0 is fine; the handle solves
    afterwards like a fresh one."""
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    ta = np.array([w.t0_ns + 1], np.int64); tb = np.array([w.t0_ns + 3 * w.dt_ns + 5], np.int64); win = np.zeros(1, np.int32)
    x = np.zeros(7); cov = np.zeros(36); st = np.zeros(1, np.int32)
    q = np.array([0.0, 0.0, 0.0, 1.0]); q0 = np.zeros(4); t3 = np.array([0.1, 0.2, 0.3])
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        assert lib.ctvio_relative_pose_batch(h, 1, p(win), p(ta), p(tb), None, None, p(x), p(cov), p(st)) == 4
        assert lib.ctvio_relative_pose(h, 0, 1, p(ta), p(tb), None, None, p(x), p(cov), p(st)) == 4
        s.set_windows([w.copy()])
        bad = np.array([1], np.int32)
        assert lib.ctvio_relative_pose_batch(h, 1, p(bad), p(ta), p(tb), None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose(h, 1, 1, p(ta), p(tb), None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose(h, -1, 1, p(ta), p(tb), None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose_batch(h, -1, p(win), p(ta), p(tb), None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose(h, 0, -1, p(ta), p(tb), None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose_batch(h, 1, None, p(ta), p(tb), None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose_batch(h, 1, p(win), None, p(tb), None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose_batch(h, 1, p(win), p(ta), None, None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose(h, 0, 1, None, p(tb), None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose(h, 0, 1, p(ta), None, None, None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose_batch(h, 1, p(win), p(ta), p(tb), None, None, None, None, None) == 1
        assert lib.ctvio_relative_pose(h, 0, 1, p(ta), p(tb), None, None, None, None, None) == 1
        assert lib.ctvio_relative_pose(h, 0, 1, p(ta), p(tb), p(q), None, p(x), p(cov), p(st)) == 1            # one of q_SI, p_SI
        assert lib.ctvio_relative_pose(h, 0, 1, p(ta), p(tb), None, p(t3), p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose_batch(h, 1, p(win), p(ta), p(tb), p(q), None, p(x), p(cov), p(st)) == 1
        assert lib.ctvio_relative_pose(h, 0, 1, p(ta), p(tb), p(q0), p(t3), p(x), p(cov), p(st)) == 1           # a zero quaternion
        assert lib.ctvio_relative_pose(h, 0, 1, p(ta), p(tb), p(q0), p(t3), p(x), None, p(st)) == 1
        with pytest.raises(cv.capi.CtvioError, match="invalid"):
            s.relative_pose_batch([3], ta, tb)
        assert lib.ctvio_relative_pose_batch(h, 0, None, None, None, None, None, None, None, None) == 0
        assert lib.ctvio_relative_pose(h, 0, 0, None, None, None, None, None, None, None) == 0
        x0, c0, s0 = s.relative_pose(0, [], [])
        assert x0.shape == (0, 7) and c0.shape == (0, 6, 6) and s0.shape == (0,)
        x1, c1, s1 = s.relative_pose(0, ta, tb)
        assert s1[0] == 0
        assert lib.ctvio_relative_pose(h, 0, 1, p(ta), p(tb), None, None, None, p(cov), None) == 0                   # each output alone
        assert np.array_equal(cov, c1[0].ravel())
        assert lib.ctvio_relative_pose(h, 0, 1, p(ta), p(tb), None, None, p(x), None, None) == 0
        assert np.array_equal(x, x1[0])
        assert lib.ctvio_relative_pose(h, 0, 1, p(ta), p(tb), None, None, None, None, p(st)) == 0 and st[0] == 0
        qh.check_usable_after(cv, w, s)


def test_adaptor_relative_pose_matches_python(cv, tmp_path):
    """Case 8: tests/relative_pose_demo.cpp through the C++ adaptor: the increments and covariances of five pairs, body and camera, equal the
    Python call on the same window at the demo's solved state, bit for bit."""
    w0 = cv.synth.make_window("config1", seed=1005)
    K, F, L = w0.K, w0.F, w0.L
    n = 5
    wa, rest = qh.run_demo(qh.build_demo("relative_pose_demo", tmp_path), w0, tmp_path, 15, n)
    got = []
    for _ in range(2):
        assert rest[0] == 1 and rest[1] == n
        got.append((rest[2:2 + 7 * n].reshape(n, 7), rest[2 + 7 * n:2 + 43 * n].reshape(n, 6, 6)))
        rest = rest[2 + 43 * n:]
    assert rest[0] == 0                               # a time outside the spline: reported, not thrown
    times = [int(w0.t0_ns + (i + 1) * (K - 4) * w0.dt_ns // (n + 1)) for i in range(n)]
    ta, tb = times, times[1:] + times[:1]
    with cv.Solver() as s:
        s.set_windows([wa])
        body = s.relative_pose(0, ta, tb)
        cam = s.relative_pose(0, ta, tb, wa.q_CI, wa.p_CI)
    for (x_cpp, c_cpp), (x, c, st) in zip(got, (body, cam)):
        assert not st.any()
        assert np.array_equal(x_cpp, x) and np.array_equal(c_cpp, c)
