"""GPU (-m gpu): ctvio_landmark_points_batch / ctvio_landmark_points (csrc/kernels_cov.hpp: k_cov_point_jac, k_cov_solve tiles of kind TILE_POINT) against
the NumPy reference of tests/lmpoint_helpers.py: the joint covariance of (trajectory, inverse depths) by the Jacobi-scaled inverse of the
un-eliminated system, formed from the DEVICE's own ctvio_linearize output of the same state (as tests/test_gpu_covariance.py, and for its
reason), mapped through the NumPy Jacobian [Jp | j_rho].

Tolerance of the covariances everywhere: cov_helpers.bound(kappa_s) * g on cov_helpers.cov_metric of the 3 x 3, g = posecov_helpers.amplification
of [Jp | j_rho] over the joint covariance; every check asserts that its bound stays below 1e-4.  Points: the sensor-pose test's rtol 1e-12 and
atol 1e-11, the atol times max(1, the window's largest depth in metres) -- a rotation error acts at the lever arm of the depth."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import query_harness as qh  # noqa: E402
from query_harness import device_joint_reference as device_reference  # noqa: E402,F401

OFF = ~np.eye(3, dtype=bool)


def check(w, ref, pts, cov, st, what, only=None):
    """Every landmark of one window (w: the window at the device's state) against the reference: the status, the point, and for status 0
    the covariance at the bound, symmetric to the bit with a positive diagonal.  Returns the worst (error, bound, g)."""
    import cov_helpers as ch
    import lmpoint_helpers as lh
    assert pts.shape == (w.L, 3) and cov.shape == (w.L, 3, 3) and st.shape == (w.L,)
    atol = lh.point_atol(w)
    worst = (0.0, 0.0, 0.0)
    for l in (range(w.L) if only is None else only):
        X, xs = lh.point(w, l)
        pj = lh.point_jacobian(w, l)
        r, rs = lh.point_cov_reference(ref, pj, l)
        assert st[l] == rs, (what, l, st[l], rs)
        if rs == lh.NONE:
            assert xs == lh.NONE and np.isnan(pts[l]).all() and np.isnan(cov[l]).all(), (what, l)
            continue
        assert np.allclose(pts[l], X, rtol=1e-12, atol=atol), (what, l, pts[l], X)
        c = cov[l]
        if rs == lh.NO_INFO:
            assert np.isposinf(np.diag(c)).all() and not c[OFF].any(), (what, l)
            continue
        assert np.isfinite(c).all() and np.array_equal(c, c.T) and (np.diag(c) > 0).all(), (what, l)
        tol, g = lh.bound(ref, pj, l)
        e = ch.cov_metric(c, r)
        assert np.isfinite(ref.kappa) and tol < 1e-4, (what, l, tol)
        assert e <= tol, (what, l, e, tol)
        worst = max(worst, (e, tol, g))
    print(f"{what}: kappa_s {ref.kappa:.3g}, worst error {worst[0]:.3g} at bound {worst[1]:.3g} (g {worst[2]:.3g})")
    return worst


def test_tiny_initial_state(cv):
    """Case 1: `tiny` seed 7 at the initial state (P = 103, L = 12: tiles of 5, 5 and 2 landmarks, ld == 0): all statuses 0."""
    w = cv.synth.make_window("tiny", seed=7)
    assert (w.P, w.L) == (103, 12) and w.ld == 0.0
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = device_reference(s, 0, w)
        pts, cov, st = s.landmark_points(0)
    assert not st.any(), st
    check(w, ref, pts, cov, st, "tiny")


@pytest.fixture(scope="module")
def config1_solved(cv):
    """`config1` seed 1000 after a 15-iteration solve on an open handle: (solver, the window at the solved state, the device reference)."""
    for s, w in qh.solved_window(cv, "config1", 1000, 15):
        yield s, w, device_reference(s, 0, w)


def test_config1_solved(config1_solved):
    """Case 2: `config1` seed 1000, solved (P = 211, L = 50: ten tiles, a free line delay != 0, rows up to 845): every landmark at the bound."""
    s, w, ref = config1_solved
    assert (w.P, w.L) == (211, 50) and w.ld != 0.0 and not w.fix_ld and int(w.v_rowi.max()) > 0
    pts, cov, st = s.landmark_points(0)
    assert not st.any(), st
    e, tol, g = check(w, ref, pts, cov, st, "config1 solved")
    print(f"config1 solved: worst (error, bound, g) = ({e:.3g}, {tol:.3g}, {g:.3g})")


def test_constants(cv):
    """Case 3: `tiny` with fixed_upto = 3 and `tiny` with fix_ld = True, both against the reference; with fix_ld the covariance of a landmark
    with row_i > 0 differs from the free-ld one (far beyond the bound: the line-delay column carries its share of the variance)."""
    import cov_helpers as ch
    import lmpoint_helpers as lh
    w = cv.synth.make_window("tiny", seed=7)
    wf = w.copy(); wf.fixed_upto = 3; wf.normalize()
    wl = w.copy(); wl.fix_ld = True; wl.normalize()
    out = {}
    for name, x in (("free", w), ("fixed_upto = 3", wf), ("fix_ld", wl)):
        with cv.Solver() as s:
            s.set_windows([x.copy()])
            ref = device_reference(s, 0, x)
            out[name] = s.landmark_points(0)
        assert not out[name][2].any()
        check(x, ref, *out[name], "tiny, " + name)
    assert np.array_equal(out["free"][0], out["fix_ld"][0]) and np.array_equal(out["free"][0], out["fixed_upto = 3"][0])
    l = next(l for l in range(w.L) if lh.anchor_of(w, l)[1] > 0)
    d = ch.cov_metric(out["fix_ld"][1][l], out["free"][1][l])
    print(f"fix_ld vs free line delay, landmark {l} (row {lh.anchor_of(w, l)[1]}): {d:.3g}")
    assert d > 1e-4


def test_statuses(cv):
    """Case 4: rho = -1 on one landmark of `tiny` (the upload accepts it, as for triangulation; never solved) and one landmark whose blocks name
    two anchor observations: status 3 and NaN, the other landmarks' points unchanged to the bit against the window without the edit -- in the
    points-only call and in the covariance call.  The covariances of the others are NOT compared with the unedited window's: both edits change
    the normal equations every landmark shares (the edited landmark's own blocks), so they are checked against the reference on the edited
    window's own linearisation instead, at the bound, in both cases (rho = -1 puts the point behind its camera, a state no solve would visit,
    but its normal equations stay positive definite and the bound stays where `tiny` has it)."""
    import lmpoint_helpers as lh
    w = cv.synth.make_window("tiny", seed=7)
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        p0, _, s0 = s.landmark_points(0, cov=False)
        p0c, c0, s0c = s.landmark_points(0)
    assert not s0.any() and not s0c.any() and np.array_equal(p0, p0c)
    wr = w.copy(); wr.rho[2] = -1.0
    others = [l for l in range(w.L) if l != 2]
    with cv.Solver() as s:
        s.set_windows([wr.copy()])
        refr = device_reference(s, 0, wr)
        p1, c1, s1 = s.landmark_points(0, cov=False)
        assert c1 is None and s1[2] == lh.NONE and np.isnan(p1[2]).all()
        assert not s1[others].any() and np.array_equal(p1[others], p0[others])
        p2, c2, s2 = s.landmark_points(0)
        assert s2[2] == lh.NONE and np.isnan(p2[2]).all() and np.isnan(c2[2]).all()
        assert not s2[others].any() and np.array_equal(p2[others], p0[others])
    check(wr, refr, p2, c2, s2, "tiny, rho = -1 on landmark 2")
    wa = w.copy()
    v = np.nonzero(wa.v_lm == 6)[0]
    assert v.shape[0] >= 2
    wa.v_pi[v[-1], 0] += 1e-3
    others = [l for l in range(w.L) if l != 6]
    with cv.Solver() as s:
        s.set_windows([wa.copy()])
        ref = device_reference(s, 0, wa)
        p3, _, s3 = s.landmark_points(0, cov=False)
        p4, c4, s4 = s.landmark_points(0)
    for p, st in ((p3, s3), (p4, s4)):
        assert st[6] == lh.NONE and np.isnan(p[6]).all() and not st[others].any() and np.array_equal(p[others], p0[others])
    assert np.isnan(c4[6]).all()
    check(wa, ref, p4, c4, s4, "tiny, landmark 6 with two anchors")


def lm_slices(ws):
    cut = np.cumsum([0] + [w.L for w in ws])
    return [slice(int(a), int(b)) for a, b in zip(cut[:-1], cut[1:])]


@pytest.fixture(scope="module")
def mixed(cv):
    """The four windows of test_gpu_covariance's mixed batch (`tiny`, `config1`, the F = 16 window on the envelope panel path, the IMU-only
    predict window with L = 0), order-fixed linearisation; the device references and the batch call's outputs -- computed once."""
    from test_gpu_covariance import DET, mixed_batch
    ws, _ = mixed_batch(cv)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        refs = [device_reference(s, i, w) if w.L else None for i, w in enumerate(ws)]
        out = s.landmark_points_batch()
    return ws, refs, out


def test_mixed_batch_against_reference(mixed):
    """Case 5: one call over the four windows, every landmark at the bound; the L = 0 window contributes nothing and breaks nothing."""
    ws, refs, (pts, cov, st) = mixed
    assert ws[3].L == 0 and pts.shape[0] == sum(w.L for w in ws) == 122
    for i, (w, sl) in enumerate(zip(ws, lm_slices(ws))):
        if w.L:
            check(w, refs[i], pts[sl], cov[sl], st[sl], f"mixed window {i} (P {w.P}, L {w.L})")


def test_mixed_batch_bits(cv, mixed):
    """Case 5: the single-window entry per window and a second batch call give the batch call's bits; so does the points-only call's points."""
    from test_gpu_covariance import DET
    ws, _, (pts, cov, st) = mixed
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        for i, sl in enumerate(lm_slices(ws)):
            p1, c1, s1 = s.landmark_points(i)
            assert p1.shape == (ws[i].L, 3) and c1.shape == (ws[i].L, 3, 3)
            assert np.array_equal(p1, pts[sl]) and np.array_equal(c1, cov[sl]) and np.array_equal(s1, st[sl]), i
        p2, c2, s2 = s.landmark_points_batch()
        assert np.array_equal(p2, pts) and np.array_equal(c2, cov) and np.array_equal(s2, st)
        p3, c3, s3 = s.landmark_points_batch(cov=False)
        assert c3 is None and np.array_equal(p3, pts) and np.array_equal(s3, st)


def test_cross_check_against_the_entries_that_exist(config1_solved):
    """Case 6: landmark 0 of `config1` seed 1000: its row of W has at most 64 non-zero columns (49 in the oracle's matrix), so
    G^T Sigma_sel G + j_rho j_rho^T / Hll with Sigma_sel = ctvio_covariance over those columns plus the anchor's unknowns, W and Hll from
    ctvio_linearize and the NumPy Jacobian, agrees with the new entry at the bound; var_rho of the same call equals 1 / Hll + a^T Sigma_sel a,
    a = w / Hll, within twice bound(kappa_s) * max(1, (sum_k |a_k| sqrt(Sigma_kk))^2 / var_rho): both sides carry the device's error."""
    import cov_helpers as ch
    import lmpoint_helpers as lh
    s, w, ref = config1_solved
    l = 0
    H, W, Hll, _, _ = s.linearize(0)
    pj = lh.point_jacobian(w, l)
    nzw = np.nonzero(W[:, l])[0]
    assert 0 < nzw.shape[0] <= 64, nzw.shape
    sel = sorted(set(nzw.tolist()) | set(np.nonzero(pj.Jp.any(axis=0))[0].tolist()))
    assert len(sel) <= 64, len(sel)
    blk, var, sing = s.covariance(0, sel, rho=True)
    assert sing == 0 and np.isfinite(blk).all()
    pts, cov, st = s.landmark_points(0)
    assert st[l] == 0
    h = Hll[l]
    G = pj.Jp[:, sel].T - np.outer(W[sel, l], pj.jrho) / h
    via = G.T @ blk @ G + np.outer(pj.jrho, pj.jrho) / h
    tol, g = lh.bound(ref, pj, l)
    e = ch.cov_metric(cov[l], via)
    print(f"landmark entry vs G^T Sigma_{len(sel)} G + j j^T / Hll ({nzw.shape[0]} non-zero columns of W): {e:.3g} at bound {tol:.3g} (g {g:.3g})")
    assert tol < 1e-4 and e <= tol
    a = W[sel, l] / h
    sll = 1.0 / h + a @ blk @ a
    ga = float((np.abs(a) @ np.sqrt(np.diag(blk))) ** 2 / var[l])
    tol_r = 2 * ch.bound(ref.kappa) * max(1.0, ga)
    print(f"var_rho vs 1 / Hll + a^T Sigma a: {abs(var[l] - sll) / var[l]:.3g} at bound {tol_r:.3g}")
    assert tol_r < 1e-4 and abs(var[l] - sll) <= tol_r * var[l]


def test_leaves_the_solve_alone(cv, mixed):
    """Case 7: state bits, graph captures and a following solve are unchanged by the calls; ctvio_covariance_batch on the same handle gives
    identical bits before and after them; the timing slots of both calls; the points-only call's points have the covariance call's bits."""
    from test_gpu_covariance import mixed_batch
    ws, _, _ = mixed
    _, sels = mixed_batch(cv)

    def calls(s, b):
        p1, c1, s1 = s.landmark_points_batch()
        assert np.isfinite(c1[s1 == 0]).all() and np.isfinite(p1[s1 != 3]).all()
        ms, launches = s.last_timing()
        assert launches[:3].tolist() == [1, 1, 1] and ms[7] >= ms[1] > 0
        p2, c2, s2 = s.landmark_points_batch(cov=False)
        ms, launches = s.last_timing()
        assert launches[:3].tolist() == [1, 0, 0] and ms[7] >= ms[0] > 0
        assert c2 is None and np.array_equal(p2, p1) and np.array_equal(s2, s1)
    qh.check_leaves_the_solve_alone(cv, ws, calls, sels)


def test_refusals_leave_the_handle_usable(cv):
    """Case 8: CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a window id out of range; all-NULL outputs are fine; the handle solves
    afterwards like a fresh one."""
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    pts = np.zeros(3 * w.L); cov = np.zeros(9 * w.L); st = np.zeros(w.L, np.int32)
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        assert lib.ctvio_landmark_points_batch(h, p(pts), p(cov), p(st)) == 4
        assert lib.ctvio_landmark_points(h, 0, p(pts), p(cov), p(st)) == 4
        with pytest.raises(cv.capi.CtvioError):
            s.landmark_points_batch()
        s.set_windows([w.copy()])
        assert lib.ctvio_landmark_points(h, 1, p(pts), p(cov), p(st)) == 1
        assert lib.ctvio_landmark_points(h, -1, p(pts), p(cov), p(st)) == 1
        assert lib.ctvio_landmark_points(h, 1, None, None, None) == 1
        with pytest.raises(cv.capi.CtvioError, match="invalid"):
            s.landmark_points(3)
        assert lib.ctvio_landmark_points_batch(h, None, None, None) == 0
        assert lib.ctvio_landmark_points(h, 0, None, None, None) == 0
        assert lib.ctvio_landmark_points(h, 0, None, p(cov), None) == 0                       # the covariances alone
        assert lib.ctvio_landmark_points_batch(h, p(pts), None, p(st)) == 0                   # points only
        p1, c1, s1 = s.landmark_points(0)
        assert not s1.any() and np.array_equal(c1.ravel(), cov) and np.array_equal(p1.ravel(), pts) and not st.any()
        qh.check_usable_after(cv, w, s)


def test_adaptor_landmark_points_matches_python(cv, tmp_path):
    """Case 9: tests/landmark_points_demo.cpp through the C++ adaptor: points, covariances and statuses equal the Python call on the same window
    at the demo's solved state, bit for bit; entry i of the adaptor is the i-th landmark in the order of first appearance among the blocks."""
    w0 = cv.synth.make_window("config1", seed=1005)
    L = w0.L
    order = list(dict.fromkeys(int(l) for l in w0.v_lm))
    assert sorted(order) == list(range(L))
    wa, rest = qh.run_demo(qh.build_demo("landmark_points_demo", tmp_path), w0, tmp_path, 15)
    assert rest[0] == 1 and rest[1] == L
    pts_cpp = rest[2:2 + 3 * L].reshape(L, 3)
    cov_cpp = rest[2 + 3 * L:2 + 12 * L].reshape(L, 3, 3)
    st_cpp = rest[2 + 12 * L:2 + 13 * L]
    rest = rest[2 + 13 * L:]
    assert rest[0] == 1 and rest[1] == L
    only_cpp = rest[2:2 + 3 * L].reshape(L, 3)
    with cv.Solver() as s:
        s.set_windows([wa])
        pts, cov, st = s.landmark_points(0)
    assert not st.any() and not st_cpp.any()
    print(f"adaptor vs Python: points {np.max(np.abs(pts_cpp - pts[order])):.3g}, covariances {np.max(np.abs(cov_cpp - cov[order])):.3g} (absolute)")
    assert np.array_equal(pts_cpp, pts[order]) and np.array_equal(only_cpp, pts[order]) and np.array_equal(cov_cpp, cov[order])
