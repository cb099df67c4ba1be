"""GPU (-m gpu): ctvio_triangulate(_batch) and ctvio_shift_anchor_batch (csrc/kernels_tri.hpp) against the NumPy restatement in
tests/tri_helpers.py (poses from splines.eval_spline, depth from np.linalg.svd).

Bounds: a triangulated depth within 1e-10 relative of the SVD reference, a shifted depth within 1e-12; flags equal; init_depth exact.  The helper
refuses a fixture whose triangulated depth lies within 1e-3 of min_depth (its flag would depend on rounding).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TRI_TOL, SHIFT_TOL = 1e-10, 1e-12
STATE, INVALID = 4, 1


def three_windows(cv):
    """Three windows with different K (so that lm0 / vis0 / anc0 are non-zero), at their initial guess; the third with a free line delay
    of 3.0e-5, so that the row times matter."""
    a = cv.synth.make_window("tiny", seed=7)
    b = cv.synth.make_window("tiny", seed=8, F=6)
    c = cv.synth.make_window("config3", seed=1001, L=24, M=400)
    c.ld = 3.0e-5
    assert not c.fix_ld and len({a.K, b.K, c.K}) == 3
    return [a, b, c]


@pytest.fixture(scope="module")
def batch(cv):
    return three_windows(cv)


@pytest.fixture(scope="module")
def batch_ref(batch):
    """(row_times) -> per window (depth, flag, raw) of the SVD reference at the initial guess, every landmark."""
    import tri_helpers as th
    return {rt: [th.triangulate_ref(w, row_times=rt) for w in batch] for rt in (1, 0)}


def compare(depth, flag, ref, what):
    """One window against its reference -> the largest relative error over the flag-1 landmarks."""
    import tri_helpers as th
    rd, rf, _ = ref
    assert np.array_equal(flag, rf), (what, flag, rf)
    ok = rf == th.OK
    err = float(th.rel_err(depth[ok], rd[ok]).max()) if ok.any() else 0.0
    print(f"{what}: flags {np.bincount(rf, minlength=4).tolist()}, max rel err {err:.3g}")
    assert err <= TRI_TOL, (what, err)
    assert np.array_equal(depth[rf != th.OK], rd[rf != th.OK]), what     # init_depth / 1 / rho: exact
    return err


@pytest.mark.parametrize("row_times", [1, 0])
def test_three_window_batch_matches_the_reference(cv, batch, batch_ref, row_times):
    """Case 4.  Largest relative error of a flag-1 depth observed on the MI355X: 1.26e-12 (row times) and 1.26e-12 (frame times: two of the three
    windows have a zero line delay at their initial guess), bound 1e-10."""
    import tri_helpers as th
    with cv.Solver() as s:
        s.set_windows([w.copy() for w in batch])
        depth, flag = s.triangulate_batch(row_times=row_times, only_unset=0, apply=0)
    for i in range(3):
        compare(depth[i], flag[i], batch_ref[row_times][i], f"window {i} row_times {row_times}")
    f0 = batch_ref[1][0][1]
    if row_times == 1:     # tiny / 7 at the initial guess: the reference itself sends 4 of 12 landmarks to init_depth
        assert (f0 == th.INIT).sum() == 4 and (depth[0][f0 == th.INIT] == 5.0).all()


def edge_window(cv):
    """`tiny` seed 7 with four hand-made landmarks: 4 with exactly 64 blocks (its own blocks repeated at their frame times with jittered rows
    and points), 6 with one block, 2 with none, 3 with blocks that name two anchor observations.  (4 and 6 triangulate to positive depths.)"""
    w = cv.synth.make_window("tiny", seed=7)
    rng = np.random.default_rng(3)
    keep = np.ones(w.V, bool)
    i1 = np.flatnonzero(w.v_lm == 6); keep[i1[1:]] = False
    keep[w.v_lm == 2] = False
    i3 = np.flatnonzero(w.v_lm == 3)
    assert i1.size >= 2 and i3.size >= 2
    rowi = w.v_rowi.copy(); rowi[i3[-1]] += 1
    i0 = np.flatnonzero(w.v_lm == 4)
    src = i0[np.arange(64 - i0.size) % i0.size]
    cat = lambda a, b: np.concatenate([a[keep], b])
    w.v_pj = cat(w.v_pj, w.v_pj[src] + rng.uniform(-1e-3, 1e-3, (src.size, 2)))
    w.v_rowj = cat(w.v_rowj, w.v_rowj[src] + rng.integers(-3, 4, src.size).astype(np.int32))
    w.v_lm, w.v_ti, w.v_tj, w.v_rowi, w.v_pi = cat(w.v_lm, w.v_lm[src]), cat(w.v_ti, w.v_ti[src]), cat(w.v_tj, w.v_tj[src]), cat(rowi, rowi[src]), cat(w.v_pi, w.v_pi[src])
    w.normalize()
    assert (w.v_lm == 4).sum() == 64 and (w.v_lm == 6).sum() == 1 and (w.v_lm == 2).sum() == 0
    return w


@pytest.mark.parametrize("row_times", [1, 0])
def test_edge_landmarks(cv, row_times):
    """Case 5: 64 blocks (lanes 0..63 and the anchor), one block (A is 4 x 4), no block and two anchors (flag 3, depth 1 / rho).  Largest
    relative error observed on the MI355X: 7.4e-14."""
    import tri_helpers as th
    w = edge_window(cv)
    ref = th.triangulate_ref(w, row_times=row_times)
    assert ref[1][4] == th.OK and ref[1][6] == th.OK and ref[1][2] == th.NONE and ref[1][3] == th.NONE
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        depth, flag = s.triangulate(0, row_times=row_times, only_unset=0, apply=1)
        after = s.get_state(0)
    compare(depth, flag, ref, f"edge window row_times {row_times}")
    assert np.array_equal(depth[2:4], 1.0 / w.rho[2:4]) and np.array_equal(after.rho[2:4], w.rho[2:4])     # never applied


def test_only_unset_apply_and_solve(cv, oracle, batch):
    """Case 6: a third of the landmarks uploaded with rho = -1; only they are triangulated and written; the solve from there matches the oracle's."""
    import tri_helpers as th
    ws = [w.copy() for w in batch]
    for w in ws:
        w.rho[::3] = -1.0
    with cv.Solver() as s:
        up = [w.copy() for w in ws]
        s.set_windows(up)
        before = s.get_batch_state()
        d0, f0 = s.triangulate_batch(only_unset=1, apply=0)
        assert all(np.array_equal(x, y) for x, y in zip(before, s.get_batch_state()))           # apply = 0: bitwise unchanged
        depth, flag = s.triangulate_batch(only_unset=1, apply=1)
        assert all(np.array_equal(x, y) for x, y in zip(d0, depth)) and all(np.array_equal(x, y) for x, y in zip(f0, flag))
        refs = []
        for i, w in enumerate(ws):
            ref = th.triangulate_ref(w, row_times=1, only_unset=1)
            compare(depth[i], flag[i], ref, f"window {i} only_unset")
            unset = np.arange(w.L) % 3 == 0
            assert np.all(flag[i][~unset] == th.SKIPPED) and np.all(flag[i][unset] != th.SKIPPED)
            st = s.get_state(i)
            assert np.array_equal(st.rho[~unset], w.rho[~unset])                                 # the others keep their bits
            assert np.array_equal(st.rho[unset], 1.0 / depth[i][unset])                          # exactly 1 / depth
            wo = w.copy()
            wo.rho[unset] = 1.0 / ref[0][unset]
            refs.append(wo)
        s.solve(15)
    for i, wo in enumerate(refs):
        oracle.OracleWindow(wo).solve(15)
        err = cv.rel_state_error(up[i], wo)["state"]
        print(f"window {i}: solve after apply vs the oracle {err:.3g}")
        assert err < 1e-4, (i, err)


def test_deterministic_and_entry_equivalence(cv, batch):
    """Case 7: two batch calls give equal bits; ctvio_triangulate(id) gives the bits of the batch slice."""
    with cv.Solver() as s:
        s.set_windows([w.copy() for w in batch])
        for rt in (1, 0):
            d1, f1 = s.triangulate_batch(row_times=rt, only_unset=0, apply=0)
            d2, f2 = s.triangulate_batch(row_times=rt, only_unset=0, apply=0)
            for i in range(3):
                ds, fs = s.triangulate(i, row_times=rt, only_unset=0, apply=0)
                assert np.array_equal(d1[i].view(np.int64), d2[i].view(np.int64)) and np.array_equal(f1[i], f2[i])
                assert np.array_equal(d1[i].view(np.int64), ds.view(np.int64)) and np.array_equal(f1[i], fs)
        ms, n = s.last_timing()
        assert ms[0] > 0 and ms[7] >= ms[0] and not ms[1:7].any() and n[0] == 1


def test_uses_the_current_state(cv):
    """Case 8: after a solve the depths are those of the helper on get_state's knots and line delay, not of the uploaded ones."""
    import tri_helpers as th
    w = cv.synth.make_window("tiny", seed=7)
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        s.solve(15, writeback=False)
        now = s.get_state(0)
        depth, flag = s.triangulate(0, only_unset=0, apply=0)
    assert now.ld != w.ld and not np.array_equal(now.quat, w.quat)
    compare(depth, flag, th.triangulate_ref(now, row_times=1), "tiny after the solve")
    old = th.triangulate_ref(w, row_times=1)
    assert not np.array_equal(old[1], flag) or th.rel_err(depth, old[0]).max() > 1e-6


def test_anchor_shift(cv, batch):
    """Case 9: every landmark anchored in frame 0 moved to its first block's observation, after a solve, both time modes; rho <= 0 gives
    flag 3, a point behind the new camera flag 2; the state is never written.  Largest relative error observed on the MI355X: 1.5e-15."""
    import tri_helpers as th
    ws = [w.copy() for w in batch]
    with cv.Solver() as s:
        s.set_windows(ws)
        s.solve(15)                                        # (writes the solved state back into ws)
        win, lm, t_new, row_new = [], [], [], []
        for i, w in enumerate(ws):
            for l in range(w.L):
                idx, one = th.landmark_observations(w, l)
                if one and w.v_ti[idx[0]] == w.t0_ns:
                    win.append(i); lm.append(l); t_new.append(w.v_tj[idx[0]]); row_new.append(w.v_rowj[idx[0]])
        win, lm, t_new, row_new = np.array(win), np.array(lm), np.array(t_new), np.array(row_new)
        assert all((win == i).sum() >= 2 for i in range(3))
        before = s.get_batch_state()
        worst = 0.0
        for rt in (1, 0):
            d, f = s.shift_anchor(win, lm, t_new, row_new if rt else None, row_times=rt)
            for i, w in enumerate(ws):
                m = win == i
                rd, rf, _ = th.shift_ref(w, lm[m], t_new[m], row_new[m] if rt else None, rt)
                assert np.array_equal(f[m], rf) and np.all(rf == th.OK)
                worst = max(worst, float(th.rel_err(d[m], rd).max()))
        print(f"anchor shift: {win.size} queries, max rel err {worst:.3g}")
        assert worst <= SHIFT_TOL
        # a landmark without a depth, and one hand-placed 1e-6 in front of its old camera where the new camera looks away from it
        w0 = ws[0].copy()
        q = np.flatnonzero(win == 0)
        trial = w0.copy(); trial.rho[:] = 1e6
        behind = next(k for k in q if th.shift_ref(trial, lm[k:k + 1], t_new[k:k + 1], row_new[k:k + 1], 1)[1][0] == th.INIT)
        unset = next(k for k in q if k != behind)
        w0.rho[lm[behind]] = 1e6; w0.rho[lm[unset]] = -1.0
        s.set_state(0, w0)
        mid = s.get_batch_state()
        d, f = s.shift_anchor(win, lm, t_new, row_new)
        rd, rf, _ = th.shift_ref(w0, lm[q], t_new[q], row_new[q], 1)
        assert np.array_equal(f[q], rf) and th.rel_err(d[q][rf == th.OK], rd[rf == th.OK]).max() <= SHIFT_TOL and f[behind] == th.INIT and d[behind] == 5.0 and f[unset] == th.NONE and np.isnan(d[unset])
        assert all(np.array_equal(x, y) for x, y in zip(mid, s.get_batch_state()))
        s.set_state(0, ws[0])
        assert all(np.array_equal(x, y) for x, y in zip(before, s.get_batch_state()))


def test_error_paths(cv, oracle_solved):
    """Case 10: CTVIO_ERR_STATE before the upload, CTVIO_ERR_INVALID for a bad id / window / landmark / NULL options; the handle still solves like a fresh one."""
    import ctypes as C
    w = cv.synth.make_window("tiny", seed=7)
    o = cv.capi.TriangulateOptions()
    one = np.zeros(1, np.int32); t = np.zeros(1, np.int64); d = np.zeros(w.L); f = np.zeros(w.L, np.int32)
    p = cv.capi._p
    with cv.Solver() as s:
        lib = s._lib
        lib.ctvio_default_triangulate_options(C.byref(o))
        o.apply = 0
        shift = lambda wi, li, opt=C.byref(o): lib.ctvio_shift_anchor_batch(s._h, opt, 1, p(np.array([wi], np.int32)), p(np.array([li], np.int32)), p(t), p(one), p(d), p(f))
        assert lib.ctvio_triangulate_batch(s._h, C.byref(o), p(d), p(f)) == STATE
        assert lib.ctvio_triangulate(s._h, 0, C.byref(o), p(d), p(f)) == STATE
        assert shift(0, 0) == STATE
        b = [w.copy()]
        s.set_windows(b)
        assert lib.ctvio_triangulate(s._h, 1, C.byref(o), p(d), p(f)) == INVALID
        assert lib.ctvio_triangulate(s._h, -1, C.byref(o), p(d), p(f)) == INVALID
        assert lib.ctvio_triangulate(s._h, 0, None, p(d), p(f)) == INVALID
        assert lib.ctvio_triangulate_batch(s._h, None, p(d), p(f)) == INVALID
        assert shift(1, 0) == INVALID and shift(-1, 0) == INVALID and shift(0, w.L) == INVALID and shift(0, -1) == INVALID
        assert shift(0, 0, None) == INVALID
        assert lib.ctvio_triangulate(s._h, 0, C.byref(o), None, None) == 0 and shift(0, 0) == 0
        captures = s.graph_captures
        sm = s.solve(15)[0]
        assert s.graph_captures <= captures + 1
    ref, so = oracle_solved("tiny", 7)
    with cv.Solver() as s2:
        b2 = [w.copy()]
        s2.set_windows(b2)
        sm2 = s2.solve(15)[0]
    assert sm == sm2 and np.array_equal(b[0].state_vector(), b2[0].state_vector())
    assert cv.rel_state_error(b[0], ref)["state"] < 1e-6
