"""GPU (-m gpu): ctvio_imu_predict_batch / ctvio_imu_predict (csrc/kernels_prop.hpp: k_imu_propagate after k_cov_nav_jac and k_cov_solve's tiles
of kind TILE_NAV) against the NumPy recurrence of tests/imuprop_helpers.py STARTED FROM THE DEVICE'S OWN ctvio_nav_state output for (window, imu_t[0],
frame): nav_state is held to the oracle by tests/test_gpu_nav_state.py, so this isolates the new kernel.

The samples are drawn here (seeded default_rng): 200 Hz from the window's newest frame time with one 7 ms gap, gyro N(0, 0.5), acc R_0^T g +
N(0, 1).

Tolerance, entry by entry: |c_ab - r_ab| / sqrt(r_aa r_bb) <= 64 max(d, 15 m 2^-53), d the same metric between the helper in float64 and in
np.longdouble on those inputs (the recurrence's own rounding), 64 for the device's other summation order and FMA contraction.  Every check
asserts that this bound is below 1e-10 and prints it: a wrong block is at least 1e-5 (J = I alone is 2.5e-3 at these rates).  States:
positions and velocities to 1e-12 max(1, |x|), rotations to 1e-12 rad, biases equal to the bit -- the tolerances of test_gpu_nav_state.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import query_harness as qh  # noqa: E402

FRAME_DT = 100_000_000      # synth.py: frame_dt_ns of every configuration used here
OFF = ~np.eye(15, dtype=bool)


def newest(w):
    return int(w.t0_ns + (w.F - 1) * FRAME_DT)


def draw(w, m, seed, t_start=None, R0=None):
    """m samples at 200 Hz from t_start (default: the newest frame time) with one 7 ms gap; gyro N(0, 0.5), acc R0^T g + N(0, 1) (R0 default I)."""
    rng = np.random.default_rng(seed)
    step = np.full(max(m - 1, 0), 5_000_000, np.int64)
    if m > 2:
        step[(m - 1) // 2] = 7_000_000
    t = (newest(w) if t_start is None else int(t_start)) + np.concatenate([[0], np.cumsum(step)]).astype(np.int64)
    gyro = rng.normal(0, 0.5, (m, 3))
    g = np.asarray(w.gravity, float)
    acc = (g if R0 is None else R0.T @ g) + rng.normal(0, 1.0, (m, 3))
    return t, gyro, acc


def unpack(x16):
    from scipy.spatial.transform import Rotation as Rot
    return Rot.from_quat(x16[3:7]).as_matrix(), x16[0:3].copy(), x16[7:10].copy(), x16[10:13].copy(), x16[13:16].copy()


def check_query(s, wid, w, frame, t, gyro, acc, noise, state, cov, what):
    """One ok query against the helper's recurrence from the device's own nav_state at (wid, t[0], frame).  Returns (worst error, bound)."""
    import imuprop_helpers as ih
    from scipy.spatial.transform import Rotation as Rot
    m = len(t)
    x0, P0, st0 = s.nav_state(wid, [int(t[0])], None if frame is None else [frame])
    assert st0[0] == 0 and state.shape == (m, 16) and cov.shape == (m, 15, 15), what
    assert np.array_equal(state[0], x0[0]) and np.array_equal(cov[0], P0[0]), what          # sample 0: nav_state's bits
    nz = ih.DEFAULT_NOISE if noise is None else noise
    xs, Ps = ih.propagate(unpack(x0[0]), P0[0], t, gyro, acc, w.gravity, nz)
    _, Pl = ih.propagate(unpack(x0[0]), P0[0], t, gyro, acc, w.gravity, nz, dtype=np.longdouble)
    d = max(ih.entry_metric(a, b) for a, b in zip(Ps, Pl))
    bound = 64 * max(d, 15 * m * 2.0 ** -53)
    worst = 0.0
    for j in range(m):
        R, p, v, bg, ba = xs[j]
        x = state[j]
        assert np.abs(x[0:3] - p).max() <= 1e-12 * max(1.0, np.abs(p).max()) and np.abs(x[7:10] - v).max() <= 1e-12 * max(1.0, np.abs(v).max()), (what, j)
        assert (Rot.from_quat(x[3:7]).inv() * Rot.from_matrix(R)).magnitude() <= 1e-12 and np.array_equal(x[10:16], x0[0][10:16]), (what, j)
        c = cov[j]
        assert np.isfinite(c).all() and np.array_equal(c, c.T), (what, j)
        worst = max(worst, ih.entry_metric(c, Pl[j]))
    print(f"{what}: m {m}, float64 vs longdouble {d:.3g}, bound {bound:.3g}, worst entry error {worst:.3g}")
    assert bound < 1e-10, (what, bound)
    assert worst <= bound, (what, worst, bound)
    return worst, bound


def test_tiny_initial_state(cv):
    """Case 1: `tiny` seed 7 at the initial state, m = 1, 2, 21 in one batch call with frames 0, F // 2 and the newest: m = 1 returns nav_state's
    bits, every sample of the others is at the bound, frame None equals F - 1, last_only returns the bits of the last samples."""
    w = cv.synth.make_window("tiny", seed=7)
    ms = [1, 2, 21]
    frames = [0, w.F // 2, w.F - 1]
    sam = [draw(w, m, 70 + i) for i, m in enumerate(ms)]
    t, gyro, acc = (np.concatenate([x[k] for x in sam]) for k in range(3))
    off = np.concatenate([[0], np.cumsum(ms)])
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        state, cov, st = s.imu_predict_batch([0, 0, 0], frames, ms, t, gyro, acc)
        assert st.tolist() == [0, 0, 0] and state.shape == (24, 16) and cov.shape == (24, 15, 15)
        for i, m in enumerate(ms):
            sl = slice(off[i], off[i + 1])
            check_query(s, 0, w, frames[i], *sam[i], None, state[sl], cov[sl], f"tiny, m {m}, frame {frames[i]}")
        x1, c1, s1 = s.nav_state(0, [int(sam[0][0][0])], [0])
        assert np.array_equal(state[0], x1[0]) and np.array_equal(cov[0], c1[0])
        ls, lc, lst = s.imu_predict_batch([0, 0, 0], frames, ms, t, gyro, acc, last_only=True)
        assert ls.shape == (3, 16) and np.array_equal(ls, state[off[1:] - 1]) and np.array_equal(lc, cov[off[1:] - 1]) and np.array_equal(lst, st)
        ns, nc, nst = s.imu_predict(0, None, *sam[2])
        assert np.array_equal(ns, state[off[2]:]) and np.array_equal(nc, cov[off[2]:]) and nst.tolist() == [0]
        ns, nc, nst = s.imu_predict_batch([0], None, [21], *sam[2])
        assert np.array_equal(ns, state[off[2]:]) and np.array_equal(nc, cov[off[2]:]) and nst.tolist() == [0]


def test_config1_solved_newest_frame(cv):
    """Case 2, the reference's use: `config1` seed 1000 after a 15-iteration solve, 21 samples from the newest frame time with the newest
    biases: samples at the bound, covariances symmetric to the bit with positive diagonals."""
    w = cv.synth.make_window("config1", seed=1000)
    with cv.Solver() as s:
        b = [w.copy()]
        s.set_windows(b)
        s.solve(15)
        x0, _, _ = s.nav_state(0, [newest(w)], cov=False)
        t, gyro, acc = draw(w, 21, 1000, R0=unpack(x0[0])[0])
        state, cov, st = s.imu_predict(0, None, t, gyro, acc)
        assert st.tolist() == [0]
        assert np.array_equal(state[:, 10:], np.tile(b[0].bias[w.F - 1], (21, 1)))
        for c in cov:
            assert np.array_equal(c, c.T) and (np.diag(c) > 0).all()
        assert (np.diag(cov[-1])[:9] > np.diag(cov[0])[:9]).all()          # 100 ms of dead reckoning: pose and velocity less certain
        e, bound = check_query(s, 0, b[0], None, t, gyro, acc, None, state, cov, "config1 solved, newest frame")
    print(f"config1 solved: worst error {e:.3g} at bound {bound:.3g}")


def test_constants(cv):
    """Case 3: `tiny` with fixed_upto = 3 and lock_bg = 1, start at segment 0, u = 0, where P_0 has the ba block alone.  With gyr_w = 0 the bg
    rows and columns hold no non-zero at any sample; the ba block feeds p and v: those diagonals are positive from sample 1 on."""
    import imuprop_helpers as ih
    w = cv.synth.make_window("tiny", seed=7)
    w.fixed_upto = 3; w.lock_bg = 1
    w.normalize()
    noise = (ih.DEFAULT_NOISE[0], ih.DEFAULT_NOISE[1], 0.0, ih.DEFAULT_NOISE[3])
    t, gyro, acc = draw(w, 21, 73, t_start=w.t0_ns)
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        state, cov, st = s.imu_predict(0, 1, t, gyro, acc, noise=noise)
        assert st.tolist() == [0]
        assert not cov[0][:12].any() and not cov[0][:, :12].any() and (np.diag(cov[0])[12:] > 0).all()
        assert not cov[:, 9:12, :].any() and not cov[:, :, 9:12].any()
        for c in cov[1:]:
            d = np.diag(c)
            assert (d[:9] > 0).all() and (d[12:] > 0).all()
        check_query(s, 0, w, 1, t, gyro, acc, noise, state, cov, "tiny, constants")


def test_statuses(cv):
    """Case 4: a start before t0 and at the spline's end give status 3, all NaN; a start that depends on the untouched last knot, the (8, 0.5)
    query of test_gpu_nav_state.test_tiny_initial_state, gives status 2: states finite for every sample, +inf diagonal and zero elsewhere for
    every sample; an ok query beside them is untouched by their company."""
    import navstate_helpers as nh
    w = cv.synth.make_window("tiny", seed=7)
    starts = [w.t0_ns - 1, w.t0_ns + (w.K - 3) * w.dt_ns, nh.time_of(w, 8, 0.5), nh.time_of(w, 5, 0.37)]
    ms = [3, 2, 6, 4]
    sam = [draw(w, m, 80 + i, t_start=t0) for i, (m, t0) in enumerate(zip(ms, starts))]
    t, gyro, acc = (np.concatenate([x[k] for x in sam]) for k in range(3))
    off = np.concatenate([[0], np.cumsum(ms)])
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        state, cov, st = s.imu_predict_batch([0] * 4, None, ms, t, gyro, acc)
        assert st.tolist() == [3, 3, 2, 0]
        assert np.isnan(state[:off[2]]).all() and np.isnan(cov[:off[2]]).all()
        u = slice(off[2], off[3])
        assert np.isfinite(state[u]).all() and np.abs(state[u][-1, :3] - state[u][0, :3]).max() > 0
        for c in cov[u]:
            assert np.isposinf(np.diag(c)).all() and not c[OFF].any()
        xv, _, stv = s.imu_predict_batch([0] * 4, None, ms, t, gyro, acc, cov=False)
        assert stv.tolist() == [3, 3, 0, 0] and np.array_equal(xv, state, equal_nan=True)
        ls, lc, lst = s.imu_predict_batch([0] * 4, None, ms, t, gyro, acc, last_only=True)
        assert np.array_equal(ls, state[off[1:] - 1], equal_nan=True) and np.array_equal(lc, cov[off[1:] - 1], equal_nan=True) and np.array_equal(lst, st)
        check_query(s, 0, w, None, *sam[3], None, state[off[3]:], cov[off[3]:], "tiny, beside refused starts")


def mixed_queries(ws):
    """Three queries per window of the mixed batch, of 1, 5 and 21 samples, interleaved across the windows, from the newest frame time with the
    bias states 0, F // 2 and F - 1: (win, frame, m, samples per query)."""
    win, fr, ms, sam = [], [], [], []
    for j, m in enumerate((1, 5, 21)):
        for i, w in enumerate(ws):
            win.append(i); fr.append([0, w.F // 2, w.F - 1][j]); ms.append(m)
            sam.append(draw(w, m, 500 + 10 * i + j))
    return win, fr, ms, sam


def cat(sam, idx):
    return tuple(np.concatenate([sam[i][k] for i in idx]) for k in range(3))


def test_mixed_batch_bits(cv):
    """Case 5, on the four-window mixed batch with the order-fixed linearisation: the bits of a query depend on its window, frame, samples and
    sigmas alone -- batch against single entry, a second call, the reversed order, subsets, queries of 1 / 5 / 21 samples sharing a call and
    a wave, last_only; cov=False gives the same state bits."""
    from test_gpu_covariance import DET, mixed_batch
    ws, _ = mixed_batch(cv)
    win, fr, ms, sam = mixed_queries(ws)
    n = len(win)
    off = np.concatenate([[0], np.cumsum(ms)])
    same = lambda a, b: all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        out = s.imu_predict_batch(win, fr, ms, *cat(sam, range(n)))
        assert not out[2].any() and np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
        per = lambda o, i: (o[0][off[i]:off[i + 1]], o[1][off[i]:off[i + 1]], o[2][i:i + 1])
        for i in range(n):
            assert same(s.imu_predict(win[i], fr[i], *sam[i]), per(out, i)), i
        assert same(s.imu_predict_batch(win, fr, ms, *cat(sam, range(n))), out)
        order = list(range(n))[::-1]
        rev = s.imu_predict_batch([win[i] for i in order], [fr[i] for i in order], [ms[i] for i in order], *cat(sam, order))
        o2 = np.concatenate([[0], np.cumsum([ms[i] for i in order])])
        for k, i in enumerate(order):
            assert same((rev[0][o2[k]:o2[k + 1]], rev[1][o2[k]:o2[k + 1]], rev[2][k:k + 1]), per(out, i)), i
        for keep in (list(range(4, n)), [0, 5, 10], [8, 9, 10, 11, 3], [11]):
            sub = s.imu_predict_batch([win[i] for i in keep], [fr[i] for i in keep], [ms[i] for i in keep], *cat(sam, keep))
            o3 = np.concatenate([[0], np.cumsum([ms[i] for i in keep])])
            for k, i in enumerate(keep):
                assert same((sub[0][o3[k]:o3[k + 1]], sub[1][o3[k]:o3[k + 1]], sub[2][k:k + 1]), per(out, i)), (keep, i)
        last = s.imu_predict_batch(win, fr, ms, *cat(sam, range(n)), last_only=True)
        assert same(last, (out[0][off[1:] - 1], out[1][off[1:] - 1], out[2]))
        xv, cv_, stv = s.imu_predict_batch(win, fr, ms, *cat(sam, range(n)), cov=False)
        assert cv_ is None and np.array_equal(xv, out[0]) and np.array_equal(stv, out[2])
        ms8, launches = s.last_timing()
        assert launches[:4].tolist() == [0, 0, 1, 1] and ms8[7] >= ms8[3] > 0 and ms8[2] > 0 and not ms8[:2].any() and not ms8[4:7].any()
        # the 21-sample query of every window at the bound (the windows beyond `tiny` and `config1`: P = 301 and the IMU-only one)
        for i in (10, 11):
            check_query(s, win[i], ws[win[i]], fr[i], *sam[i], None, *per(out, i)[:2], f"mixed window {win[i]} (P {ws[win[i]].P})")


def test_leaves_the_solve_alone(cv):
    """Case 6: state bits, graph captures and a following solve are unchanged by the call; ctvio_covariance_batch on the same handle gives
    identical bits before and after it; last_timing reports one launch in each of the slots 0..3."""
    from test_gpu_covariance import mixed_batch
    ws, sels = mixed_batch(cv)
    win, fr, ms, sam = mixed_queries(ws)
    args = (win, fr, ms) + cat(sam, range(len(win)))

    def calls(s, b):
        o1 = s.imu_predict_batch(*args)
        assert np.isfinite(o1[1][np.repeat(o1[2] == 0, ms)]).all() and np.isfinite(o1[0]).all()
        ms8, launches = s.last_timing()
        assert launches[:4].tolist() == [1, 1, 1, 1] and ms8[7] >= ms8[3] > 0 and (ms8[:3] > 0).all() and not ms8[4:7].any()
        s.imu_predict_batch(*args, cov=False)
        s.imu_predict_batch(*args, last_only=True)
    qh.check_leaves_the_solve_alone(cv, ws, calls, sels)


def test_refusals_leave_the_handle_usable(cv):
    """Case 7: CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a window id or frame out of range, n < 0, a NULL n_imu / imu_t / imu_gyro
    / imu_acc / noise / win with n > 0, all three outputs NULL, m < 1 or m > 4096, times not strictly increasing, a non-finite measurement,
    a negative or non-finite sigma; n == 0 is fine; the handle solves afterwards like a fresh one."""
    import ctypes as C
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    t, gyro, acc = draw(w, 3, 90)
    win = np.zeros(1, np.int32); fr = np.zeros(1, np.int32); m = np.array([3], np.int32)
    x = np.zeros(3 * 16); cov = np.zeros(3 * 225); st = np.zeros(1, np.int32)
    nz = cv.capi.ImuNoise(4e-3, 8e-2, 2e-6, 4e-5)
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        batch = lambda n=1, win=win, fr=None, m=m, t=t, g=gyro, a=acc, nz=nz, lo=0, x=x, c=cov, st=st: lib.ctvio_imu_predict_batch(
            h, n, None if win is None else p(win), None if fr is None else p(fr), None if m is None else p(m), None if t is None else p(t),
            None if g is None else p(g), None if a is None else p(a), None if nz is None else C.byref(nz), lo,
            None if x is None else p(x), None if c is None else p(c), None if st is None else p(st))
        single = lambda wid=0, f=-1, m=3, t=t, g=gyro, a=acc, nz=nz, x=x, c=cov, st=st: lib.ctvio_imu_predict(
            h, wid, f, m, None if t is None else p(t), None if g is None else p(g), None if a is None else p(a), None if nz is None else C.byref(nz), 0,
            None if x is None else p(x), None if c is None else p(c), None if st is None else p(st))
        assert batch() == 4 and single() == 4                                     # before the upload
        s.set_windows([w.copy()])
        assert batch(win=np.array([1], np.int32)) == 1 and batch(win=np.array([-1], np.int32)) == 1
        assert single(wid=1) == 1 and single(wid=-1) == 1
        for f in (-1, w.F):
            assert batch(fr=np.array([f], np.int32)) == 1
        assert single(f=w.F) == 1 and single(f=-2) == 1
        assert batch(n=-1) == 1
        for k in ("win", "m", "t", "g", "a", "nz"):
            assert batch(**{k: None}) == 1, k
        for k in ("t", "g", "a", "nz"):
            assert single(**{k: None}) == 1, k
        assert batch(x=None, c=None, st=None) == 1 and single(x=None, c=None, st=None) == 1
        assert batch(m=np.array([0], np.int32)) == 1 and batch(m=np.array([4097], np.int32)) == 1 and single(m=0) == 1 and single(m=4097) == 1
        for bad_t in (t[[0, 2, 1]].copy(), t[[0, 1, 1]].copy()):
            assert batch(t=bad_t) == 1 and single(t=bad_t) == 1
        for val in (np.nan, np.inf):
            bad = gyro.copy(); bad[1, 2] = val
            assert batch(g=bad) == 1 and batch(a=bad) == 1 and single(g=bad) == 1
        for k in ("gyr_n", "acc_n", "gyr_w", "acc_w"):
            for val in (-1e-3, np.nan, np.inf):
                b = cv.capi.ImuNoise(4e-3, 8e-2, 2e-6, 4e-5)
                setattr(b, k, val)
                assert batch(nz=b) == 1 and batch(nz=b, c=None) == 1 and single(nz=b) == 1, (k, val)
        with pytest.raises(cv.capi.CtvioError, match="invalid"):
            s.imu_predict_batch([3], None, [3], t, gyro, acc)
        assert lib.ctvio_imu_predict_batch(h, 0, None, None, None, None, None, None, None, 0, None, None, None) == 0
        x0, c0, s0 = s.imu_predict_batch([], None, [], [], np.zeros((0, 3)), np.zeros((0, 3)))
        assert x0.shape == (0, 16) and c0.shape == (0, 15, 15) and s0.shape == (0,)
        x1, c1, s1 = s.imu_predict(0, None, t, gyro, acc)
        assert s1[0] == 0
        assert batch(x=None, st=None) == 0 and np.array_equal(cov, c1.ravel())     # each output alone
        assert batch(c=None, st=None) == 0 and np.array_equal(x, x1.ravel())
        st[0] = 7
        assert batch(x=None, c=None) == 0 and st[0] == 0
        zero = cv.capi.ImuNoise(0.0, 0.0, 0.0, 0.0)
        assert batch(nz=zero) == 0                                                 # sigma 0 is allowed
        qh.check_usable_after(cv, w, s)


def test_adaptor_predict_matches_python(cv, tmp_path):
    """Case 8: tests/imu_predict_demo.cpp through the C++ adaptor: the states and covariances of 11 samples from the newest frame time, with the
    newest bias state and with bias state 1, equal the Python call on the same window at the demo's solved state, bit for bit."""
    w0 = cv.synth.make_window("config1", seed=1005)
    K, F, L = w0.K, w0.F, w0.L
    m = 11
    t, gyro, acc = draw(w0, m, 1005)
    with open(tmp_path / "samples.txt", "w") as fh:
        fh.write(f"{m}\n")
        for j in range(m):
            fh.write(f"{int(t[j])} " + " ".join(repr(float(v)) for v in np.concatenate([gyro[j], acc[j]])) + "\n")
    wa, rest = qh.run_demo(qh.build_demo("imu_predict_demo", tmp_path), w0, tmp_path, 15, str(tmp_path / "samples.txt"))
    got = []
    for _ in range(2):
        assert rest[0] == 1 and rest[1] == m
        got.append((rest[2:2 + 10 * m].reshape(m, 10), rest[2 + 10 * m:2 + 235 * m].reshape(m, 15, 15)))
        rest = rest[2 + 235 * m:]
    assert rest.size == 0
    with cv.Solver() as s:
        s.set_windows([wa])
        new = s.imu_predict(0, None, t, gyro, acc)
        one = s.imu_predict(0, 1, t, gyro, acc)
    for (x_cpp, c_cpp), (x, c, st) in zip(got, (new, one)):
        assert not st.any()
        assert np.array_equal(x_cpp, x[:, :10]) and np.array_equal(c_cpp, c)
    assert not np.array_equal(new[0][-1, :10], one[0][-1, :10])                    # another bias state: another prediction
