"""GPU (-m gpu): ctvio_body_rates_batch / ctvio_body_rates (csrc/kernels_cov.hpp: k_cov_rates_jac, k_cov_solve tiles of kind TILE_RATES) against the
NumPy reference: cov_helpers.cov_reference on the DEVICE's own ctvio_linearize output of the same state with all P unknowns selected (as
tests/test_gpu_nav_state.py, and for its reason), mapped through the NumPy Jacobian of tests/rates_helpers.py.

Tolerance, entry by entry, the nav-state test's: |C_ab - ref_ab| / sqrt(ref_aa ref_bb) <= 4 kappa_s 2^-53 sqrt(g_a g_b), with
g_a = (sum_k |J_ak| sqrt(Sigma_kk))^2 / Pi_aa the amplification of row a through J.  EVERY entry of every status-0 query is compared at this
bound.  Before comparing, the bound itself is held under a cap -- 1e-4 among bias rows (g = 1), 1e-3 for entries with an omega, f or v_B row
-- wherever the REFERENCE ALONE can meet that cap.  The omega rows are first differences of knots, the f rows second differences, so
their g grows along the window, away from the prior, much faster than the velocity rows' of the nav-state test.  Measured on the CPU from
the helper and the oracle's linearisation at the initial state (kappa_s 3.1e10 on `tiny`, 4 kappa_s 2^-53 = 1.4e-5; 1.7e10 and 7.6e-6 on
`config1` seed 1003):

  `tiny` (s, u)      g omega   g f      g v_B   largest bound without the f rows   with the f rows
  (0, 0)             3.2       21.7     2.3     4.4e-5                             3.0e-4
  (1, 0.9)           6.0       46.1     2.6     8.4e-5                             6.4e-4
  (5, 0.37)          61.3      776      19.1    8.5e-4                             1.1e-2
  (7, 0.999)         51.4      2.2e4    23.4    7.2e-4                             0.31
  (8, 0)             51.2      2.2e4    23.3    7.1e-4                             0.31
  `config1` initial: g f between 341 (segment 0) and 7.4e5 (segment 20): bound 2.6e-3 .. 5.6 -- no u at which an f row meets 1e-3;
  g omega 7.5 .. 15.6 at segment 0, 15 .. 34 at 3, 75 .. 162 at 8, 165 .. 352 at 12 (bound 2.7e-3); g v_B 3 .. 6, 13 .. 33, 41 .. 95, 67 .. 150.

So the cap is asserted on every entry among the omega, v_B and bias rows of every query, and on the entries with an f row at the `tiny`
queries (0, 0) and (1, 0.9); an f row of `config1` cannot meet 1e-3 at any u for the reference alone, so the f rows are held to the cap on
`tiny` only, and there not at (5, 0.37), (7, 0.999) and (8, 0), where the reference alone misses it by a factor of 11 to 310.  The cap is
not widened anywhere; the f entries without a cap are still compared at their bound.  What covers the f rows beside the two capped
queries: tests/test_ratesjac_host.py (the device function against the helper at 1e-11), tests/test_rates_reference.py (the helper against
the oracle's IMU residual Jacobian), and case 3 here (the f values against ctvio_residual_summary).  The `config1` queries of case 2 are
taken from the first four segments, where the omega and v_B rows keep the cap at the initial kappa_s as well; kappa_s and g per row class
are printed by every check.

Measured on an MI355X (the device's own linearisation).  `tiny`, initial: kappa_s 3.14e10 and the g of the table above to three digits;
largest bound among the capped entries 8.5e-4, largest error 1.2e-6 (a bias entry, at its bound 1.4e-5: error / bound 0.084).  `config1`
seed 1003 after solve(15): kappa_s 4.47e9, 4 kappa_s 2^-53 = 2.0e-6; g omega 26 .. 143, g f 786 .. 5.7e3 (bound 1.6e-3 .. 1.1e-2: above
the cap at the solved state too), g v_B 5 .. 56; largest bound among the capped entries 2.9e-4; worst error / bound 0.068 (1.3e-7 at 2.0e-6).
`tiny` with locked biases: kappa_s 4.2e4, every bound below 5e-8, worst error / bound 0.034."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import query_harness as qh  # noqa: E402
from query_harness import DET, device_reference  # noqa: E402,F401

OFF = ~np.eye(15, dtype=bool)
TINY_QUERIES = ((0, 0.0), (1, 0.9), (5, 0.37), (7, 0.999), (8, 0.0), (8, 0.5))
TINY_F_CAPPED = (0, 1)                                  # the `tiny` queries whose f rows are held to the cap (see above)
C1_QUERIES = ((0, 0.0), (0, 0.37), (1, 0.9), (2, 0.25), (3, 0.0), (3, 0.37))


def check(w, ref, times, frames, rates, cov, st, what, f_capped=(), expect=None):
    """Every query of one window (w: the window at the device's state) against the reference: the status, the rule of that status, the values
    against the oracle's NumPy spline evaluation, and for status 0 every entry of the covariance at its bound.  f_capped: the queries whose
    f-row entries are held to the cap as well.  Returns the largest (error / bound, error, bound) over the entries."""
    import cov_helpers as ch
    import navstate_helpers as nh
    import rates_helpers as rh
    n = len(times)
    assert rates.shape == (n, 9) and cov.shape == (n, 15, 15) and st.shape == (n,)
    worst = (0.0, 0.0, 0.0)
    for i, t in enumerate(times):
        f = None if frames is None else int(frames[i])
        jac = rh.rates_jacobian(w, t, f)
        r, rs = nh.nav_cov_reference(ref, jac, w.K)
        assert st[i] == rs, (what, i, t, st[i], rs)
        if expect is not None:
            assert st[i] == expect[i], (what, i, t, st[i], expect[i])
        c = cov[i]
        if rs == rh.OUTSIDE:
            assert np.isnan(c).all() and np.isnan(rates[i]).all(), (what, i)
            continue
        val, _ = rh.rates_numpy(w, t, f)
        assert (np.abs(rates[i] - val) <= 1e-12 * np.maximum(1.0, np.abs(val))).all(), (what, i, rates[i], val)
        if rs == rh.UNTOUCHED:
            assert np.isposinf(np.diag(c)).all() and not c[OFF].any(), (what, i)
            continue
        assert np.isfinite(c).all() and np.array_equal(c, c.T), (what, i)
        if not r.any():                            # only constant unknowns: the exact zero matrix
            assert not c.any(), (what, i)
            continue
        assert (np.diag(c)[np.diag(r) > 0] > 0).all(), (what, i)
        g = nh.row_amplification(jac.J, ref.cov_full)
        tol, _ = nh.entry_bounds(ch.bound(ref.kappa), g)
        cap = rh.caps()
        held = np.ones((15, 15), bool)
        if i not in f_capped:
            held[rh.FORCE, :] = False
            held[:, rh.FORCE] = False
        e = nh.entry_errors(c, r)
        k = np.unravel_index(np.argmax(e / tol), e.shape)
        print(f"{what} query {i} (s {jac.s}, u {jac.u:.3g}, frame {jac.frame}): kappa_s {ref.kappa:.3g}, g omega {g[rh.OMEGA].max():.3g} f {g[rh.FORCE].max():.3g} "
              f"v_B {g[rh.VELB].max():.3g} bias {g[9:].max():.3g}, bound bias {tol[9:, 9:].max():.3g} capped entries {tol[held].max():.3g} all {tol.max():.3g}, "
              f"worst entry {k}: error {e[k]:.3g} at bound {tol[k]:.3g}")
        assert np.isfinite(ref.kappa) and (tol[held] < cap[held]).all(), (what, i, float(tol[held].max()))
        assert (e <= tol).all(), (what, i, k, float(e[k]), float(tol[k]))
        worst = max(worst, (float(e[k] / tol[k]), float(e[k]), float(tol[k])))
    return worst


def same(a, b):
    return qh.same_bits(tuple(a), tuple(b))


def test_tiny_initial_state(cv):
    """Case 1: `tiny` seed 7 at the initial state (P = 103, four 32-row blocks, bias rows at 72..101, the last knot untouched): the statuses the
    helper derives, 0, 0, 0, 0, 0, 2, 3, 3, with frames i mod F; frame = NULL equals frame F - 1."""
    import rates_helpers as rh
    w = cv.synth.make_window("tiny", seed=7)
    assert (w.K, w.P, w.F) == (12, 103, 5)
    times = [rh.time_of(w, s, u) for s, u in TINY_QUERIES]
    times += [w.t0_ns - 1, w.t0_ns + (w.K - 3) * w.dt_ns]           # before t0; the end of the spline
    frames = [i % w.F for i in range(len(times))]
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = device_reference(s, 0, w)
        rates, cov, _, st = s.body_rates(0, times, frames)
        rates_n, cov_n, _, st_n = s.body_rates(0, times)
        out_l = s.body_rates(0, times, [w.F - 1] * len(times))
    check(w, ref, times, frames, rates, cov, st, "tiny", f_capped=TINY_F_CAPPED, expect=[0, 0, 0, 0, 0, 2, 3, 3])
    check(w, ref, times, None, rates_n, cov_n, st_n, "tiny, newest frame", f_capped=TINY_F_CAPPED)
    assert same((rates_n, cov_n, None, st_n), out_l)
    assert np.isposinf(np.diag(cov[5])).all() and not cov[5][OFF].any() and np.isfinite(rates[5]).all()
    assert np.isnan(cov[6:]).all() and np.isnan(rates[6:]).all()


@pytest.fixture(scope="module")
def config1_solved(cv):
    """`config1` seed 1003 after a 15-iteration solve on an open handle: (solver, the window at the solved state, the device reference, the
    queries, the covariance call's outputs)."""
    import rates_helpers as rh
    for s, w in qh.solved_window(cv, "config1", 1003, 15):
        times = np.array([rh.time_of(w, sg, u) for sg, u in C1_QUERIES], np.int64)
        frames = np.array([i % w.F for i in range(len(times))], np.int32)
        yield s, w, device_reference(s, 0, w), times, frames, s.body_rates(0, times, frames)


def test_config1_solved_against_reference(config1_solved):
    """Case 2: `config1` seed 1003, solved (P = 211: the block substitution crosses 32-row blocks and reads inside the envelope)."""
    s, w, ref, times, frames, (rates, cov, _, st) = config1_solved
    assert w.P == 211 and not st.any(), st
    e = check(w, ref, [int(t) for t in times], frames, rates, cov, st, "config1 solved")
    print(f"config1 solved: worst error / bound {e[0]:.3g} (error {e[1]:.3g} at bound {e[2]:.3g})")


def test_config1_solved_bits(cv, config1_solved):
    """Case 2: the bits of a query depend on its own arguments alone: the values-only call, the batch entry, a permuted order, a call with the
    gate, a second call; and a 2-window batch of `tiny` + `config1` under deterministic = 2 against its single-window entries."""
    s, w, _, times, frames, out = config1_solved
    n = len(times)
    vals = s.body_rates(0, times, frames, cov=False)
    assert vals[1] is None and vals[2] is None and np.array_equal(vals[0], out[0]) and np.array_equal(vals[3], out[3])
    ms, launches = s.last_timing()
    assert launches[:3].tolist() == [0, 0, 1] and ms[7] >= ms[2] > 0
    assert same(s.body_rates_batch(np.zeros(n, np.int32), times, frames), out)
    perm = np.random.default_rng(3).permutation(n)
    po = s.body_rates(0, times[perm], frames[perm])
    assert same([x[perm] for x in out[:2]] + [None, out[3][perm]], po)
    meas = np.tile(np.array([0.1, -0.2, 0.3, 0.5, -0.4, 9.6]), (n, 1))
    go = s.body_rates(0, times, frames, meas=meas)
    assert np.isfinite(go[2]).all() and (go[2] > 0).all() and same((go[0], go[1], None, go[3]), out)
    ms, launches = s.last_timing()
    assert launches[:3].tolist() == [1, 1, 1] and ms[7] >= ms[1] > 0 and not ms[3:7].any()
    assert same(s.body_rates(0, times, frames, meas=meas), go) and same(s.body_rates(0, times, frames), out)
    import rates_helpers as rh
    tiny = cv.synth.make_window("tiny", seed=7)
    c1 = cv.synth.make_window("config1", seed=1003)
    tt = [rh.time_of(tiny, sg, u) for sg, u in TINY_QUERIES]
    tc = [rh.time_of(c1, sg, u) for sg, u in C1_QUERIES]
    win = np.array([0, 1] * len(tt), np.int32)
    t2 = np.array([x for pair in zip(tt, tc) for x in pair], np.int64)
    f2 = np.array([i % 5 for i in range(len(t2))], np.int32)
    m2 = np.tile(np.array([0.1, -0.2, 0.3, 0.5, -0.4, 9.6]), (len(t2), 1))
    with cv.Solver(**DET) as d:
        d.set_windows([tiny.copy(), c1.copy()])
        both = d.body_rates_batch(win, t2, f2, meas=m2)
        assert same(d.body_rates_batch(win, t2, f2, meas=m2), both)
        rev = d.body_rates_batch(win[::-1].copy(), t2[::-1].copy(), f2[::-1].copy(), meas=m2[::-1].copy())
        assert same([x[::-1] for x in rev], both)
        for i in (0, 1):
            idx = np.nonzero(win == i)[0]
            assert same(d.body_rates(i, t2[idx], f2[idx], meas=m2[idx]), [x[idx] for x in both]), i
        assert both[3].tolist() == [0, 0] * 5 + [2, 0]


def test_values_against_residual_summary(cv):
    """Case 3: every IMU sample time of `tiny` with the sample's own bias state, values only: sum_k |imu_w (rates + bias - meas)| per
    component equals ctvio_residual_summary's IMU sums.  The two device paths differ in rounding alone; per sample and component that is
    held to 64 x 2^-53 x imu_w x max(|z|, |meas|), summed over the samples."""
    w = cv.synth.make_window("tiny", seed=7)
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        rates, cov, chi, st = s.body_rates(0, w.imu_t, w.imu_bias, cov=False)
        sums, cnt = s.residual_summary(0)["imu"]
    assert cov is None and chi is None and not st.any() and cnt == w.M
    z = rates[:, :6] + w.bias[w.imu_bias]
    meas = np.concatenate([w.imu_gyro, w.imu_acc], 1)
    got = (np.abs(z - meas) * w.imu_w).sum(0)
    tol = (64 * 2.0 ** -53 * w.imu_w * np.maximum(np.abs(z), np.abs(meas))).sum(0)
    print("IMU sums", sums, "difference", np.abs(got - sums), "tolerance", tol)
    assert (np.abs(got - sums) <= tol).all()


def test_gate(cv):
    """Case 4: the window's own sample at a query time and the same sample plus ten sigma on one axis: chi2 against NumPy on the RETURNED
    cov225 and rates9 bits at rtol 64 cond(S) 2^-53; noise6 = 1 / imu_w gives the bits of noise6 = NULL; status 2 gives 0, status 3 NaN."""
    import rates_helpers as rh
    w = cv.synth.make_window("tiny", seed=7)
    sig = 1.0 / w.imu_w
    pick = [int(m) for m in (1, w.M // 3, w.M // 2)]
    times = [int(w.imu_t[m]) for m in pick] * 2 + [rh.time_of(w, 8, 0.5), w.t0_ns - 1]
    frames = [int(w.imu_bias[m]) for m in pick] * 2 + [0, 0]
    meas = np.array([np.concatenate([w.imu_gyro[m], w.imu_acc[m]]) for m in pick] * 2 + [np.zeros(6)] * 2)
    for j in range(3):
        meas[3 + j, 2 * j] += 10 * sig[2 * j]               # ten sigma on axes 0, 2, 4
    custom = np.array([2e-3, 3e-3, 4e-3, 0.05, 0.06, 0.07])
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        rates, cov, chi, st = s.body_rates(0, times, frames, meas=meas)
        assert same(s.body_rates(0, times, frames, meas=meas, noise=sig), (rates, cov, chi, st))
        _, cov_c, chi_c, _ = s.body_rates(0, times, frames, meas=meas, noise=custom)
    assert st.tolist() == [0] * 6 + [2, 3] and chi[6] == 0.0 and np.isnan(chi[7]) and chi_c[6] == 0.0 and np.isnan(chi_c[7])
    assert np.array_equal(cov_c, cov, equal_nan=True)
    for i in range(6):
        for c2, sg in ((chi, sig), (chi_c, custom)):
            ref, S = rh.gate(rates[i], w.bias[frames[i]], cov[i], meas[i], sg)
            rtol = 64 * np.linalg.cond(S) * 2.0 ** -53
            print(f"gate {i}: chi2 {c2[i]:.6g} numpy {ref:.6g} cond(S) {np.linalg.cond(S):.3g}")
            assert abs(c2[i] - ref) <= rtol * ref, (i, c2[i], ref, rtol)


def test_constants(cv):
    """Case 5: `tiny` with lock_bg = lock_ba = 1: exact zero bias rows and columns; with every knot constant as well (fixed_upto = K - 1): the
    exact zero matrix and status 0."""
    import rates_helpers as rh
    w = cv.synth.make_window("tiny", seed=7)
    w.lock_bg = 1; w.lock_ba = 1
    w.normalize()
    times = [rh.time_of(w, 0, 0.0), rh.time_of(w, 1, 0.9)]
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = device_reference(s, 0, w)
        rates, cov, _, st = s.body_rates(0, times, [1, 2])
    assert st.tolist() == [0, 0]
    for c in cov:
        assert not c[9:].any() and not c[:, 9:].any() and (np.diag(c)[:9] > 0).all()
    check(w, ref, times, [1, 2], rates, cov, st, "tiny, locked biases", f_capped=(0, 1))
    w.fixed_upto = w.K - 1
    w.normalize()
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        rates, cov, chi, st = s.body_rates(0, times + [rh.time_of(w, 8, 0.5)], [1, 2, 0], meas=np.ones((3, 6)))
    assert st.tolist() == [0, 0, 0] and not cov.any() and np.isfinite(rates).all() and np.isfinite(chi).all() and (chi > 0).all()


def test_leaves_the_solve_alone(cv):
    """Case 6: state bits, graph captures and a following solve are unchanged by the call."""
    import rates_helpers as rh
    w = cv.synth.make_window("config1", seed=1003)
    times = [rh.time_of(w, sg, u) for sg, u in C1_QUERIES]

    def calls(s, b):
        o1 = s.body_rates(0, times, meas=np.ones((len(times), 6)))
        assert not o1[3].any() and np.isfinite(o1[1]).all() and np.isfinite(o1[2]).all()
        s.body_rates(0, times, cov=False)
    qh.check_leaves_the_solve_alone(cv, [w], calls, solver_kw={})


def test_refusals_leave_the_handle_usable(cv):
    """Case 7: CTVIO_ERR_STATE before the upload; every CTVIO_ERR_INVALID case of ctvio.h, each followed by a valid call on the same handle;
    n == 0 is fine."""
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    t = np.array([w.t0_ns + 1], np.int64); win = np.zeros(1, np.int32); fr = np.zeros(1, np.int32)
    x = np.zeros(9); cov = np.zeros(225); chi = np.zeros(1); st = np.zeros(1, np.int32)
    z = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 9.8]); sg = np.full(6, 0.1)
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        batch = lambda n, wi, tt, f, m, ns, a, b, c, d: lib.ctvio_body_rates_batch(h, n, wi, tt, f, m, ns, a, b, c, d)
        single = lambda i, n, tt, f, m, ns, a, b, c, d: lib.ctvio_body_rates(h, i, n, tt, f, m, ns, a, b, c, d)
        assert batch(1, p(win), p(t), None, None, None, p(x), p(cov), None, p(st)) == 4
        assert single(0, 1, p(t), None, None, None, p(x), p(cov), None, p(st)) == 4
        s.set_windows([w.copy()])

        def valid():
            assert single(0, 1, p(t), None, p(z), None, p(x), p(cov), p(chi), p(st)) == 0 and st[0] == 0 and np.isfinite(chi[0])

        valid()
        x1, c1, chi1 = x.copy(), cov.copy(), chi.copy()
        bad = np.array([1], np.int32)
        inf6, nan6, neg6, zero6 = z.copy(), z.copy(), sg.copy(), sg.copy()
        inf6[2] = np.inf; nan6[4] = np.nan; neg6[1] = -0.1; zero6[5] = 0.0
        infs = sg.copy(); infs[0] = np.inf
        refused = [
            lambda: batch(1, p(bad), p(t), None, None, None, p(x), p(cov), None, p(st)),               # window id out of range
            lambda: single(1, 1, p(t), None, None, None, p(x), p(cov), None, p(st)),
            lambda: single(-1, 1, p(t), None, None, None, p(x), p(cov), None, p(st)),
            lambda: batch(1, p(win), p(t), p(np.array([-1], np.int32)), None, None, p(x), p(cov), None, p(st)),   # frame out of range
            lambda: single(0, 1, p(t), p(np.array([w.F], np.int32)), None, None, p(x), None, None, p(st)),
            lambda: batch(-1, p(win), p(t), None, None, None, p(x), p(cov), None, p(st)),              # n < 0
            lambda: single(0, -1, p(t), None, None, None, p(x), p(cov), None, p(st)),
            lambda: batch(1, None, p(t), None, None, None, p(x), p(cov), None, p(st)),                 # NULL win / t_ns
            lambda: batch(1, p(win), None, None, None, None, p(x), p(cov), None, p(st)),
            lambda: single(0, 1, None, None, None, None, p(x), p(cov), None, p(st)),
            lambda: batch(1, p(win), p(t), None, p(z), None, None, None, None, None),                  # every output NULL
            lambda: single(0, 1, p(t), p(fr), None, None, None, None, None, None),
            lambda: single(0, 1, p(t), None, None, None, p(x), p(cov), p(chi), p(st)),                 # chi2 without meas6
            lambda: single(0, 1, p(t), None, p(inf6), None, p(x), p(cov), p(chi), p(st)),              # non-finite meas6
            lambda: single(0, 1, p(t), None, p(nan6), None, p(x), p(cov), p(chi), p(st)),
            lambda: single(0, 1, p(t), None, p(z), p(neg6), p(x), p(cov), p(chi), p(st)),              # noise6: negative, zero, non-finite
            lambda: single(0, 1, p(t), None, p(z), p(zero6), p(x), p(cov), p(chi), p(st)),
            lambda: single(0, 1, p(t), None, p(z), p(infs), p(x), p(cov), p(chi), p(st)),
        ]
        for i, call in enumerate(refused):
            assert call() == 1, i
            valid()
            assert np.array_equal(x, x1) and np.array_equal(cov, c1) and np.array_equal(chi, chi1), i
        with pytest.raises(cv.capi.CtvioError, match="invalid"):
            s.body_rates_batch([3], t)
        assert batch(0, None, None, None, None, None, None, None, None, None) == 0
        assert single(0, 0, None, None, None, None, None, None, None, None) == 0
        r0, c0, ch0, s0 = s.body_rates(0, [])
        assert r0.shape == (0, 9) and c0.shape == (0, 15, 15) and ch0 is None and s0.shape == (0,)
        assert single(0, 1, p(t), None, None, None, None, p(cov), None, None) == 0 and np.array_equal(cov, c1)     # each output alone
        assert single(0, 1, p(t), None, None, None, p(x), None, None, None) == 0 and np.array_equal(x, x1)
        assert single(0, 1, p(t), None, p(z), None, None, None, p(chi), None) == 0 and np.array_equal(chi, chi1)
        assert single(0, 1, p(t), None, None, None, None, None, None, p(st)) == 0 and st[0] == 0
        wz = w.copy()                                      # a non-positive weight (the same H: weights enter squared): the default noise has no sigma for it
        wz.imu_w = wz.imu_w.copy(); wz.imu_w[5] = -wz.imu_w[5]
        s.set_windows([wz])
        assert single(0, 1, p(t), None, p(z), None, p(x), p(cov), p(chi), p(st)) == 1
        assert single(0, 1, p(t), None, p(z), p(sg), p(x), p(cov), p(chi), p(st)) == 0 and np.isfinite(chi[0])
        assert single(0, 1, p(t), None, None, None, p(x), p(cov), None, p(st)) == 0
        qh.check_usable_after(cv, w, s)


def test_adaptor_body_rates_matches_python(cv, tmp_path):
    """tests/body_rates_demo.cpp through the C++ adaptor: the rates, covariances, twists and the gated sample equal the Python call on the same
    window at the demo's solved state, bit for bit."""
    w0 = cv.synth.make_window("config1", seed=1005)
    K, F, L = w0.K, w0.F, w0.L
    n, g = 4, w0.M // 4
    wa, rest = qh.run_demo(qh.build_demo("body_rates_demo", tmp_path), w0, tmp_path, 15, n, g)
    assert rest[0] == 1 and rest[1] == n
    r_cpp, c_cpp = rest[2:2 + 9 * n].reshape(n, 9), rest[2 + 9 * n:2 + 234 * n].reshape(n, 15, 15)
    tw = rest[2 + 234 * n:2 + 276 * n].reshape(n, 42)
    ok_gate, chi_cpp = rest[2 + 276 * n:2 + 276 * n + 2]
    times = [int(w0.t0_ns + (i + 1) * (K - 4) * w0.dt_ns // (n + 1)) for i in range(n)]
    with cv.Solver() as s:
        s.set_windows([wa])
        rates, cov, _, st = s.body_rates(0, times)
        _, _, chi, stg = s.body_rates(0, [int(w0.imu_t[g])], [int(w0.imu_bias[g])], meas=np.concatenate([w0.imu_gyro[g], w0.imu_acc[g]])[None])
    assert not st.any() and np.array_equal(r_cpp, rates) and np.array_equal(c_cpp, cov)
    pick = [6, 7, 8, 0, 1, 2]
    assert np.array_equal(tw[:, :6], rates[:, pick]) and np.array_equal(tw[:, 6:].reshape(n, 6, 6), cov[:, pick][:, :, pick])
    assert ok_gate == 1 and stg[0] == 0 and chi_cpp == chi[0]
