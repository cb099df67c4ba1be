"""GPU (-m gpu): ctvio_imu_gate_batch / ctvio_imu_gate (csrc/kernels_cov.hpp: k_cov_imugate_jac, k_cov_solve tiles of kind TILE_IMUGATE,
k_cov_imugate_reduce) against the NumPy reference of tests/imugate_helpers.py on the DEVICE's own ctvio_linearize output of the same state
(as tests/test_gpu_visual_gate.py, and for its reason).

Per sample, in this order: the status (samples whose reference redundancy lies within a factor 4 of min_redundancy are not compared on it,
at most 5 % of a window); res6 within imu_w_k 1e-12 max(1, |z_k|), the body-rates value convention; redundancy within
hat_bound + 64 * 2^-53 (imugate_helpers: hat_bound = 4 kappa_s 2^-53 |A|_2, norm-wise; 64 * 2^-53 the 6 x 6 step's own rounding,
tests/test_imugate_host.py); cov36 symmetric to the bit with a positive diagonal and |C - ref|_2 / |ref + I|_2 <= (hat_bound + 64 * 2^-53) /
redundancy, hat_bound < 1e-4 asserted first; chi2 against r^T (I - A_ref)^-1 r formed from the RETURNED res6, at the same relative bound.
Per bias state: the count and the extremes bit-equal to the returned per-sample arrays, the mean within n 2^-52 of their NumPy sum."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import query_harness as qh  # noqa: E402
from query_harness import DET, device_joint_reference as device_reference  # noqa: E402,F401

EPS = 2.0 ** -53
FIELDS = ("res", "redundancy", "cov", "chi2", "status", "frame_stats")
VALUES = ("res",)
IMU_ARRAYS = ("imu_t", "imu_gyro", "imu_acc", "imu_bias")


def references(w, ref, min_red=0.01):
    import imugate_helpers as ig
    return [ig.sample_reference(w, ref, m, min_red) for m in range(w.M)]


def same(a, b, fields=FIELDS):
    return qh.same_bits(a, b, fields)


def take(o, ms, fs):
    return SimpleNamespace(**{f: (getattr(o, f)[fs] if f == "frame_stats" else getattr(o, f)[ms]) for f in FIELDS})


def check(w, R, out, what, min_red=0.01, values_only=False):
    """out (Solver.imu_gate) against the per-sample references R; returns the worst (error / bound, bound) of cov36."""
    import imugate_helpers as ig
    M = w.M
    assert out.res.shape == (M, 6) and out.status.shape == (M,)
    wgt = np.asarray(w.imu_w, float)
    skipped, worst, worst_red, worst_chi = 0, (0.0, 0.0), 0.0, 0.0
    for m, r in enumerate(R):
        near = not values_only and r.status in (ig.OK, ig.WEAK) and min_red / 4 <= r.redundancy <= 4 * min_red
        if near:
            skipped += 1
            assert out.status[m] in (ig.OK, ig.WEAK), (what, m, out.status[m])
        else:
            assert out.status[m] == (ig.OK if values_only else r.status), (what, m, out.status[m], r.status, r.redundancy)      # 1. the status
        st = int(out.status[m])
        assert (np.abs(out.res[m] - r.res) <= wgt * 1e-12 * np.maximum(1.0, np.abs(r.z))).all(), (what, m, out.res[m], r.res)     # 2. the values
        if values_only:
            continue
        c = out.cov[m]
        off = c[~np.eye(6, dtype=bool)]
        if st == ig.NO_INFO:
            assert out.redundancy[m] == 0.0 and np.isposinf(np.diag(c)).all() and not off.any() and out.chi2[m] == 0.0, (what, m)
            continue
        tol = r.tol + ig.STEP
        e = abs(out.redundancy[m] - r.redundancy)                                                                            # 3. the redundancy
        assert e <= tol, (what, m, out.redundancy[m], r.redundancy, tol)
        worst_red = max(worst_red, e / tol)
        if st == ig.WEAK:
            assert np.isposinf(np.diag(c)).all() and not off.any() and out.chi2[m] == 0.0, (what, m)
            continue
        assert np.isfinite(c).all() and np.array_equal(c, c.T) and ((np.diag(c) > 0).all() or not r.A.any()), (what, m, c)      # 4. the covariance
        if r.status != ig.OK:
            continue       # (a sample near the threshold that the reference calls weak: it has no reference covariance)
        assert r.tol < 1e-4, (what, m, r.tol)
        e = ig.cov_error(c, r.cov)
        assert e <= tol / r.redundancy, (what, m, e, tol / r.redundancy, r.redundancy)
        worst = max(worst, (e / (tol / r.redundancy), tol / r.redundancy))
        val = ig.chi2_of(out.res[m], r.A)                                                                                    # 5. the gate
        assert abs(out.chi2[m] - val) <= tol / r.redundancy * val, (what, m, out.chi2[m], val, tol / r.redundancy)
        worst_chi = max(worst_chi, abs(out.chi2[m] - val) / (tol / r.redundancy * val) if val > 0 else 0.0)
    assert skipped <= 0.05 * M, (what, skipped, M)
    if not values_only:                                                                                                      # 6. the bias states
        assert out.frame_stats.shape == (w.F, 4)
        for f in range(w.F):
            ms = np.nonzero(np.asarray(w.imu_bias) == f)[0]
            ok = ms[out.status[ms] == ig.OK]
            n, mean, cmax, rmin = out.frame_stats[f]
            assert n == ok.shape[0], (what, f, n, ok.shape[0])
            reds = out.redundancy[ms][(out.status[ms] == ig.OK) | (out.status[ms] == ig.WEAK)]
            assert cmax == (out.chi2[ok].max() if ok.shape[0] else 0.0) and rmin == (reds.min() if reds.shape[0] else np.inf), (what, f, out.frame_stats[f])
            if ok.shape[0] == 0:
                assert np.isnan(mean), (what, f, mean)
                continue
            want = out.chi2[ok].sum() / ok.shape[0]
            assert abs(mean - want) <= ok.shape[0] * 2.0 ** -52 * want, (what, f, mean, want)
    print(f"{what}: {M} samples ({skipped} near the threshold), worst use of the bounds: redundancy {worst_red:.3g}, cov36 {worst[0]:.3g} "
          f"(bound {worst[1]:.3g}), chi2 {worst_chi:.3g}")
    return worst


def run(cv, w, what, min_red=0.01, solve=0):
    """One window on a fresh handle: (the window at the device's state, references, values-only output, full output)."""
    with cv.Solver() as s:
        b = [w.copy()]
        s.set_windows(b)
        if solve:
            s.solve(solve)
        R = references(b[0], device_reference(s, 0, b[0]), min_red)
        vals = s.imu_gate(0, cov=False, min_redundancy=min_red)
        full = s.imu_gate(0, min_redundancy=min_red)
    check(b[0], R, vals, what + ", values only", min_red, values_only=True)
    check(b[0], R, full, what, min_red)
    assert same(vals, full, VALUES) and vals.cov is None and vals.frame_stats is None and (vals.status == 0).all()
    return b[0], R, vals, full


def fixture_window(cv, golden_dir, cfg, seed):
    fx = np.load(os.path.join(golden_dir, f"cov_{cfg}_seed{seed}.npz"))
    w = cv.synth.make_window(cfg, seed=seed)
    w.quat[:] = fx["quat"]; w.pos[:] = fx["pos"]; w.bias[:] = fx["bias"]; w.rho[:] = fx["rho"]; w.ld = float(fx["ld"])
    return w


def test_tiny(cv, golden_dir):
    """`tiny` seed 7 at its covariance fixture's state (K 12, M 80; unconverged: huge chi2): no sample near the threshold; eight samples
    at u = 0."""
    import imugate_helpers as ig
    w = fixture_window(cv, golden_dir, "tiny", 7)
    assert (w.K, w.M) == (12, 80)
    _, R, _, full = run(cv, w, "tiny")
    assert all(r.status == ig.OK for r in R) and min(r.redundancy for r in R) > 0.04
    assert (full.chi2 > 0).all() and (full.frame_stats[:, 0].sum() == 80)


def test_config1(cv, golden_dir):
    """`config1` seed 1000 at its covariance fixture's state (K 24, P 211, M 500): no sample near the threshold; the mean deleted chi2
    over the window is 6 within (0.8, 1.25)."""
    import imugate_helpers as ig
    w = fixture_window(cv, golden_dir, "config1", 1000)
    assert (w.K, w.P, w.M) == (24, 211, 500)
    _, R, _, full = run(cv, w, "config1")
    assert all(r.status == ig.OK for r in R) and min(r.redundancy for r in R) > 0.04
    assert 0.8 < full.chi2.mean() / 6 < 1.25, full.chi2.mean()


def test_long_window(cv):
    """K = 34 (P = 301): the linearisation that does not keep the packed Hessian in LDS, the envelope panel Cholesky."""
    w = cv.synth.make_window("config1", seed=1400, F=16, L=60, M=750)
    assert w.K == 34 and w.M == 750
    run(cv, w, "long k34", solve=4)


def weak_window(w0, m):
    w = w0.copy()
    w.bias = np.vstack([w.bias, w.bias[w.imu_bias[m]]])
    w.imu_bias[m] = w0.F
    return w


def test_variants(cv, golden_dir):
    """`tiny`: a sample given a bias state of its own (status 4, reference redundancy below min_redundancy / 10, its neighbours unchanged);
    locked biases; every knot and bias state constant -- the samples depend on constant unknowns alone -- (A = 0: redundancy 1, a zero
    cov36, chi2 = |r|^2); odd M (the last tile holds one sample)."""
    import imugate_helpers as ig
    w = fixture_window(cv, golden_dir, "tiny", 7)
    m = w.M // 2
    xs, R, _, f = run(cv, weak_window(w, m), "tiny, a bias state of its own")
    assert R[m].status == ig.WEAK and R[m].redundancy < 0.01 / 10 and f.status[m] == ig.WEAK
    assert sum(r.status == ig.WEAK for r in R) == 1 and (f.redundancy[[m - 1, m + 1]] > 0.4).all()
    assert f.frame_stats[w.F].tolist()[0] == 0 and np.isnan(f.frame_stats[w.F, 1]) and f.frame_stats[w.F, 2] == 0.0 and f.frame_stats[w.F, 3] == f.redundancy[m]
    x = w.copy(); x.lock_bg = True; x.lock_ba = True
    run(cv, x, "tiny, locked biases")
    x = w.copy(); x.lock_bg = True; x.lock_ba = True; x.fixed_upto = x.K - 1
    _, R, _, f = run(cv, x, "tiny, every knot and bias state constant")
    assert (f.status == 0).all() and (f.redundancy == 1.0).all() and not f.cov.any()
    assert np.allclose(f.chi2, (f.res ** 2).sum(axis=1), rtol=4 * EPS, atol=0)
    x = w.copy()
    for a in IMU_ARRAYS:
        setattr(x, a, getattr(x, a)[:-3])
    assert x.M == 77
    run(cv, x, "tiny, M = 77")


def mixed_windows(cv, golden_dir):
    empty = cv.synth.make_window("tiny", seed=9)
    for a in IMU_ARRAYS:
        setattr(empty, a, getattr(empty, a)[:0])
    empty.normalize()
    assert empty.M == 0 and empty.F > 0
    return [fixture_window(cv, golden_dir, "tiny", 7), fixture_window(cv, golden_dir, "config1", 1000), empty]


def test_bits(cv, golden_dir, monkeypatch):
    """deterministic on: the batch entry over (tiny, config1, a window with M = 0), the single-window entry, a second call, the values-only
    call (for the values), a call with one output alone, a call forced into more than one slice (CTVIO_GATE_SLICE), and that again with
    CTVIO_POISON=1 are bitwise equal."""
    p = cv.capi._p
    ws = mixed_windows(cv, golden_dir)
    moff = np.concatenate([[0], np.cumsum([w.M for w in ws])]); foff = np.concatenate([[0], np.cumsum([w.F for w in ws])])
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        out = s.imu_gate_batch()
        assert out.res.shape[0] == moff[-1] and out.frame_stats.shape[0] == foff[-1]
        assert (out.status == 0).all() and (out.frame_stats[foff[2]:, 0] == 0).all() and np.isnan(out.frame_stats[foff[2]:, 1]).all()
        assert (out.frame_stats[foff[2]:, 2] == 0).all() and np.isposinf(out.frame_stats[foff[2]:, 3]).all()
        for i in range(3):
            assert same(s.imu_gate(i), take(out, slice(moff[i], moff[i + 1]), slice(foff[i], foff[i + 1]))), i
        assert same(s.imu_gate_batch(), out)
        assert same(s.imu_gate_batch(cov=False), out, VALUES)
        o = cv.capi.GateOptions(0.01)
        chi = np.zeros(moff[-1]); red = np.zeros(moff[-1]); fs = np.zeros((foff[-1], 4)); cov = np.zeros((moff[-1], 6, 6))
        assert s._lib.ctvio_imu_gate_batch(s._h, C.byref(o), None, None, None, p(chi), None, None) == 0
        assert s._lib.ctvio_imu_gate_batch(s._h, C.byref(o), None, p(red), None, None, None, None) == 0
        assert s._lib.ctvio_imu_gate_batch(s._h, C.byref(o), None, None, None, None, None, p(fs)) == 0
        assert s._lib.ctvio_imu_gate_batch(s._h, C.byref(o), None, None, p(cov), None, None, None) == 0
        assert np.array_equal(chi, out.chi2) and np.array_equal(red, out.redundancy) and np.array_equal(fs, out.frame_stats, equal_nan=True)
        assert np.array_equal(cov, out.cov)
    monkeypatch.setenv("CTVIO_GATE_SLICE", "64")
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        assert same(s.imu_gate_batch(), out)
        assert same(s.imu_gate(1), take(out, slice(moff[1], moff[2]), slice(foff[1], foff[2])))
    monkeypatch.setenv("CTVIO_POISON", "1")      # (reused scratch starts as NaN: nothing reads what the call has not written)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        assert same(s.imu_gate_batch(), out)
        assert same(s.imu_gate_batch(cov=False), out, VALUES)


def test_leaves_the_solve_alone(cv, golden_dir):
    """State bits, graph captures and a following solve are unchanged by the calls; the timing slots of both modes.  Cross-checks: res6 is
    imu_w (rates9[:6] + bias - meas) from ctvio_body_rates at the sample times, to the bit; the per-component sum of |res6| is
    ctvio_residual_summary's IMU sum within M 2^-52 relative."""
    ws = mixed_windows(cv, golden_dir)[:2]

    def calls(s, b):
        o1 = s.imu_gate_batch()
        ms, launches = s.last_timing()
        assert launches[:4].tolist() == [1, 1, 1, 1] and ms[7] >= ms[1] > 0 and ms[2] > 0 and ms[3] > 0
        o2 = s.imu_gate_batch(cov=False)
        ms, launches = s.last_timing()
        assert launches[:4].tolist() == [0, 0, 1, 0] and ms[7] >= ms[2] > 0
        assert same(o1, o2, VALUES)
        return o1

    def cross_checks(s, b, o1):
        s.writeback_all()
        m0 = 0
        for i, w in enumerate(b):
            rates, _, _, st = s.body_rates(i, w.imu_t, frame=w.imu_bias, cov=False)
            assert (st == 0).all()
            meas = np.concatenate([w.imu_gyro, w.imu_acc], axis=1)
            want = np.asarray(w.imu_w, float) * ((rates[:, :6] + w.bias[w.imu_bias]) - meas)
            assert np.array_equal(o1.res[m0:m0 + w.M], want), (i, np.abs(o1.res[m0:m0 + w.M] - want).max())
            sums, cnt = s.residual_summary(i)["imu"]
            mine = np.abs(o1.res[m0:m0 + w.M]).sum(axis=0)
            print(f"window {i}: sum |res6| against the residual summary: {np.abs(mine - sums) / sums} of M 2^-52 = {w.M * 2.0 ** -52:.3g}")
            assert cnt == w.M and (np.abs(mine - sums) <= w.M * 2.0 ** -52 * sums).all(), (i, mine, sums)
            m0 += w.M
    qh.check_leaves_the_solve_alone(cv, ws, calls, compare_ld=False, then=cross_checks)


def test_callers_sample_order(cv, golden_dir):
    """A window uploaded with its IMU samples shuffled: the per-sample outputs are the same permutation of the unshuffled window's (the
    upload sorts the samples by segment and bias state -- stably, so the packed order and with it the normal equations may differ: the
    values to the bit -- a sample's value depends on its own data alone --, the covariances within the bound).  A wrong inverse permutation
    fails the value comparison."""
    import imugate_helpers as ig
    w = fixture_window(cv, golden_dir, "config1", 1000)
    sh = np.random.default_rng(5).permutation(w.M)
    x = w.copy()
    for a in IMU_ARRAYS:
        setattr(x, a, getattr(x, a)[sh])
    assert not np.array_equal(x.imu_t, w.imu_t)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy()])
        R = references(w, device_reference(s, 0, w))
        a = s.imu_gate(0)
    with cv.Solver(**DET) as s:
        s.set_windows([x.copy()])
        b = s.imu_gate(0)
    assert same(b, take(a, sh, slice(None)), ("res", "status"))
    assert not np.array_equal(b.res, a.res)
    for i, m in enumerate(sh):
        tol = 2 * (R[m].tol + ig.STEP)
        assert abs(b.redundancy[i] - a.redundancy[m]) <= tol, (i, m)
        assert ig.cov_error(b.cov[i], a.cov[m]) <= tol / R[m].redundancy, (i, m)
    assert np.array_equal(b.frame_stats[:, 0], a.frame_stats[:, 0])


def test_refusals_leave_the_handle_usable(cv):
    """CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a bad id, NULL options, min_redundancy outside (0, 1) or non-finite, every
    output NULL with M > 0; the handle gives the same answer afterwards."""
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        st = np.zeros(w.M, np.int32)
        o = cv.capi.GateOptions(0.01)
        none4 = [None] * 4
        assert lib.ctvio_imu_gate_batch(h, C.byref(o), *none4, p(st), None) == 4
        s.set_windows([w.copy()])
        ok = s.imu_gate(0)
        assert lib.ctvio_imu_gate(h, 1, C.byref(o), *none4, p(st), None) == 1
        assert lib.ctvio_imu_gate(h, -1, C.byref(o), *none4, p(st), None) == 1
        assert lib.ctvio_imu_gate(h, 0, None, *none4, p(st), None) == 1
        for bad in (0.0, 1.0, -0.5, 2.0, float("nan"), float("inf")):
            assert lib.ctvio_imu_gate(h, 0, C.byref(cv.capi.GateOptions(bad)), *none4, p(st), None) == 1, bad
        assert lib.ctvio_imu_gate(h, 0, C.byref(o), *none4, None, None) == 1
        assert lib.ctvio_imu_gate(h, 0, C.byref(o), *none4, p(st), None) == 0
        assert np.array_equal(st, ok.status)
        assert same(s.imu_gate(0), ok)
