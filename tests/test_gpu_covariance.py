"""GPU (-m gpu): ctvio_covariance_batch / ctvio_covariance (csrc/kernels_cov.hpp) against the NumPy reference (tests/cov_helpers.py) applied to
the DEVICE's own ctvio_linearize output of the same state -- this isolates the new kernels from linearisation differences (the device's H
is held to the oracle's at 1e-10 elsewhere; kappa_s x 1e-10 would be O(1)).  Tolerance everywhere: 4 kappa_s 2^-53 with kappa_s from the
helper, on max |Sigma_a - Sigma_b| / sqrt(Sigma_ii Sigma_jj) over the finite selected pairs and on the relative error of var_rho.  The smallest
modelling error this must catch -- leftover LM damping at radius 1e4 -- moves Sigma by about 1e-4."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import query_harness as qh  # noqa: E402
from query_harness import DET, same_bits  # noqa: E402,F401  (the other entries' tests take both from here)


def reference(s, wid, w, sel):
    import cov_helpers as ch
    H, W, Hll, _, _ = s.linearize(wid)
    return ch.cov_reference(H, W, Hll, ~ch.constant_mask(w), sel)


def check(cov, var, ref, what):
    """The errors of one window against its reference, asserted at the bound; returns (error of the block, error of var_rho, bound)."""
    import cov_helpers as ch
    tol = ch.bound(ref.kappa)
    assert np.isfinite(ref.kappa) and tol < 1e-4, (what, ref.kappa)   # (a leftover damping moves Sigma by 1e-4: the bound must stay below)
    e = ch.cov_metric(cov, ref.cov_full)
    er = ch.rel_metric(var, ref.rho_full) if var is not None else 0.0
    print(f"{what}: kappa_s {ref.kappa:.3g}, bound {tol:.3g}, error block {e:.3g}, var_rho {er:.3g}, cpu routes {ref.e_cpu:.3g}")
    assert np.array_equal(np.isinf(cov), np.isinf(ref.cov_full)), what
    assert not cov[ref.cov_full == 0].any(), what        # (the reference's exact zeros are the rule's: rows and columns of excluded unknowns)
    assert np.array_equal(cov, cov.T), what
    assert e <= tol, (what, e, tol)
    if var is not None:
        assert np.array_equal(np.isinf(var), np.isinf(ref.rho_full)), what
        assert er <= tol, (what, er, tol)
    return e, er, tol


def test_tiny_initial_state(cv, golden_dir):
    """Case 1: `tiny` seed 7 at the initial state (P = 103, the last knot untouched): 32 selected + var_rho; the +inf and zero rules."""
    import cov_helpers as ch
    w = cv.synth.make_window("tiny", seed=7)
    sel = ch.tiny_selection(w)
    assert len(sel) == 32
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = reference(s, 0, w, sel)
        cov, var, sing = s.covariance(0, sel, rho=True)
    assert sing == 0
    assert ref.untouched[6 * (w.K - 1):6 * w.K].all() and not ref.untouched[:6 * (w.K - 1)].any()
    check(cov, var, ref, "tiny")
    assert np.isinf(cov[31, 31]) and not cov[31, :31].any() and not cov[:31, 31].any()
    assert np.isfinite(cov[:31, :31]).all() and (np.diag(cov)[:31] > 0).all() and np.isfinite(var).all() and (var > 0).all()
    fx = np.load(os.path.join(golden_dir, "cov_tiny_seed7.npz"))      # reported, not asserted: the oracle's H differs from the device's
    print(f"tiny vs the 50-digit fixture on the oracle's H: block {ch.cov_metric(cov, fx['block']):.3g}, var_rho {ch.rel_metric(var, fx['var_rho']):.3g}")


def test_config1_solved_64_scattered(cv, golden_dir):
    """Case 2: `config1` seed 1000 after a 15-iteration solve (P = 211: 14 tile rows, the last one partial): 64 selected, unsorted, over all
    tiles, 0 and P - 1 among them -- four selection tiles, all ten tile pairs of the Gram."""
    import cov_helpers as ch
    w = cv.synth.make_window("config1", seed=1000)
    rng = np.random.default_rng(5)
    per_tile = [int(16 * t + rng.integers(1, min(16, w.P - 1 - 16 * t))) for t in range(14)]   # one per tile row, neither 0 nor P - 1
    rest = [int(i) for i in rng.permutation(np.arange(1, w.P - 1)) if i not in per_tile]
    sel = [w.P - 1, 0] + per_tile + rest[:48]
    sel = [sel[i] for i in rng.permutation(64)]
    assert len(set(sel)) == 64 and {0, w.P - 1} <= set(sel) and len({i // 16 for i in sel}) == 14
    with cv.Solver() as s:
        b = [w.copy()]
        s.set_windows(b)
        s.solve(15)
        ref = reference(s, 0, b[0], sel)
        cov, var, sing = s.covariance(0, sel, rho=True)
    assert sing == 0
    check(cov, var, ref, "config1 solved")
    fx = np.load(os.path.join(golden_dir, "cov_config1_seed1000.npz"))
    with cv.Solver() as s:
        wf = w.copy()
        wf.quat[:] = fx["quat"]; wf.pos[:] = fx["pos"]; wf.bias[:] = fx["bias"]; wf.rho[:] = fx["rho"]; wf.ld = float(fx["ld"])
        s.set_windows([wf])
        covf, varf, _ = s.covariance(0, fx["sel"], rho=True)
    print(f"config1 vs the 50-digit fixture on the oracle's H: block {ch.cov_metric(covf, fx['block']):.3g}, var_rho {ch.rel_metric(varf, fx['var_rho']):.3g}")


def test_constant_unknowns_give_zero_rows(cv):
    """Case 3: `tiny` with fixed_upto = 3, lock_bg, fix_ld: constant selections give zero rows and columns, the rest matches the reference."""
    w = cv.synth.make_window("tiny", seed=7)
    w.fixed_upto = 3; w.lock_bg = True; w.fix_ld = True
    w.normalize()
    K, P = w.K, w.P
    sel = [P - 1, 6 * 3 + 1, 6 * 4 + 1, 6 * K + 1, 6 * K + 4, 0, 6 * (K - 2), 6 * (K - 2) + 5, 6 * K + 6 * (w.F - 1) + 2, 6 * K + 6 * (w.F - 1) + 3]
    const = [0, 1, 3, 5, 8]          # positions in sel of the constant ones
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        ref = reference(s, 0, w, sel)
        cov, var, sing = s.covariance(0, sel, rho=True)
    assert sing == 0
    check(cov, var, ref, "tiny, constants")
    free = [i for i in range(len(sel)) if i not in const]
    assert not cov[const, :].any() and not cov[:, const].any()
    assert (np.diag(cov)[free] > 0).all()


def mixed_batch(cv):
    """`tiny`, `config1`, a 16-frame window (K = 34, P = 301: the envelope panel path) and an IMU-only K = 27 window without landmarks
    (its first four knots held constant: inertial factors alone leave the position and the yaw of the spline undetermined)."""
    tiny = cv.synth.make_window("tiny", seed=7)
    c1 = cv.synth.make_window("config1", seed=1000)
    long16 = cv.synth.make_window("config1", seed=1400, F=16, L=60, M=750)
    pred = cv.Solver.predict_window(cv.synth.make_window("config1", seed=1200, F=10, dt_ns=40_000_000, with_prior=False), fixed_upto=3)
    pred.rho = pred.rho[:0]
    pred.normalize()
    ws = [tiny, c1, long16, pred]
    assert [w.P for w in ws] == [103, 211, 301, 223] and pred.L == 0
    rng = np.random.default_rng(11)
    sels = [[int(x) for x in rng.permutation(tiny.P)[:20]], [], [int(x) for x in rng.permutation(long16.P)[:40]] ,
            [int(x) for x in rng.permutation(6 * pred.K)[:17]]]
    return ws, sels


# The bit-for-bit comparisons run with query_harness.DET (order-fixed linearisation, and why); cases 1, 2, 3 and 5 run the default mode.


def run_mixed(cv, ws, sels):
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        return s.covariance_batch(sels, rho=True)


@pytest.fixture(scope="module")
def mixed(cv):
    """The mixed batch, its selections, the references from the device's own linearisation, and the plain call's outputs -- computed once."""
    ws, sels = mixed_batch(cv)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        refs = [reference(s, i, w, sel) for i, (w, sel) in enumerate(zip(ws, sels))]
        out = s.covariance_batch(sels, rho=True)
    return ws, sels, refs, out


def check_mixed(ws, sels, refs, out, what):
    covs, vars_, sing = out
    assert not sing.any(), (what, sing)
    for i, w in enumerate(ws):
        assert covs[i].shape == (len(sels[i]), len(sels[i])) and vars_[i].shape == (w.L,)
        check(covs[i], vars_[i], refs[i], f"{what} window {i} (P {w.P})")


def test_mixed_batch_one_call(cv, mixed):
    """Case 4: one call on the mixed batch; the n_sel differ, one is 0 with var_rho only."""
    ws, sels, refs, out = mixed
    check_mixed(ws, sels, refs, out, "mixed")


@pytest.mark.parametrize("env", [{"CTVIO_DENSE": "1"}, {"CTVIO_CHOL_COMPACT": "4"}], ids=["dense", "slots4"])
def test_mixed_batch_other_factorisations(cv, mixed, monkeypatch, env):
    """Case 4: the same batch with the dense sparsity plan and through the slot-indexed panel kernel with overflow tiles: same tolerance."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ws, sels, refs, _ = mixed
    check_mixed(ws, sels, refs, run_mixed(cv, ws, sels), str(env))


def test_mixed_batch_poisoned_scratch_same_bits(cv, mixed, monkeypatch):
    """Case 4: with CTVIO_POISON=1 (reused scratch and the tiles left of the envelope start as NaN) the call gives the same BITS."""
    ws, sels, _, out = mixed
    monkeypatch.setenv("CTVIO_POISON", "1")
    assert same_bits(run_mixed(cv, ws, sels), out)


def test_long_window_slot_kernel(cv):
    """Case 5: config5_spread @ 23 ms (P = 1003, L = 1000, two untouched knots) at the initial state: the last 32 touched unknowns + var_rho,
    through the slot-indexed panel kernel."""
    w = cv.synth.make_window("config5_spread", seed=1000, dt_ns=23_000_000)
    assert (w.P, w.L) == (1003, 1000)
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        H = s.linearize(0)[0]
        touched = np.nonzero(np.diag(H) != 0)[0]
        assert w.P - touched.shape[0] == 12        # two knots no factor touches
        sel = [int(i) for i in touched[-32:]]
        ref = reference(s, 0, w, sel)
        cov, var, sing = s.covariance(0, sel, rho=True)
    assert sing == 0
    check(cov, var, ref, "config5_spread @ 23 ms")


def test_repeatable_and_leaves_the_solve_alone(cv, mixed):
    """Case 6: two calls give equal bits; the single-window entry gives the batch entry's bits; state and graph captures unchanged by the
    call; a solve after the call equals, bit for bit, the same solve on a fresh handle that never asked for a covariance."""
    ws, sels, _, out = mixed
    with cv.Solver(**DET) as s:
        b = [w.copy() for w in ws]
        s.set_windows(b)
        s.solve(6, writeback=False)                 # (the graph is captured; the state has moved.  The iteration limit is part of the
                                                    #  kernels' arguments: the same limit below, or the pass is captured again anyway)
        cap, st = s.graph_captures, s.get_batch_state()
        o1 = s.covariance_batch(sels, rho=True)
        o2 = s.covariance_batch(sels, rho=True)
        assert same_bits(o1, o2)
        for i in range(len(ws)):
            c, v, sg = s.covariance(i, sels[i], rho=True)
            assert np.array_equal(c, o1[0][i]) and np.array_equal(v, o1[1][i], equal_nan=True) and sg == o1[2][i], i
        assert s.graph_captures == cap
        assert all(np.array_equal(x, y) for x, y in zip(st, s.get_batch_state()))
        sm = s.solve(6)
        assert s.graph_captures == cap
    with cv.Solver(**DET) as f:
        fb = [w.copy() for w in ws]
        f.set_windows(fb)
        f.solve(6, writeback=False)
        smf = f.solve(6)
        assert f.graph_captures == cap
    assert sm == smf
    for x, y in zip(b, fb):
        for a in ("quat", "pos", "bias", "rho"):
            assert np.array_equal(getattr(x, a), getattr(y, a)), a
        assert x.ld == y.ld
    # the first call of a fresh handle at the initial state: the bits of the module's plain call
    assert same_bits(run_mixed(cv, ws, sels), out)


def test_refusals_leave_the_handle_usable(cv):
    """Case 7: an entry outside [0, P), a duplicate, n_sel > 64 -> CTVIO_ERR_INVALID; a call before the upload -> CTVIO_ERR_STATE; the handle
    solves afterwards."""
    import ctypes as C
    w = cv.synth.make_window("tiny", seed=7)
    with cv.Solver() as s:
        lib = s._lib
        ns = np.array([1], np.int32); sel = np.array([0], np.int32); cov = np.zeros(1)
        assert lib.ctvio_covariance_batch(s._h, cv.capi._p(ns), cv.capi._p(sel), cv.capi._p(cov), None, None) == 4
        assert lib.ctvio_covariance(s._h, 0, 1, cv.capi._p(sel), cv.capi._p(cov), None, None) == 4
        s.set_windows([w.copy()])
        for bad in ([w.P], [-1], [3, 7, 3], list(range(65))):
            with pytest.raises(cv.capi.CtvioError, match="invalid"):
                s.covariance(0, bad)
            with pytest.raises(cv.capi.CtvioError, match="invalid"):
                s.covariance_batch([bad])
        cov, var, sing = s.covariance(0, [], rho=False)
        assert cov.shape == (0, 0) and var is None and sing == 0
        qh.check_usable_after(cv, w, s)


def test_adaptor_covariance_matches_python(cv, tmp_path):
    """Case 8: tests/covariance_demo.cpp through the C++ adaptor: the covariance of the newest touched knot and the last bias state equals
    the Python call on the same window to 1e-12 relative."""
    w0 = cv.synth.make_window("config1", seed=1005)
    K, F, L = w0.K, w0.F, w0.L
    knot = K - 2
    wa, rest = qh.run_demo(qh.build_demo("covariance_demo", tmp_path), w0, tmp_path, 15, knot)
    assert rest[0] == 1 and rest[1] == 12
    cov_cpp = rest[2:2 + 144].reshape(12, 12)
    ok2, v0, v1, refused = rest[146:150]
    assert ok2 == 1 and refused == 1
    sel = list(range(6 * knot, 6 * knot + 6)) + list(range(6 * K + 6 * (F - 1), 6 * K + 6 * F))
    with cv.Solver() as s:
        s.set_windows([wa])
        cov, var, sing = s.covariance(0, sel, rho=True)
    assert sing == 0 and np.isfinite(cov).all()
    scale = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    assert np.max(np.abs(cov_cpp - cov) / scale) <= 1e-12
    assert abs(v0 - var[0]) <= 1e-12 * var[0] and abs(v1 - var[1]) <= 1e-12 * var[1]
