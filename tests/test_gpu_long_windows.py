"""GPU (-m gpu): windows with 591 < P <= 1024 trajectory unknowns -- the panel Cholesky's slot-indexed variant (csrc/kernels_solve.hpp:
k_cholesky_solve<NW, true>), whose LDS holds only the tiles that take part in a panel and whose overflow tiles are read back from S.  Against
the oracle iterate for iterate: long ragged windows, dense envelopes (CTVIO_DENSE=1, a small forced slot budget), mixed and large batches,
a window that carries a real prior from ctvio_marginalize_batch; bit for bit against today's panel kernel; the refusal beyond 1024."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# (config, knot spacing in ms): P = 709, 937, 1003
LONG = [("config2", 10), ("config5_spread", 25), ("config5_spread", 23)]
# LM iterations compared against the oracle.  Short knots make these windows weakly determined: the ORACLE's own 15-iteration solve moves
# when the start state is scaled by 1 + 1e-13 -- config2 @ 10 ms by 6.6e-2 in the state and 5.9e-3 in the cost, config5_spread @ 25 ms by
# 1.5e-5 already after 5 iterations (config5_spread @ 23 ms: 1.8e-13 after 15).  After 4 iterations the three move by 6e-12, 4e-9 and
# < 1e-12: that is where a different summation order can be held to the 1e-9 / 1e-6 bar.
ITERS = 4


def long_window(cv, cfg, dt_ms, seed=1000):
    return cv.synth.make_window(cfg, seed=seed, dt_ns=dt_ms * 1_000_000)


@pytest.fixture(scope="module")
def long_solved(cv, oracle):
    """(config, dt) -> (window as given, the oracle's solved copy, its summary); each solved once per module."""
    cache = {}

    def get(cfg, dt_ms):
        if (cfg, dt_ms) not in cache:
            w = long_window(cv, cfg, dt_ms)
            ref = w.copy()
            so = oracle.OracleWindow(ref).solve(ITERS)
            cache[(cfg, dt_ms)] = (w, ref, so)
        return cache[(cfg, dt_ms)]
    return get


def check(cv, sm, so, got, ref, what, tol=1e-6):
    assert (sm["iterations"], sm["num_successful"], sm["num_unsuccessful"]) == (so.iterations, so.num_successful, so.num_unsuccessful), what
    assert sm["final_cost"] == pytest.approx(so.final_cost, rel=1e-9), what
    err = cv.rel_state_error(got, ref)["state"]
    assert err < tol, (what, err)
    return err


def solve_batch(cv, ws, iters=ITERS, **kw):
    batch = [w.copy() for w in ws]
    with cv.Solver(**kw) as s:
        s.set_windows(batch)
        sms = s.solve(iters)
    return batch, sms


def test_long_windows_vs_oracle(cv, long_solved):
    """config2 @ 10 ms (P 709), config5_spread @ 25 ms (P 937) and @ 23 ms (P 1003) as one ragged batch."""
    cases = [long_solved(c, dt) for c, dt in LONG]
    assert [w.P for w, _, _ in cases] == [709, 937, 1003]
    batch, sms = solve_batch(cv, [w for w, _, _ in cases])
    for i, ((w, ref, so), sm) in enumerate(zip(cases, sms)):
        print(f"P {w.P}: state error {check(cv, sm, so, batch[i], ref, i):.2e}")


@pytest.mark.parametrize("env", [{"CTVIO_DENSE": "1"}, {"CTVIO_CHOL_COMPACT": "4"}], ids=["dense", "slots4"])
def test_long_windows_overflow_vs_oracle(cv, long_solved, monkeypatch, env):
    """The same shapes with more tiles per panel than the LDS holds: the dense envelope (43 / 57 / 61 tiles against 35 slots) and a forced
    budget of 4 slots -- the overflow route on real data."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cases = [long_solved(c, dt) for c, dt in LONG]
    batch, sms = solve_batch(cv, [w for w, _, _ in cases])
    for i, ((w, ref, so), sm) in enumerate(zip(cases, sms)):
        print(f"{env} P {w.P}: state error {check(cv, sm, so, batch[i], ref, i):.2e}")


def test_slot_variant_bitwise_equals_panel_kernel(cv, monkeypatch):
    """A deterministic config-2 batch through today's panel kernel (CTVIO_CHOL_TILES=0) and through its slot-indexed variant, with every
    tile in LDS and with budgets that overflow (the window needs 9 slots): the same bits."""
    ws = [cv.synth.make_window("config2", seed=1000 + i) for i in range(8)]
    monkeypatch.setenv("CTVIO_CHOL_TILES", "0")
    runs = {}
    for compact in (None, "1", "5", "2"):
        if compact is None:
            monkeypatch.delenv("CTVIO_CHOL_COMPACT", raising=False)
        else:
            monkeypatch.setenv("CTVIO_CHOL_COMPACT", compact)
        batch, sms = solve_batch(cv, ws, 15, deterministic=1)
        runs[compact] = (batch, sms)
    base_b, base_s = runs[None]
    for compact, (b, sms) in runs.items():
        for i in range(len(ws)):
            assert sms[i] == base_s[i], (compact, i)
            for a in ("quat", "pos", "bias", "rho"):
                assert np.array_equal(getattr(b[i], a), getattr(base_b[i], a)), (compact, i, a)
            assert b[i].ld == base_b[i].ld, (compact, i)


def test_mixed_small_and_long_windows(cv, oracle_solved, long_solved):
    """211-unknown windows and P 937 windows in one batch: the long windows decide the kernel for all."""
    w937, ref937, so937 = long_solved("config5_spread", 25)
    refs, sos = zip(*[oracle_solved("config2", 1000 + i, ITERS) for i in range(2)])
    small = [cv.synth.make_window("config2", seed=1000 + i) for i in range(2)]
    batch, sms = solve_batch(cv, [small[0], w937, small[1], w937])
    check(cv, sms[0], sos[0], batch[0], refs[0], "config2 0")
    check(cv, sms[2], sos[1], batch[2], refs[1], "config2 1")
    check(cv, sms[1], so937, batch[1], ref937, "P 937 a")
    check(cv, sms[3], so937, batch[3], ref937, "P 937 b")


def test_64_long_windows(cv, long_solved):
    """64 copies of the P 937 shape: the 2 x 2 blocked Schur tile kernel and the 8-wave selection; first and last copy against the oracle.
    Prints the time of a 15-iteration solve of one window and of the 64."""
    w, ref, so = long_solved("config5_spread", 25)
    times = {}
    for n in (1, 64):
        with cv.Solver() as s:
            s.set_windows([w.copy() for _ in range(n)])
            s.solve(15, writeback=False)              # warm-up (allocation, graph capture)
            s.set_windows([w.copy() for _ in range(n)])
            t0 = time.perf_counter()
            s.solve(15, writeback=False)
            times[n] = time.perf_counter() - t0
            batch = [w.copy() for _ in range(n)]
            s.set_windows(batch)
            sms = s.solve(ITERS)
        check(cv, sms[0], so, batch[0], ref, f"{n}: first")
        check(cv, sms[-1], so, batch[-1], ref, f"{n}: last")
    print(f"P 937 solve (15 iterations): one window {1e3 * times[1]:.1f} ms, 64 windows {1e3 * times[64]:.1f} ms")


def test_chained_window_with_dense_prior(cv, oracle):
    """A prior from ctvio_marginalize_batch's blocked path (more than 591 kept unknowns) on a P 937 window: its envelope is dense over the
    prior's blocks, more tiles than the LDS holds.  The next window solved with that prior against the oracle solving it with the same prior.
    chain_case's split (the first half of the landmarks) with the inertial factors and the gauge anchor on the MARGINALISED side, so that the
    prior reaches every pose unknown (the visual blocks alone touch 93 of the 125 knots: n 559)."""
    from chain_helpers import split_by_landmarks, prior_arrays
    w = long_window(cv, "config5_spread", 25, seed=1500)
    keep = np.arange(w.L) >= w.L // 2
    wR, wD, _, _ = split_by_landmarks(w, keep)        # wD: the dropped landmarks + IMU + bias chain; wR: the kept landmarks' visual blocks
    for a in ("pJ0", "pr0", "p_kind", "p_index", "p_off", "p_x0"):
        setattr(wD, a, np.array(getattr(w, a), copy=True))
    wD.normalize()
    with cv.Solver() as s:
        s.set_windows([wD.copy()])
        Hpp = s.linearize(0)[0]
        role = np.where(np.arange(wD.N) >= wD.P, 1, np.where(np.concatenate([np.diag(Hpp), np.ones(wD.L)]) > 0, 0, -1)).astype(np.int8)
        (kept, J0, r0), = s.marginalize_batch([role])
        assert not s.marginalize_ran_on_host()
    m, n = int((role == 1).sum()), int((role == 0).sum())
    assert m > 180 and len(kept) > 591, (m, n, len(kept))
    wR.pJ0, wR.pr0, wR.p_kind, wR.p_index, wR.p_off, wR.p_x0 = prior_arrays(wR, kept, J0, r0)
    wR.normalize()
    env = cv.packer.reduced_system_envelope(wR)
    assert cv.packer.chol_panel_slots(wR.P, env) > 35
    ref = wR.copy()
    so = oracle.OracleWindow(ref).solve(ITERS)
    batch, sms = solve_batch(cv, [wR])
    err = check(cv, sms[0], so, batch[0], ref, "chained")
    print(f"chained P {wR.P} (m {m} / n {n}, {len(kept)} kept): state error {err:.2e}")


def test_refusal_beyond_1024(cv, oracle_solved):
    """config5_spread @ 20 ms (P 1117) is refused with a message naming the bound; the handle then still solves a valid batch."""
    big = long_window(cv, "config5_spread", 20)
    assert big.P > 1024
    ref, so = oracle_solved("config2", 1000, ITERS)
    with cv.Solver() as s:
        with pytest.raises(cv.capi.CtvioError, match="1024"):
            s.set_windows([big.copy()])
        batch = [cv.synth.make_window("config2", seed=1000)]
        s.set_windows(batch)
        sms = s.solve(ITERS)
    check(cv, sms[0], so, batch[0], ref, "after the refusal")


def test_sharded_entry_long_windows(cv, long_solved):
    """ctvio_solve_sharded shares the upload: the three long shapes through it (one device) against the oracle."""
    import ctypes as C
    lib = cv.capi.load_library()
    cases = [long_solved(c, dt) for c, dt in LONG]
    ws = [w.copy() for w, _, _ in cases]
    n = len(ws)
    keep = []
    arr = (cv.capi.CWindow * n)()
    for i, w in enumerate(ws):
        arr[i] = cv.capi.to_cwindow(w, keep)
    K = sum(w.K for w in ws); F = sum(w.F for w in ws); L = sum(w.L for w in ws)
    opt = cv.capi.Options()
    lib.ctvio_default_options(C.byref(opt))
    sm = (cv.capi.Summary * n)()
    q = np.zeros((K, 4)); p = np.zeros((K, 3)); b = np.zeros((F, 6)); r = np.zeros(L); ld = np.zeros(n)
    try:
        cv.capi.check(lib.ctvio_solve_sharded(C.byref(opt), 1, n, C.cast(arr, C.c_void_p), ITERS, C.cast(sm, C.c_void_p),
                                              cv.capi._p(q), cv.capi._p(p), cv.capi._p(b), cv.capi._p(r), cv.capi._p(ld)))
    finally:
        lib.ctvio_sharded_release()
    k0 = f0 = l0 = 0
    for i, (w, ref, so) in enumerate(cases):
        got = w.copy()
        got.quat[:] = q[k0:k0 + w.K]; got.pos[:] = p[k0:k0 + w.K]; got.bias[:] = b[f0:f0 + w.F]; got.rho[:] = r[l0:l0 + w.L]; got.ld = float(ld[i])
        check(cv, sm[i].as_dict(), so, got, ref, f"sharded {i}")
        k0 += w.K; f0 += w.F; l0 += w.L
