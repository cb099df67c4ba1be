"""GPU (-m gpu): ctvio_options.deterministic = 2 -- order-fixed accumulation for every batch the solver accepts.  Windows whose packed Hessian
is not LDS resident (K > 25, up to P = 1024) assemble their pose block with one owner per entry (csrc/kernels_assemble.hpp: k_assemble_wide,
k_bias_rows_wide) in an order fixed by the upload plan; the LDS-resident ones run exactly as under deterministic = 1.  Against the oracle
(config 5, the three long shapes, a mixed batch, the normal equations), bit for bit from run to run (two handles, one handle twice, profiling,
no graph, split linearisation, poisoned scratch), across a marginalisation slide and through ctvio_solve_sharded."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_gpu_long_windows import ITERS, LONG, check, long_window  # noqa: E402

import prior_helpers as ph  # noqa: E402

C5_SEEDS = [1011 + i for i in range(8)]


def config5_batch(cv):
    return [cv.synth.make_window("config5", seed=s) for s in C5_SEEDS]


def long_batch(cv):
    return [long_window(cv, c, dt) for c, dt in LONG]


def run(cv, ws, iters, monkeypatch=None, env=None, twice=False, profiling=False, **kw):
    """Solve copies of ws on a fresh handle; returns (states, summaries, ctvio_linearize of every window at the result).  twice: solve,
    restore the snapshot taken before, solve again on the same handle -- the second solve is returned."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        batch = [w.copy() for w in ws]
        with cv.Solver(**kw) as s:
            s.set_windows(batch)
            if profiling:
                s.set_profiling(True)
            if twice:
                s.snapshot_state()
                s.solve(iters, writeback=False)
                s.restore_state()
            sms = s.solve(iters)
            lin = [s.linearize(i) for i in range(len(batch))]
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k)
    states = [np.concatenate([w.quat.ravel(), w.pos.ravel(), w.bias.ravel(), w.rho.ravel(), [w.ld]]) for w in batch]
    return states, sms, lin


def assert_same_bits(a, b, what):
    sa, ma, la = a
    sb, mb, lb = b
    for i in range(len(sa)):
        assert np.array_equal(sa[i], sb[i]), (what, i, np.abs(sa[i] - sb[i]).max())
        assert ma[i] == mb[i], (what, i)
        for x, y in zip(la[i][:4], lb[i][:4]):
            assert np.array_equal(x, y), (what, i)
        assert la[i][4] == lb[i][4], (what, i)


def test_config5_accepted_vs_oracle(cv, oracle_solved):
    """8 config-5 windows (K 64, P 571): refused by deterministic = 1, accepted by 2, every window against the oracle's 15-iteration solve with
    the bar of test_config5_timed_shape_vs_oracle."""
    uniq = config5_batch(cv)
    assert all(w.P == 571 for w in uniq)
    with cv.Solver(deterministic=1) as s:
        with pytest.raises(cv.capi.CtvioError):
            s.set_windows([w.copy() for w in uniq])
    refs, sms_o = zip(*[oracle_solved("config5", sd) for sd in C5_SEEDS])
    batch = [w.copy() for w in uniq]
    with cv.Solver(deterministic=2) as s:
        s.set_windows(batch)
        sms = s.solve(15)
    for i, sm in enumerate(sms):
        so = sms_o[i]
        assert (sm["iterations"], sm["num_successful"], sm["num_unsuccessful"]) == (so.iterations, so.num_successful, so.num_unsuccessful), i
        assert sm["final_cost"] == pytest.approx(so.final_cost, rel=1e-9), i
        assert cv.rel_state_error(batch[i], refs[i])["state"] < 1e-6, i


def test_long_windows_accepted_vs_oracle(cv, oracle):
    """config2 @ 10 ms (P 709), config5_spread @ 25 ms (P 937) and @ 23 ms (P 1003) as one batch under deterministic = 2, at
    test_gpu_long_windows' ITERS with its check()."""
    ws = long_batch(cv)
    assert [w.P for w in ws] == [709, 937, 1003]
    batch = [w.copy() for w in ws]
    with cv.Solver(deterministic=2) as s:
        s.set_windows(batch)
        sms = s.solve(ITERS)
    for i, w in enumerate(ws):
        ref = w.copy()
        so = oracle.OracleWindow(ref).solve(ITERS)
        print(f"P {w.P}: state error {check(cv, sms[i], so, batch[i], ref, i):.2e}")


@pytest.mark.parametrize("shape", ["config5", "long"])
def test_bitwise_run_to_run(cv, monkeypatch, shape):
    """15 iterations, the same bits (states, summaries, ctvio_linearize at the result) from: two handles, one handle twice (snapshot /
    restore), profiling on, no hipGraph, CTVIO_SPLIT_LINEARIZE=1."""
    ws = config5_batch(cv) if shape == "config5" else long_batch(cv)
    base = run(cv, ws, 15, deterministic=2)
    assert_same_bits(base, run(cv, ws, 15, deterministic=2), "second handle")
    assert_same_bits(base, run(cv, ws, 15, deterministic=2, twice=True), "same handle twice")
    assert_same_bits(base, run(cv, ws, 15, deterministic=2, profiling=True), "profiling")
    assert_same_bits(base, run(cv, ws, 15, deterministic=2, use_graph=False), "no graph")
    assert_same_bits(base, run(cv, ws, 15, monkeypatch, {"CTVIO_SPLIT_LINEARIZE": "1"}, deterministic=2), "split linearisation")


@pytest.mark.parametrize("poison", ["1", "2"])
def test_poisoned_scratch_same_bits(cv, monkeypatch, poison):
    """CTVIO_POISON: every reused double scratch segment starts as a pattern -- the wide windows' Hpp (outside the per-upload zeroed region)
    is written entry by entry, so the bits do not change."""
    ws = config5_batch(cv)[:4] + long_batch(cv)[:1]
    base = run(cv, ws, 15, deterministic=2)
    assert_same_bits(base, run(cv, ws, 15, monkeypatch, {"CTVIO_POISON": poison}, deterministic=2), f"poison {poison}")


def mixed_windows(cv):
    tiny = cv.synth.make_window("tiny", seed=11)
    big = cv.synth.make_window("config1", seed=1200, F=10, dt_ns=40_000_000, with_prior=False)    # K = 27
    pred = cv.Solver.predict_window(big, fixed_upto=-1)
    assert pred.V == 0 and pred.K >= 25
    c5 = cv.synth.make_window("config5", seed=1011)
    c2 = cv.synth.make_window("config2", seed=1000)
    assert c2.pn > 0
    return [tiny, pred, c5, c2]


def test_mixed_batch(cv, oracle, monkeypatch):
    """The tiny window and the IMU-only K = 27 predict window that deterministic = 1 refuses (test_gpu_parity), a config-5 window and a
    config-2 window with a prior, in one batch: accepted, every window against the oracle, two runs bitwise equal."""
    ws = mixed_windows(cv)
    with cv.Solver(deterministic=1) as s:
        with pytest.raises(cv.capi.CtvioError):
            s.set_windows([w.copy() for w in ws])
    batch = [w.copy() for w in ws]
    with cv.Solver(deterministic=2) as s:
        s.set_windows(batch)
        sms = s.solve(8)
    for i, w in enumerate(ws):
        wo = w.copy()
        so = oracle.OracleWindow(wo).solve(8)
        assert (sms[i]["iterations"], sms[i]["num_successful"]) == (so.iterations, so.num_successful), i
        assert sms[i]["final_cost"] == pytest.approx(so.final_cost, rel=1e-8), i
        assert cv.rel_state_error(batch[i], wo)["state"] < 1e-6, i
    assert_same_bits(run(cv, ws, 8, deterministic=2), run(cv, ws, 8, deterministic=2), "mixed")


def test_lds_resident_batches_unchanged(cv):
    """A batch deterministic = 1 accepts (ragged config-2 / tiny / config-1 shapes) gives identical bits under 1 and 2."""
    ws = [cv.synth.make_window("config2", seed=1000 + i) for i in range(3)] + [cv.synth.make_window("tiny", seed=7),
                                                                               cv.synth.make_window("config1", seed=1001)]
    assert_same_bits(run(cv, ws, 15, deterministic=1), run(cv, ws, 15, deterministic=2), "1 vs 2")


def test_linearize_parity_vs_oracle(cv, oracle):
    """ctvio_linearize of wide windows under deterministic = 2: Hpp, W, Hll, g and cost against the oracle's normal equations
    (test_gpu_prior.check_linearize) -- config 5, a P 709 window, and a P 709 window whose prior covers every pose unknown (pn 709 > 600)."""
    from test_gpu_prior import check_linearize
    c5 = cv.synth.make_window("config5", seed=1012)
    lw = long_window(cv, "config2", 10)
    dense = ph.dense_prior_window(long_window(cv, "config2", 10, seed=1001), 77, full=True)
    assert dense.pn > 600
    ws = [c5, lw, dense]
    with cv.Solver(deterministic=2) as s:
        s.set_windows([w.copy() for w in ws])
        for i, w in enumerate(ws):
            check_linearize(s, oracle, i, w, f"wide {i}")


def slide_once(cv):
    from chain_helpers import prior_arrays, split_by_landmarks
    w = cv.synth.make_window("config5", seed=1013)
    keep = np.arange(w.L) >= w.L // 2
    wR, wD, _, _ = split_by_landmarks(w, keep)
    for a in ("pJ0", "pr0", "p_kind", "p_index", "p_off", "p_x0"):
        setattr(wD, a, np.array(getattr(w, a), copy=True))
    wD.normalize()
    with cv.Solver(deterministic=2) as s:
        d = [wD.copy()]
        s.set_windows(d)
        s.solve(15)
        Hpp = s.linearize(0)[0]
        role = np.where(np.arange(wD.N) >= wD.P, 1, np.where(np.concatenate([np.diag(Hpp), np.ones(wD.L)]) > 0, 0, -1)).astype(np.int8)
        (kept, J0, r0), = s.marginalize_batch([role])
        wR.pJ0, wR.pr0, wR.p_kind, wR.p_index, wR.p_off, wR.p_x0 = prior_arrays(wR, kept, J0, r0)
        wR.normalize()
        nxt = [wR.copy()]
        s.set_windows(nxt)
        sm = s.solve(15)
    return d[0], kept, J0, r0, nxt[0], sm


def test_slide_bitwise(cv):
    """config-5 solve -> ctvio_marginalize_batch -> the next window solved with that prior, twice: n_keep, kept, J0, r0 and both final states
    bitwise equal."""
    a, b = slide_once(cv), slide_once(cv)
    assert len(a[1]) == len(b[1]) and len(a[1]) > 0
    for x, y in zip(a[1:4], b[1:4]):
        assert np.array_equal(x, y)
    for wa, wb in ((a[0], b[0]), (a[4], b[4])):
        for f in ("quat", "pos", "bias", "rho"):
            assert np.array_equal(getattr(wa, f), getattr(wb, f)), f
        assert wa.ld == wb.ld
    assert a[5] == b[5]


def test_sharded_mixed_batch(cv, oracle, monkeypatch):
    """ctvio_solve_sharded with two shards on one device (CTVIO_SHARD_OVERSUBSCRIBE=1) and deterministic = 2 on the mixed batch: the option
    reaches the shard handles, every window against the oracle."""
    lib = cv.capi.load_library()
    ws = [w.copy() for w in mixed_windows(cv)]
    n = len(ws)
    keep = []
    arr = (cv.capi.CWindow * n)()
    for i, w in enumerate(ws):
        arr[i] = cv.capi.to_cwindow(w, keep)
    K = sum(w.K for w in ws); F = sum(w.F for w in ws); L = sum(w.L for w in ws)
    opt = cv.capi.Options()
    lib.ctvio_default_options(C.byref(opt))
    opt.deterministic = 2
    sm = (cv.capi.Summary * n)()
    q = np.zeros((K, 4)); p = np.zeros((K, 3)); b = np.zeros((F, 6)); r = np.zeros(L); ld = np.zeros(n)
    monkeypatch.setenv("CTVIO_SHARD_OVERSUBSCRIBE", "1")
    try:
        assert lib.ctvio_shards_used(2, n) == 2
        cv.capi.check(lib.ctvio_solve_sharded(C.byref(opt), 2, n, C.cast(arr, C.c_void_p), 8, C.cast(sm, C.c_void_p),
                                              cv.capi._p(q), cv.capi._p(p), cv.capi._p(b), cv.capi._p(r), cv.capi._p(ld)))
    finally:
        lib.ctvio_sharded_release()
    k0 = f0 = l0 = 0
    for i, w in enumerate(ws):
        got = w.copy()
        got.quat[:] = q[k0:k0 + w.K]; got.pos[:] = p[k0:k0 + w.K]; got.bias[:] = b[f0:f0 + w.F]; got.rho[:] = r[l0:l0 + w.L]; got.ld = float(ld[i])
        wo = w.copy()
        so = oracle.OracleWindow(wo).solve(8)
        s = sm[i].as_dict()
        assert (s["iterations"], s["num_successful"]) == (so.iterations, so.num_successful), i
        assert s["final_cost"] == pytest.approx(so.final_cost, rel=1e-8), i
        assert cv.rel_state_error(got, wo)["state"] < 1e-6, i
        k0 += w.K; f0 += w.F; l0 += w.L
