"""GPU (-m gpu): the marginalisation prior (r = r0 + J0 dx over the kept blocks, MarginalizationFactor) on every device path, against the
fp64 oracle, with the dense all-kind priors of tests/prior_helpers.py (non-symmetric J0, shuffled offsets, BG / BA / LD blocks,
negated-quaternion x0, priors over every pose unknown and over constant blocks).  The paths (ctvio.hip: launch_linearize /
launch_assemble):

  merged store    deterministic, <= 128 windows, not profiling: k_pre_linearize -> misc_body<64>, prior_H / prior_g via pinv in the tail
  split store     deterministic + CTVIO_SPLIT_LINEARIZE=1 (or profiling): k_misc with store = 1
  accumulate      deterministic = 0 (or > 64 windows): k_misc with store = 0, with_imu = 1, atomics into Hpp / g
  accumulate+band a window with K > 25 in the batch: k_misc with with_imu = 2, the band behind dx at ((maxPn + 1) & ~1)
  cost only       ctvio_cost: k_misc(COST_AT_X); ctvio_residual_summary: k_residual_summary

Switches (CTVIO_*) are read once per solver handle: the environment is set before the handle is created."""
import numpy as np
import pytest

import prior_helpers as ph

pytestmark = pytest.mark.gpu


def _ragged_batch(cv):
    """~12 windows: config1 / config2 / tiny, with no prior, a small dense prior and a prior over every pose unknown; one window (tiny)
    and one (config1) with constant blocks in their priors."""
    ws = []
    for i, (cfg, kind) in enumerate([("tiny", None), ("tiny", "small"), ("tiny", "full"), ("config1", "small"), ("config1", "full"),
                                     ("config1", None), ("config2", "small"), ("config2", "full"), ("tiny", "small"), ("config2", None)]):
        w = cv.synth.make_window(cfg, seed=2100 + i)
        pr = None if kind is None else ph.make_prior(w, 50 + i, full=(kind == "full"))
        ws.append(ph.with_prior(w, pr))
    c = cv.synth.make_window("tiny", seed=2150)
    c.fixed_upto = 1
    kc = np.zeros(c.K, np.uint8); kc[5] = 1
    c.knot_const = kc
    c.lock_bg = True; c.fix_ld = True
    ws.append(ph.dense_prior_window(c.normalize(), 61, with_const=True))
    c = cv.synth.make_window("config1", seed=2151)
    kc = np.zeros(c.K, np.uint8); kc[[0, 9]] = 1
    c.knot_const = kc
    c.lock_ba = True
    ws.append(ph.dense_prior_window(c.normalize(), 62, with_const=True, n_bias=4))
    assert any(w.pn == w.P for w in ws) and any(w.pn == 0 for w in ws)
    return ws


def _band_window(cv):
    """K = 27 (packed Hessian not in LDS: k_misc runs the IMU band) with a prior SMALLER than the batch's largest one."""
    w = cv.synth.make_window("config1", seed=2170, F=10, dt_ns=40_000_000)
    assert w.K > 25
    return ph.dense_prior_window(w, 70, n_knots=3, n_bias=2)


_ORACLE = {}


def _oracle_normal(oracle, w):
    key = id(w)
    if key not in _ORACLE:
        ow = oracle.OracleWindow(w.copy())
        H, g, cost = ow.build_normal()
        _ORACLE[key] = (w, H, g, cost, ow.active_mask())
    return _ORACLE[key][1:]


def check_linearize(s, oracle, wid, w, tag):
    """The device's normal equations of window `wid` (a copy of w) against the oracle's: the metric and bounds of
    test_random_factor_structures_match_oracle (scaled 1e-10 on H / W / g, rel 1e-12 on the cost), over the active unknowns."""
    H, g, cost, act = _oracle_normal(oracle, w)
    P = w.P
    Hg, Wg, Hllg, gg, costg = s.linearize(wid)
    assert costg == pytest.approx(cost, rel=1e-12), (tag, wid)
    sc = np.sqrt(np.maximum(np.diag(H), 1e-30))
    ap, al = act[:P], act[P:]
    dH = np.abs((Hg - H[:P, :P]) / np.outer(sc[:P], sc[:P]))
    assert dH[np.ix_(ap, ap)].max() < 1e-10, (tag, wid)
    if w.L and al.any():
        dW = np.abs((Wg - H[:P, P:]) / np.outer(sc[:P], sc[P:]))
        assert dW[np.ix_(ap, al)].max() < 1e-10, (tag, wid)
        obs = al & (np.diag(H)[P:] > 0)
        if obs.any():
            assert np.abs(Hllg[obs] / np.diag(H)[P:][obs] - 1).max() < 1e-10, (tag, wid)
    gs = np.maximum(sc, 1e-12)
    assert np.abs((gg - g) / gs)[act].max() < 1e-10 * max(np.abs(g / gs)[act].max(), 1.0), (tag, wid)


@pytest.fixture(scope="module")
def batch(cv):
    return _ragged_batch(cv)


@pytest.mark.parametrize("path", ["merged_store", "split_store", "accumulate", "accumulate_band"])
def test_linearize_parity_on_every_path(cv, oracle, batch, path, monkeypatch):
    """Every window's H, W, g and cost through each linearising path of the prior (see the module docstring) against the oracle.  The
    path is selected by what is asserted here: deterministic = 1 (refused unless the store-semantics tail can take the batch) with at
    most 128 windows and profiling off = merged; + CTVIO_SPLIT_LINEARIZE=1 = split; deterministic = 0 = accumulate; a K > 25 window
    in the batch = the band (its pn below the batch's maxPn, so the band offset comes from maxPn, not from the window's own pn)."""
    ws = list(batch)
    det = 1
    if path == "split_store":
        monkeypatch.setenv("CTVIO_SPLIT_LINEARIZE", "1")
    if path.startswith("accumulate"):
        det = 0
    if path == "accumulate_band":
        big = _band_window(cv)
        maxpn = max(w.pn for w in ws)
        assert 0 < big.pn < maxpn and big.K > 25
        # the band fits the launch's LDS (ctvio.hip launch_assemble: dx + 144 maxK doubles <= 150 KB)
        assert (((maxpn + 1) & ~1) + 144 * big.K) * 8 <= 150 * 1024
        ws = ws[:6] + [big] + ws[6:]
        det = -1                                   # the default: a K > 25 window takes the batch to the accumulate path
    assert len(ws) <= 128 and all(w.K <= 25 for w in ws if det == 1)
    with cv.Solver(deterministic=det) as s:
        s.set_windows([w.copy() for w in ws])
        for i, w in enumerate(ws):
            check_linearize(s, oracle, i, w, path)


def test_linearize_parity_accumulate_large_batch(cv, oracle, batch):
    """The accumulate path on > 128 windows (copies of the ragged batch): the first and the last copy against the oracle."""
    reps = 128 // len(batch) + 1
    ws = [w for _ in range(reps) for w in batch]
    assert len(ws) > 128
    with cv.Solver() as s:                         # (> 64 windows: the default is the accumulate path)
        s.set_windows([w.copy() for w in ws])
        for i, w in enumerate(batch):
            check_linearize(s, oracle, i, w, "large-first")
            check_linearize(s, oracle, len(ws) - len(batch) + i, w, "large-last")


def test_cost_and_residual_summary(cv, oracle, batch):
    """ctvio_cost (k_misc(COST_AT_X)) against the oracle's cost, rel 1e-12; the prior sums of ctvio_residual_summary (k_residual_summary)
    against |oracle prior_residual()|, rel 1e-9 -- on non-symmetric J0 with negated-quaternion blocks."""
    with cv.Solver() as s:
        s.set_windows([w.copy() for w in batch])
        for i, w in enumerate(batch):
            ow = oracle.OracleWindow(w.copy())
            assert s.cost(i) == pytest.approx(ow.cost(), rel=1e-12), i
            rs = s.residual_summary(i)
            sums, _ = rs["prior"]
            assert sums.shape == (w.pn,), i
            if w.pn:
                assert ph.has_negated_rotation(w) and not np.allclose(w.pJ0, w.pJ0.T), i
                r, _ = ow.prior_residual()
                assert np.abs(sums - np.abs(r)).max() <= 1e-9 * np.abs(r).max(), i


@pytest.mark.parametrize("det", [1, 0])
def test_lm_step_with_dense_prior(cv, oracle, det):
    """lm_step(wid, 1e4) against the oracle's dense solve, with the bounds of test_lm_step_matches_oracle, on a config1 window with a
    dense prior over every pose unknown and one with a small dense prior (store-semantics and accumulate assembly)."""
    base = cv.synth.make_window("config1", seed=1000)
    base.ld = 1.1e-5
    ws = [ph.dense_prior_window(base, 80, full=True), ph.dense_prior_window(base, 81)]
    for w in ws:
        d_o, mc_o = oracle.OracleWindow(w.copy()).lm_step(1e4, use_schur=False)
        with cv.Solver(deterministic=det) as s:
            s.set_windows([w.copy()])
            d_g, mc_g = s.lm_step(0, 1e4)
        assert np.abs(d_g - d_o).max() <= 1e-8 * np.abs(d_o).max()
        assert mc_g == pytest.approx(mc_o, rel=1e-9)


SOLVE_CASES = [("config1", 1000), ("config1", 1001), ("config2", 1000), ("config2", 1001), ("config3", 1000), ("config3", 1001),
               ("tumrs", 1000), ("tumrs", 1001)]


@pytest.fixture(scope="module")
def solved(cv, oracle):
    """8 distinct windows with dense priors near their state (one of them over every pose unknown) and their oracle solves."""
    out = []
    for i, (cfg, seed) in enumerate(SOLVE_CASES):
        w = ph.dense_prior_window(cv.synth.make_window(cfg, seed=seed), 90 + i, full=(i == 2))
        wo = w.copy()
        out.append((w, wo, oracle.OracleWindow(wo).solve(15)))
    return out


@pytest.mark.parametrize("mode", ["default", "accumulate_200"])
def test_solve_parity_with_dense_priors(cv, solved, mode):
    """Same iteration count, final cost within rel 1e-9 and state within 1e-6 of the oracle: the 8 windows alone (the default mode: the
    merged store path) and 25 copies of them (200 windows: the accumulate path), every window checked."""
    reps = 1 if mode == "default" else 25
    src = [x for _ in range(reps) for x in solved]
    with cv.Solver() as s:
        ws = [w.copy() for w, _, _ in src]
        s.set_windows(ws)
        sms = s.solve(15)
    for i, (wg, sm, (_, wo, sm_o)) in enumerate(zip(ws, sms, src)):
        assert sm["iterations"] == sm_o.iterations, (mode, i)
        assert sm["final_cost"] == pytest.approx(sm_o.final_cost, rel=1e-9), (mode, i)
        assert cv.rel_state_error(wg, wo)["state"] < 1e-6, (mode, i)


def _prior_only_window(cv, seed):
    """No IMU, no visual blocks: a bias chain of 11 links (66 terms) and a prior over every pose unknown (pn = P = 145) -- the window's
    whole cost is the misc share (bias chain + prior), so its cost bits are those of that reduction alone."""
    rng = np.random.default_rng(seed)
    K, F = 12, 12
    q = rng.normal(size=(K, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w = cv.Window(t0_ns=0, dt_ns=50_000_000, quat=q, pos=rng.normal(size=(K, 3)), bias=rng.normal(0.0, 0.01, (F, 6)), rho=np.zeros(0), ld=1.5e-5,
                  bc_i=np.arange(F - 1), bc_j=np.arange(1, F), bc_w=rng.uniform(50.0, 200.0, (F - 1, 6))).normalize()
    return ph.dense_prior_window(w, seed + 1, full=True)


def test_deterministic_bitwise_across_paths(cv, monkeypatch):
    """deterministic = 1 promises equal bits for two runs of the same batch (include/ctvio.h) -- also when the launch shape changes:
    plain (merged store path, misc_body<64> in k_pre_linearize), profiled (split store path, k_misc with 256 threads), and a handle
    created under CTVIO_SPLIT_LINEARIZE=1.  Summaries, every state entry and every window's linearisation cost must be identical.  Two
    prior-only windows carry a cost that is the misc share alone (elsewhere the IMU and visual shares round its last bits away)."""
    cfgs = ["config1", "config2", "tiny", "config3"]
    ws = [ph.dense_prior_window(cv.synth.make_window(cfgs[i % 4], seed=2200 + i), 100 + i, full=(i % 5 == 0)) for i in range(14)]
    ws += [_prior_only_window(cv, 2250), _prior_only_window(cv, 2260)]
    assert all(w.K <= 25 for w in ws) and len(ws) <= 128
    runs = []
    for variant in ("plain", "profiled", "split"):
        if variant == "split":
            monkeypatch.setenv("CTVIO_SPLIT_LINEARIZE", "1")
        with cv.Solver(deterministic=1) as s:
            if variant == "profiled":
                s.set_profiling(True)
            batch = [w.copy() for w in ws]
            s.set_windows(batch)
            costs = [s.linearize(i)[4] for i in range(len(ws))]
            s.set_windows(batch)
            runs.append((variant, costs, s.solve(15), batch))
    _, c0, sm0, b0 = runs[0]
    for variant, c, sm, b in runs[1:]:
        assert c == c0, (variant, [i for i, (x, y) in enumerate(zip(c, c0)) if x != y])
        assert sm == sm0, variant
        for x, y in zip(b, b0):
            assert np.array_equal(x.quat, y.quat) and np.array_equal(x.pos, y.pos) and np.array_equal(x.bias, y.bias), variant
            assert np.array_equal(x.rho, y.rho) and x.ld == y.ld, variant


def test_refused_priors(cv, oracle):
    """add_window and set_batch return CTVIO_ERR_INVALID for two prior blocks with the same (kind, index) at different offsets (every
    kind) and for an LD block with index != 0 -- refused on the host before anything is packed or launched: the handle then solves a
    valid batch as if nothing had happened."""
    w = ph.dense_prior_window(cv.synth.make_window("tiny", seed=2300), 110)
    bads = [ph.duplicate_block(w, k) for k in (ph.PK_ROT, ph.PK_POS, ph.PK_BG, ph.PK_BA, ph.PK_LD)]
    ld = w.copy(); ld.p_index = ld.p_index.copy(); ld.p_index[ld.p_kind == ph.PK_LD] = 1
    bads.append(ld.normalize())
    with cv.Solver() as s:
        for bad in bads:
            with pytest.raises(cv.capi.CtvioError, match=r"\(1\)"):
                s.add_window(bad)
            with pytest.raises(cv.capi.CtvioError, match=r"\(1\)"):
                s.set_windows([w.copy(), bad])
        with pytest.raises(cv.capi.CtvioError, match="duplicate"):
            s.set_windows([bads[0]])
        wg = w.copy()
        s.set_windows([wg])
        assert s.cost(0) == pytest.approx(oracle.OracleWindow(w.copy()).cost(), rel=1e-12)
