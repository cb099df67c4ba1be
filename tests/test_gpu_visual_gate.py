"""GPU (-m gpu): ctvio_visual_gate_batch / ctvio_visual_gate (csrc/kernels_cov.hpp: k_cov_gate_jac, k_cov_solve tiles of kind TILE_GATE,
k_cov_gate_reduce) against the NumPy reference of tests/visgate_helpers.py on the DEVICE's own ctvio_linearize output of the same state (as
tests/test_gpu_project_landmarks.py, and for its reason).

Per block, in this order: the status (blocks whose reference redundancy lies within a factor 4 of min_redundancy are not compared on it, at
most 5 % of a window); res2 / depth at projection_helpers.value_atol scaled by img_w; weight within 8 ulp of the closed form from the returned
res2; cov4 symmetric to the bit with a positive diagonal and cov_metric <= visgate_helpers.loo_bound -- the projection bound 4 kappa_s 2^-53 g
through the first-order map dC_loo = K dCw K^T, K = C_loo Cw^-1 of norm 1 / redundancy, plus the 2 x 2 step's own rounding --, the bound
itself below 1e-2; redundancy within visgate_helpers.redundancy_bound; chi2 against the extended-precision value from the returned res2 / cov4
at relative 16 kappa_2(C_loo + I) 2^-53.  Per landmark: the count, the mean against the NumPy sum of the returned per-block values within
lm_count 2^-52 relative, max and min bit-equal to the extremes of the returned per-block arrays."""
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
FIELDS = ("res", "weight", "depth", "redundancy", "cov", "chi2", "status", "lm_stats", "lm_count")
VALUES = ("res", "weight", "depth", "lm_count")


def references(w, ref, min_red=0.01):
    import visgate_helpers as vg
    return [vg.block_reference(w, ref, v, min_red) for v in range(w.V)]


def same(a, b, fields=FIELDS):
    return qh.same_bits(a, b, fields)


def take(o, vs, ls):
    return SimpleNamespace(**{f: (getattr(o, f)[ls] if f.startswith("lm_") else getattr(o, f)[vs]) for f in FIELDS})


def check(w, R, out, what, min_red=0.01, values_only=False):
    """out (Solver.visual_gate) against the per-block references R; returns the worst (error / bound, bound) of cov4."""
    import cov_helpers as ch
    import projection_helpers as pr
    import visgate_helpers as vg
    V = w.V
    assert out.res.shape == (V, 2) and out.status.shape == (V,) and out.lm_count.shape == (w.L,)
    skipped, worst = 0, (0.0, 0.0)
    for v, r in enumerate(R):
        want = r.status if not values_only or r.status == vg.NONE else vg.OK
        near = not values_only and r.status in (vg.OK, vg.WEAK) and min_red / 4 <= r.redundancy <= 4 * min_red
        if near:
            skipped += 1
            assert out.status[v] in (vg.OK, vg.WEAK), (what, v, out.status[v])
        else:
            assert out.status[v] == want, (what, v, out.status[v], want, r.redundancy)                       # 1. the status
        st = int(out.status[v])
        if st == vg.NONE:
            assert np.isnan(out.res[v]).all() and np.isnan(out.weight[v]) and np.isnan(out.depth[v]), (what, v)
            assert values_only or (np.isnan(out.cov[v]).all() and np.isnan(out.chi2[v]) and np.isnan(out.redundancy[v])), (what, v)
            continue
        proj = np.array([r.res[0] / w.img_w + w.v_pj[v, 0], r.res[1] / w.img_w + w.v_pj[v, 1], r.depth])
        txy, tz = pr.value_atol(w, proj)                                                                    # 2. the values
        assert (np.abs(out.res[v] - r.res) <= w.img_w * txy).all(), (what, v, out.res[v], r.res, txy)
        assert abs(out.depth[v] - r.depth) <= 1e-12 * abs(r.depth) + tz, (what, v, out.depth[v], r.depth)
        wgt = vg.corrector(out.res[v], vg.cauchy_width(w, v))[0]
        assert abs(out.weight[v] - wgt) <= 8 * np.spacing(wgt), (what, v, out.weight[v], wgt)
        if values_only:
            continue
        c = out.cov[v]
        if st == vg.NO_INFO:
            assert out.redundancy[v] == 0.0 and np.isposinf(np.diag(c)).all() and c[0, 1] == 0 and c[1, 0] == 0 and out.chi2[v] == 0.0, (what, v)
            continue
        rb = vg.redundancy_bound(r)                                                                         # 3. the redundancy
        assert abs(out.redundancy[v] - r.redundancy) <= rb, (what, v, out.redundancy[v], r.redundancy, rb)
        if st == vg.WEAK:
            assert np.isposinf(np.diag(c)).all() and c[0, 1] == 0 and c[1, 0] == 0 and out.chi2[v] == 0.0, (what, v)
            continue
        assert np.isfinite(c).all() and c[0, 1] == c[1, 0] and (np.diag(c) > 0).all(), (what, v, c)         # 4. the covariance
        if r.status != vg.OK:
            continue       # (a block near the threshold that the reference calls weak: it has no reference covariance)
        tol = vg.loo_bound(r)
        e = ch.cov_metric(c, r.cov)
        print(f"  {what} block {v}: error {e:.3g}, bound {tol:.3g}, redundancy {r.redundancy:.3g}") if e > 0.5 * tol else None
        assert tol < 1e-2, (what, v, tol)
        assert e <= tol, (what, v, e, tol, r.redundancy)
        worst = max(worst, (e / tol, tol))
        val, k2 = vg.chi2_reference(out.res[v], c)                                                          # 5. the gate
        assert abs(out.chi2[v] - val) <= 16 * k2 * EPS * val, (what, v, out.chi2[v], val, k2)
    assert skipped <= 0.05 * V, (what, skipped, V)
    for l in range(w.L):                                                                                    # 6. the landmarks
        vs = np.nonzero((np.asarray(w.v_lm) == l) & (out.status != vg.NONE))[0]
        assert out.lm_count[l] == vs.shape[0], (what, l, out.lm_count[l], vs.shape[0])
        if values_only:
            continue
        m, cmax, rmin = out.lm_stats[l]
        if vs.shape[0] == 0:
            assert np.isnan(m) and cmax == 0.0 and np.isposinf(rmin), (what, l, out.lm_stats[l])
            continue
        terms = np.sqrt(out.res[vs, 0] * out.res[vs, 0] + out.res[vs, 1] * out.res[vs, 1]) / w.img_w
        mean = terms.sum() / vs.shape[0]
        assert abs(m - mean) <= vs.shape[0] * 2.0 ** -52 * mean, (what, l, m, mean)
        chis = out.chi2[vs][out.status[vs] == vg.OK]
        reds = out.redundancy[vs][(out.status[vs] == vg.OK) | (out.status[vs] == vg.WEAK)]
        assert cmax == (chis.max() if chis.shape[0] else 0.0) and rmin == (reds.min() if reds.shape[0] else np.inf), (what, l, out.lm_stats[l])
    print(f"{what}: {V} blocks ({skipped} near the threshold), cov4 worst error {worst[0]:.3g} of its bound {worst[1]:.3g}")
    return worst


def run(cv, w, what, min_red=0.01, solve=0):
    """One window on a fresh handle: (the window at the device's state, references, values-only output, full output)."""
    with cv.Solver() as s:
        b = [w.copy()]
        s.set_windows(b)
        if solve:
            s.solve(solve)
        R = references(b[0], device_reference(s, 0, b[0]), min_red)
        vals = s.visual_gate(0, cov=False, min_redundancy=min_red)
        full = s.visual_gate(0, min_redundancy=min_red)
    check(b[0], R, vals, what + ", values only", min_red, values_only=True)
    check(b[0], R, full, what, min_red)
    assert same(vals, full, VALUES) and vals.cov is None and vals.lm_stats is None
    return b[0], R, vals, full


def fixture_window(cv, golden_dir, cfg, seed):
    fx = np.load(os.path.join(golden_dir, f"cov_{cfg}_seed{seed}.npz"))
    w = cv.synth.make_window(cfg, seed=seed)
    w.quat[:] = fx["quat"]; w.pos[:] = fx["pos"]; w.bias[:] = fx["bias"]; w.rho[:] = fx["rho"]; w.ld = float(fx["ld"])
    return w


def test_tiny(cv, golden_dir):
    """`tiny` seed 7 at its covariance fixture's state (K 12, V 32; unconverged, heavily down-weighted): no block near the threshold."""
    import visgate_helpers as vg
    w = fixture_window(cv, golden_dir, "tiny", 7)
    assert (w.K, w.V) == (12, 32)
    _, R, _, full = run(cv, w, "tiny")
    assert all(r.status == vg.OK for r in R) and min(r.redundancy for r in R) > 0.04
    assert (full.weight < 1).all() and (full.chi2 > 0).all()


def test_config1(cv, golden_dir):
    """`config1` seed 1000 at its covariance fixture's state (K 24, V 201, a free line delay): no block near the threshold."""
    import visgate_helpers as vg
    w = fixture_window(cv, golden_dir, "config1", 1000)
    assert (w.K, w.V) == (24, 201)
    _, R, _, _ = run(cv, w, "config1")
    assert all(r.status == vg.OK for r in R) and min(r.redundancy for r in R) > 0.04


def test_long_window(cv):
    """K = 34 (P = 301): the linearisation that does not keep the packed Hessian in LDS, the envelope panel Cholesky."""
    w = cv.synth.make_window("config1", seed=1400, F=16, L=60, M=750)
    assert w.K == 34 and w.K > 25
    run(cv, w, "long k34", solve=4)


def test_variants(cv, golden_dir):
    """`tiny`: fix_ld; per-block v_cauchy mixing 1, 2 and <= 0 (on `config1`); a landmark with a single block and a free depth (status 4, reference redundancy
    below min_redundancy / 10); a landmark with two anchors (status 3); a landmark of `config1` whose depth column underflows (rho = 1e154: Hll == 0,
    status 2 where the anchor camera lies in front of the observing one)."""
    import visgate_helpers as vg
    w = fixture_window(cv, golden_dir, "tiny", 7)
    x = w.copy(); x.fix_ld = True
    run(cv, x, "tiny, fix_ld")
    x = fixture_window(cv, golden_dir, "config1", 1000)      # (converged: without a loss an unconverged block of `tiny` is its landmark's information)
    x.v_cauchy = np.array([(1.0, 2.0, 0.0, -1.0)[v % 4] for v in range(x.V)])
    _, _, _, f = run(cv, x, "config1, v_cauchy 1 / 2 / <= 0")
    assert (f.weight[2::4] == 1.0).all() and (f.weight[3::4] == 1.0).all()
    x = w.copy()
    keep = np.ones(w.V, bool)
    vs = np.nonzero(w.v_lm == 4)[0]
    assert vs.shape[0] >= 2
    keep[vs[1:]] = False
    for a in ("v_lm", "v_ti", "v_tj", "v_rowi", "v_rowj", "v_pi", "v_pj"):
        setattr(x, a, getattr(x, a)[keep])
    xs, R, _, f = run(cv, x, "tiny, landmark 4 with a single block")
    v = int(np.nonzero(xs.v_lm == 4)[0][0])
    assert R[v].status == vg.WEAK and R[v].redundancy < 0.01 / 10 and f.status[v] == vg.WEAK
    assert sum(r.status == vg.WEAK for r in R) == 1 and f.lm_stats[4, 1] == 0.0 and f.lm_stats[4, 2] == f.redundancy[v]
    x = w.copy()
    vs = np.nonzero(x.v_lm == 6)[0]
    x.v_pi[vs[-1], 0] += 1e-3
    _, R, _, f = run(cv, x, "tiny, landmark 6 with two anchors")
    assert (f.status[vs] == vg.NONE).all() and f.lm_count[6] == 0 and np.isnan(f.lm_stats[6, 0])
    w1 = fixture_window(cv, golden_dir, "config1", 1000)      # (`tiny` has no camera that looks at another camera's centre)
    found = False
    for l in range(w1.L):
        x = w1.copy(); x.rho[l] = 1e154
        if any(r.status == vg.OK for r in references(x, None) if r.l == l):
            found = True
            break
    assert found, "no landmark whose anchor camera lies in front of an observing one"
    _, R, _, f = run(cv, x, f"config1, rho[{l}] = 1e154")
    assert any(r.status == vg.NO_INFO for r in R) and all(r.status in (vg.NO_INFO, vg.NONE) for r in R if r.l == l)


def mixed_windows(cv, golden_dir):
    empty = cv.synth.make_window("tiny", seed=9)
    for a in ("v_lm", "v_ti", "v_tj", "v_rowi", "v_rowj", "v_pi", "v_pj"):
        setattr(empty, a, getattr(empty, a)[:0])
    empty.normalize()
    assert empty.V == 0 and empty.L > 0
    return [fixture_window(cv, golden_dir, "tiny", 7), fixture_window(cv, golden_dir, "config1", 1000), empty]


def test_bits(cv, golden_dir, monkeypatch):
    """deterministic on: the batch entry over (tiny, config1, a window with V = 0), the single-window entry, a second call, the values-only
    call (for the values), a call with some outputs alone, a call forced into more than one slice (CTVIO_GATE_SLICE), and that again with CTVIO_POISON=1 are
    bitwise equal."""
    p = cv.capi._p
    ws = mixed_windows(cv, golden_dir)
    voff = np.concatenate([[0], np.cumsum([w.V for w in ws])]); loff = np.concatenate([[0], np.cumsum([w.L for w in ws])])
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        out = s.visual_gate_batch()
        assert out.res.shape[0] == voff[-1] and out.lm_count.shape[0] == loff[-1]
        assert (out.status[:voff[2]] == 0).all() and (out.lm_count[loff[2]:] == 0).all()
        assert np.isnan(out.lm_stats[loff[2]:, 0]).all() and (out.lm_stats[loff[2]:, 1] == 0).all() and np.isposinf(out.lm_stats[loff[2]:, 2]).all()
        for i in range(3):
            assert same(s.visual_gate(i), take(out, slice(voff[i], voff[i + 1]), slice(loff[i], loff[i + 1]))), i
        assert same(s.visual_gate_batch(), out)
        assert same(s.visual_gate_batch(cov=False), out, VALUES)
        chi = np.zeros(voff[-1]); o = cv.capi.GateOptions(0.01)
        import ctypes as C
        assert s._lib.ctvio_visual_gate_batch(s._h, C.byref(o), None, None, None, None, None, p(chi), None, None, None) == 0
        assert np.array_equal(chi, out.chi2)
    monkeypatch.setenv("CTVIO_GATE_SLICE", "64")
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        assert same(s.visual_gate_batch(), out)
        assert same(s.visual_gate(1), take(out, slice(voff[1], voff[2]), slice(loff[1], loff[2])))
    monkeypatch.setenv("CTVIO_POISON", "1")      # (reused scratch starts as NaN: nothing reads what the call has not written)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        assert same(s.visual_gate_batch(), out)
        assert same(s.visual_gate_batch(cov=False), out, VALUES)


def test_leaves_the_solve_alone(cv, golden_dir):
    """State bits, graph captures and a following solve are unchanged by the calls; the timing slots of both modes; the residuals agree with
    ctvio_project_landmarks of the blocks' own (l, t_j, row_j) within the value bound."""
    import projection_helpers as pr
    ws = mixed_windows(cv, golden_dir)[:2]

    def calls(s, b):
        o1 = s.visual_gate_batch()
        ms, launches = s.last_timing()
        assert launches[:4].tolist() == [1, 1, 1, 1] and ms[7] >= ms[1] > 0 and ms[2] > 0 and ms[3] > 0
        o2 = s.visual_gate_batch(cov=False)
        ms, launches = s.last_timing()
        assert launches[:4].tolist() == [0, 0, 1, 0] and ms[7] >= ms[2] > 0
        assert same(o1, o2, VALUES)
        return o1

    def cross_checks(s, b, o1):
        s.writeback_all()
        v0 = 0
        for i, w in enumerate(b):
            pl = s.project_landmarks(i, w.v_lm, w.v_tj, w.v_rowj, cov=False)
            for v in range(w.V):
                txy, _ = pr.value_atol(w, pl.proj[v])
                assert (np.abs(o1.res[v0 + v] - w.img_w * (pl.proj[v, :2] - w.v_pj[v])) <= w.img_w * txy).all(), (i, v)
            v0 += w.V
    qh.check_leaves_the_solve_alone(cv, ws, calls, compare_ld=False, then=cross_checks)


def test_callers_block_order(cv, golden_dir):
    """A window uploaded with its visual blocks shuffled: the per-block outputs are the same permutation of the unshuffled window's (the
    normal equations are summed in another order: the values to the bit -- a block's value depends on its own data alone --, the covariances
    within the bound); the per-landmark counts are unchanged.  A wrong inverse permutation fails the value comparison."""
    import cov_helpers as ch
    import visgate_helpers as vg
    w = fixture_window(cv, golden_dir, "config1", 1000)
    sh = np.random.default_rng(5).permutation(w.V)
    x = w.copy()
    for a in ("v_lm", "v_ti", "v_tj", "v_rowi", "v_rowj", "v_pi", "v_pj"):
        setattr(x, a, getattr(x, a)[sh])
    assert not np.array_equal(x.v_pj, w.v_pj)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy()])
        R = references(w, device_reference(s, 0, w))
        a = s.visual_gate(0)
    with cv.Solver(**DET) as s:
        s.set_windows([x.copy()])
        b = s.visual_gate(0)
    assert same(b, take(a, sh, slice(None)), ("res", "weight", "depth", "status", "lm_count"))
    for i, v in enumerate(sh):
        assert ch.cov_metric(b.cov[i], a.cov[v]) <= 2 * vg.loo_bound(R[v]), (i, v)
        assert abs(b.redundancy[i] - a.redundancy[v]) <= 2 * vg.redundancy_bound(R[v]), (i, v)


def test_refusals_leave_the_handle_usable(cv):
    """CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a bad id, NULL options, min_redundancy outside (0, 1) or non-finite, every
    output NULL with V > 0; the handle gives the same answer afterwards."""
    import ctypes as C
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        st = np.zeros(w.V, np.int32)
        o = cv.capi.GateOptions(0.01)
        none8 = [None] * 8
        assert lib.ctvio_visual_gate_batch(h, C.byref(o), None, None, None, None, None, None, p(st), None, None) == 4
        s.set_windows([w.copy()])
        ok = s.visual_gate(0)
        assert lib.ctvio_visual_gate(h, 1, C.byref(o), *none8[:6], p(st), None, None) == 1
        assert lib.ctvio_visual_gate(h, -1, C.byref(o), *none8[:6], p(st), None, None) == 1
        assert lib.ctvio_visual_gate(h, 0, None, *none8[:6], p(st), None, None) == 1
        for bad in (0.0, 1.0, -0.5, 2.0, float("nan"), float("inf")):
            assert lib.ctvio_visual_gate(h, 0, C.byref(cv.capi.GateOptions(bad)), *none8[:6], p(st), None, None) == 1, bad
        assert lib.ctvio_visual_gate(h, 0, C.byref(o), *none8[:6], None, None, None) == 1
        assert lib.ctvio_visual_gate(h, 0, C.byref(o), *none8[:6], p(st), None, None) == 0
        assert np.array_equal(st, ok.status)
        assert same(s.visual_gate(0), ok)
