"""GPU (-m gpu): ctvio_cull_visual_batch / ctvio_cull_visual (csrc/kernels_cov.hpp: k_vis_cull behind the gate's kernels).  The cull decides on
the very bits ctvio_visual_gate returns at the same state and flags, so every expectation here is cull_helpers.decide on a gate call of the
same handle, compared EXACTLY.  Shapes: `tiny` seed 7, `config1` seed 1000 and K 34 / V 270 (tests/test_gpu_visual_active.py: make), each with
max(3, V // 20) observations shifted by N(0, 0.05)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cull_helpers as cu  # noqa: E402
import query_harness as qh  # noqa: E402
from query_harness import DET  # noqa: E402
from test_gpu_visual_active import SHAPES, make  # noqa: E402


def expected(w, gate, active, **opts):
    return cu.decide(w.v_lm, gate.status, gate.chi2, gate.lm_stats, gate.lm_count, active, **opts)


@pytest.mark.parametrize("name", SHAPES)
def test_cull_is_the_gates_decision(cv, name):
    """After the solve: visual_gate, then cull_visual with the same options -- the culled set is {status 0 and chi2 > chi2_max} of the gate's
    arrays exactly, n_culled and the returned flags agree with visual_active(); worst_only takes per landmark the arg-max; the landmark rule
    takes exactly the landmarks with lm_stats[:, 0] > 0.01; a second cull at the same state takes what a fresh gate call says, no more."""
    import visgate_helpers as vg
    x, bad, _ = make(cv, name)
    iters = 4 if name == "k34" else 15
    with cv.Solver(**DET) as s:
        s.set_windows([x.copy()])
        s.solve(iters, writeback=False)
        on = np.ones(x.V, np.uint8)
        gate = s.visual_gate(0)
        # ---- worst_only
        want = expected(x, gate, on, worst_only=1)
        got = s.cull_visual(0, worst_only=1)
        assert want.any() and np.array_equal(got.active == 0, want) and got.n_culled.tolist() == [int(want.sum())]
        assert np.bincount(np.asarray(x.v_lm)[want]).max() == 1
        s.set_visual_active(None, 0)
        # ---- the landmark rule alone
        want = expected(x, gate, on, chi2_max=0.0, mean_error_max=0.01)
        got = s.cull_visual(0, chi2_max=0.0, mean_error_max=0.01)
        hit = np.nan_to_num(gate.lm_stats[:, 0]) > 0.01
        assert hit.any() and np.array_equal(got.active == 0, want) and np.array_equal(want, hit[x.v_lm] & (gate.status == vg.OK))
        s.set_visual_active(None, 0)
        # ---- the block rule (defaults)
        want = expected(x, gate, on)
        got = s.cull_visual(0)
        ms, launches = s.last_timing()
        assert launches[:5].tolist() == [1, 1, 1, 1, 1] and ms[4] > 0 and ms[7] >= ms[1] > 0
        assert np.array_equal(want, (gate.status == vg.OK) & (gate.chi2 > cu.CHI2_99))
        assert want.any() and np.array_equal(got.active == 0, want) and got.n_culled.tolist() == [int(want.sum())]
        assert np.array_equal(s.visual_active(0), got.active) and np.array_equal(s.visual_active(), got.active)
        assert not want[gate.status == vg.WEAK].any()
        # ---- again, at the same state and the new flags: what a fresh gate says (the survivors' chi2 has moved with H)
        gate2 = s.visual_gate(0)
        assert (gate2.status[want] != vg.OK).all() and np.isin(gate2.status[want], (cu.INACTIVE, vg.NO_INFO, vg.NONE)).all()
        want2 = expected(x, gate2, got.active)
        got2 = s.cull_visual(0)
        assert not (want2 & want).any() and got2.n_culled.tolist() == [int(want2.sum())]
        assert np.array_equal(got2.active == 0, want | want2)
    print(f"{name}: culled {np.nonzero(want)[0].tolist()} (shifted {bad.tolist()}), then {np.nonzero(want2)[0].tolist()}")


def test_entries_and_slices_agree(cv, monkeypatch):
    """A 3-window mixed batch (tiny, config1, a window without blocks), order-fixed: the batch entry, the single-window entries and a handle
    forced into several slices (CTVIO_GATE_SLICE=64) cull the same blocks, which are the gate's decision."""
    ws = [make(cv, "tiny")[0], make(cv, "config1")[0]]
    empty = cv.synth.make_window("tiny", seed=9)
    for a in cu.BLOCK_ARRAYS:
        setattr(empty, a, getattr(empty, a)[:0])
    empty.normalize()
    ws.append(empty)
    voff = np.concatenate([[0], np.cumsum([w.V for w in ws])])
    v_lm = np.concatenate([np.asarray(w.v_lm) + o for w, o in zip(ws, np.concatenate([[0], np.cumsum([w.L for w in ws])]))])

    def run(s, single):
        s.set_windows([w.copy() for w in ws])
        s.solve(15, writeback=False)
        gate = s.visual_gate_batch()
        if single:
            outs = [s.cull_visual(i) for i in range(3)]
            return gate, np.concatenate([o.n_culled for o in outs]), np.concatenate([o.active for o in outs]), s.visual_active()
        o = s.cull_visual()
        return gate, o.n_culled, o.active, s.visual_active()
    with cv.Solver(**DET) as s:
        gate, nc, act, now = run(s, False)
    want = cu.decide(v_lm, gate.status, gate.chi2, gate.lm_stats, gate.lm_count, np.ones(voff[-1], np.uint8))
    assert np.array_equal(act == 0, want) and np.array_equal(act, now)
    assert nc.tolist() == [int(want[voff[i]:voff[i + 1]].sum()) for i in range(3)] and nc[0] > 0 and nc[1] > 0 and nc[2] == 0
    with cv.Solver(**DET) as s:
        _, nc1, act1, now1 = run(s, True)
    assert np.array_equal(nc1, nc) and np.array_equal(act1, act) and np.array_equal(now1, act)
    monkeypatch.setenv("CTVIO_GATE_SLICE", "64")
    with cv.Solver(**DET) as s:
        _, nc2, act2, now2 = run(s, False)
    assert np.array_equal(nc2, nc) and np.array_equal(act2, act) and np.array_equal(now2, act)


@pytest.mark.parametrize("name", ["tiny", "config1"])
def test_separation_and_resolve(cv, oracle, name):
    """The culled set is the shifted blocks, no block of gate status 4 is touched, and the following solve(15) equals the oracle's solve of the
    reduced window from the same state (cost rel 1e-9, state <= 1e-6)."""
    import visgate_helpers as vg
    x, bad, _ = make(cv, name)
    with cv.Solver() as s:
        b = [x.copy()]
        s.set_windows(b)
        s.solve(15)
        gate = s.visual_gate(0)
        got = s.cull_visual(0)
        assert np.array_equal(np.nonzero(got.active == 0)[0], bad) and got.n_culled.tolist() == [bad.shape[0]]
        assert got.active[gate.status == vg.WEAK].all()
        print(f"{name}: shifted chi2 >= {gate.chi2[bad].min():.4g}, clean <= {np.delete(gate.chi2, bad).max():.4g}")
        wo = cu.without_blocks(b[0], bad)
        so = oracle.OracleWindow(wo).solve(15)
        sm = s.solve(15)[0]
    print(f"{name}: re-solve {sm['iterations']} iterations (oracle {so.iterations}), cost {sm['initial_cost']:.6g} -> {sm['final_cost']:.6g}")
    assert sm["iterations"] == so.iterations
    assert abs(sm["final_cost"] - so.final_cost) <= 1e-9 * so.final_cost
    assert cv.rel_state_error(b[0], wo)["state"] <= 1e-6


def test_failed_factorisation_loses_nothing(cv):
    """A batch of two corrupted windows after the solve; then a late knot of window 0 gets a position that is not a number (ctvio_set_state
    takes the caller's values as they are), so that the knot's rows of Hpp are NaN and the factorisation reports a bad pivot.  The gate says
    status 1 for the blocks whose own values are untouched by it (2 or 3 for the landmarks that see the knot); the cull takes NOTHING from it
    -- neither by chi2, which is garbage, nor by drop_uncomputable, which would not need the factorisation: the window is left alone
    entirely -- and its flags are unchanged, while the healthy window beside it is culled per the gate."""
    import visgate_helpers as vg
    ws = [make(cv, "config1")[0], make(cv, "tiny")[0]]
    V0 = ws[0].V
    with cv.Solver(**DET) as s:
        b = [w.copy() for w in ws]
        s.set_windows(b)
        s.solve(15)
        broken = b[0].copy()
        broken.pos[broken.K - 3] = np.nan       # knot 21 of 24: IMU samples and 36 blocks of 18 landmarks touch it, 121 blocks of 32 landmarks do not
        s.set_state(0, broken)
        gate = s.visual_gate_batch()
        st0 = gate.status[:V0]
        print("statuses of the broken window:", np.bincount(st0, minlength=6).tolist())
        assert np.isin(st0, (vg.SINGULAR, vg.NO_INFO, vg.NONE)).all() and (st0 == vg.SINGULAR).sum() >= 100, st0
        assert np.isnan(gate.chi2[:V0][st0 != vg.NO_INFO]).all()
        got = s.cull_visual(mean_error_max=1e-6)            # every rule on: block, landmark, uncomputable
        assert got.n_culled[0] == 0 and got.active[:V0].all() and s.visual_active(0).all()
        want = cu.decide(ws[1].v_lm, gate.status[V0:], gate.chi2[V0:], gate.lm_stats[ws[0].L:], gate.lm_count[ws[0].L:], np.ones(ws[1].V, np.uint8),
                         mean_error_max=1e-6)
        assert want.any() and np.array_equal(got.active[V0:] == 0, want) and got.n_culled[1] == want.sum()
        assert np.array_equal(s.visual_active(), got.active)
        one = s.cull_visual(0, mean_error_max=1e-6)          # the single-window entry: the same
        assert one.n_culled.tolist() == [0] and one.active.all()


def test_leaves_state_and_graph_alone(cv):
    """State bits, graph captures and a following solve are unchanged by a cull that takes nothing (chi2_max above every chi2): what a cull
    does to the solve, it does through the flags alone.  A cull that does switch blocks off leaves the state bits and the captured graph as
    they were as well, and the solve that follows replays the same graph."""
    ws = [cv.synth.make_window("tiny", seed=7), cv.synth.make_window("config1", seed=1000)]

    def calls(s, b):
        o = s.cull_visual(chi2_max=1e30, drop_uncomputable=0)
        assert o.n_culled.tolist() == [0, 0] and o.active.all() and s.visual_active().all()
        return o
    qh.check_leaves_the_solve_alone(cv, ws, calls)
    xs = [make(cv, "tiny")[0], make(cv, "config1")[0]]
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in xs])
        s.solve(6, writeback=False)
        cap, state = s.graph_captures, s.get_batch_state()
        o = s.cull_visual()
        assert (o.n_culled > 0).all() and not o.active.all()
        assert s.graph_captures == cap and qh.same_bits(state, s.get_batch_state())
        sm = s.solve(6)
        assert s.graph_captures == cap and all(np.isfinite(m["final_cost"]) for m in sm)
        assert np.array_equal(s.visual_active(), o.active)           # a solve does not touch the flags


def test_refusals_leave_the_handle_usable(cv):
    """CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a bad id, NULL options, min_redundancy outside (0, 1); CTVIO_OK with both
    outputs NULL; the handle solves like a fresh one afterwards."""
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        o = cv.capi.CullOptions()
        lib.ctvio_default_cull_options(C.byref(o))
        nc = np.zeros(1, np.int32); a = np.zeros(w.V, np.uint8)
        assert lib.ctvio_cull_visual_batch(h, C.byref(o), p(nc), p(a)) == 4
        s.set_windows([w.copy()])
        assert lib.ctvio_cull_visual(h, 1, C.byref(o), p(nc), p(a)) == 1 and lib.ctvio_cull_visual(h, -1, C.byref(o), p(nc), p(a)) == 1
        assert lib.ctvio_cull_visual(h, 0, None, p(nc), p(a)) == 1 and lib.ctvio_cull_visual_batch(h, None, p(nc), p(a)) == 1
        for bad in (0.0, 1.0, -0.5, float("nan")):
            ob = cv.capi.CullOptions(bad, 9.21, 0.0, 0, 1)
            assert lib.ctvio_cull_visual(h, 0, C.byref(ob), p(nc), p(a)) == 1, bad
        assert s.visual_active().all()
        o.chi2_max = 1e30
        assert lib.ctvio_cull_visual(h, 0, C.byref(o), None, None) == 0 and s.visual_active().all()
        qh.check_usable_after(cv, w, s)
