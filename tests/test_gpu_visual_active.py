"""GPU (-m gpu): the per-block ACTIVE flag (include/ctvio.h: ctvio_set_visual_active; Dev::v_on, honoured by vis_eval_body, k_residual_summary,
k_cov_gate_jac and k_cov_gate_reduce).  An inactive block is not a factor of the window: a handle that holds the whole (corrupted) window with
an off set switched off is compared with the oracle on -- and with a second handle uploaded with -- the REDUCED window, which lacks those
blocks (cull_helpers.without_blocks).  The off set is the shifted blocks plus every block of landmark 0, which leaves a landmark without a
factor.  Shapes: `tiny` seed 7 (K 12, V 32), `config1` seed 1000 (K 24, V 201, free line delay) and K 34 / V 270 (the wide path)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cull_helpers as cu  # noqa: E402
import query_harness as qh  # noqa: E402

SHAPES = ("tiny", "config1", "k34")


def make(cv, name):
    if name == "tiny":
        w = cv.synth.make_window("tiny", seed=7)
        assert (w.K, w.V) == (12, 32)
    elif name == "config1":
        w = cv.synth.make_window("config1", seed=1000)
        assert (w.K, w.V) == (24, 201) and not w.fix_ld
    else:
        w = cv.synth.make_window("config1", seed=1400, F=16, L=60, M=750)
        assert (w.K, w.V) == (34, 270)
    x, bad = cu.corrupted(w)
    return x, bad, cu.off_set(x, bad)


@pytest.fixture(scope="module")
def cases(cv):
    """name -> (the corrupted window, its shifted blocks, the off set, the reduced window); built once, never changed."""
    out = {}
    for name in SHAPES:
        x, bad, off = make(cv, name)
        out[name] = (x, bad, off, cu.without_blocks(x, off))
    return out


def scaled(H):
    return np.sqrt(np.maximum(np.diag(H), 1e-30))


def assert_normal_equations(w, got, H, g, cost, what, tol=1e-10):
    """tests/test_gpu_parity.py::test_linearize_matches_oracle's four scaled bounds (the Hll ratio where the oracle's is non-zero) and the cost."""
    Hg, Wg, Hllg, gg, costg = got
    P = w.P
    sc = scaled(H)
    assert costg == pytest.approx(cost, rel=1e-10), what
    assert np.abs((Hg - H[:P, :P]) / np.outer(sc[:P], sc[:P])).max() < tol, what
    assert np.abs((Wg - H[:P, P:]) / np.outer(sc[:P], sc[P:])).max() < tol, what
    d = np.diag(H)[P:]
    nz = d != 0
    assert np.abs(Hllg[nz] / d[nz] - 1).max() < tol and (Hllg[~nz] == 0).all(), what
    assert np.abs((gg - g) / sc).max() < tol * np.abs(g / sc).max(), what


@pytest.mark.parametrize("name", SHAPES)
def test_linearisation_is_the_reduced_windows(cv, oracle, cases, name):
    """ctvio_linearize / ctvio_cost with the off set against the oracle's normal equations of the reduced window at the same state; landmark 0
    has Hll == 0, a zero row of W and a zero gradient entry, exactly; one more block off changes H by that block's J~^T J~
    (visgate_helpers.corrected_jacobian on the device's own linearisation), to the same bound."""
    import visgate_helpers as vg
    x, bad, off, red = cases[name]
    H, g, cost = oracle.OracleWindow(red.copy()).build_normal()
    P = x.P
    with cv.Solver() as s:
        s.set_windows([x.copy()])
        full = s.linearize(0)
        s.set_visual_active(cu.flags(x, off), 0)
        assert np.array_equal(s.visual_active(0), cu.flags(x, off)) and np.array_equal(s.visual_active(), cu.flags(x, off))
        got = s.linearize(0)
        assert_normal_equations(x, got, H, g, cost, name)
        assert s.cost(0) == pytest.approx(cost, rel=1e-10)
        assert got[2][0] == 0.0 and (got[1][:, 0] == 0.0).all() and got[3][P] == 0.0
        assert full[2][0] > 0 and full[4] > got[4]
        # one more block: the first active block of the landmark with the most active blocks
        act = cu.flags(x, off).astype(bool)
        l = np.bincount(np.asarray(x.v_lm)[act], minlength=x.L).argmax()
        v = int(np.nonzero(act & (np.asarray(x.v_lm) == l))[0][0])
        ref = qh.device_joint_reference(s, 0, x)
        b = vg.block_reference(x, ref, v)
        assert b.status == vg.OK
        _, Jt = vg.corrected_jacobian(x, ref, b)
        more = cu.flags(x, np.r_[off, v])
        s.set_visual_active(more, 0)
        less = s.linearize(0)
        s.set_visual_active(None, 0)
        assert s.visual_active(0).all()
        again = s.linearize(0)
    Hk = vg.kept_system(ref)                           # over the kept unknowns, with the off set off; then with block v off as well
    Hl = vg.kept_system(SimpleNamespace(kp=ref.kp, kl=ref.kl, Hpp=less[0], W=less[1], Hll=less[2]))
    sc = scaled(Hk)
    err = np.abs((Hk - Hl - Jt.T @ Jt) / np.outer(sc, sc)).max()
    print(f"{name}: block {v} off changes H by its J~^T J~ to {err:.3g} (scaled)")
    assert np.abs(Jt.T @ Jt).max() > 0 and err < 1e-10, (name, err)
    sf = scaled(np.block([[full[0], full[1]], [full[1].T, np.diag(full[2])]]))
    for a, c, d in zip(full[:3], again[:3], (np.outer(sf[:P], sf[:P]), np.outer(sf[:P], sf[P:]), sf[P:] ** 2)):
        assert np.abs((a - c) / d).max() < 1e-12, name      # switched on again: the window's own normal equations (atomic sums on the wide path)


@pytest.mark.parametrize("name,iters", [("tiny", 15), ("config1", 15), ("k34", 4)])
def test_solve_matches_the_oracle_on_the_reduced_window(cv, oracle, cases, name, iters):
    """From the synthetic start, the masked handle against the oracle on the reduced window: equal iteration and success counts, final cost
    rel 1e-9, state <= 1e-6; the captured graph does not move when the flags change."""
    x, bad, off, red = cases[name]
    wo = red.copy()
    so = oracle.OracleWindow(wo).solve(iters)
    with cv.Solver() as s:
        b = [x.copy()]
        s.set_windows(b)
        s.snapshot_state()
        s.solve(iters, writeback=False)
        cap = s.graph_captures
        s.restore_state()
        s.set_visual_active(cu.flags(x, off), 0)
        sm = s.solve(iters)[0]
        assert s.graph_captures == cap
    print(f"{name}: oracle {so.iterations} iterations, {so.num_successful} successful, final cost {so.final_cost:.6g}; device {sm}")
    assert sm["iterations"] == so.iterations and sm["num_successful"] == so.num_successful
    assert abs(sm["final_cost"] - so.final_cost) <= 1e-9 * so.final_cost
    assert cv.rel_state_error(b[0], wo)["state"] <= 1e-6
    assert b[0].rho[0] == x.rho[0]                     # the landmark without a factor does not move
    if name == "tiny":
        assert so.iterations == 15 and so.num_successful == 15 and so.final_cost == pytest.approx(206.0, abs=0.05)
    if name == "config1":
        assert so.iterations == 15 and so.num_successful == 15 and so.final_cost == pytest.approx(1526.9, abs=0.05)


@pytest.mark.parametrize("name,det,poison", [("tiny", 1, False), ("config1", 1, False), ("config1", 1, True), ("k34", 2, False), ("k34", 2, True)])
def test_nothing_stale(cv, cases, monkeypatch, name, det, poison):
    """Order-fixed linearisation: solve, restore, switch the off set off, solve, restore, switch everything on, solve -- the bits of the first
    solve; two masked solves have equal bits and differ from the unmasked one.  Also with CTVIO_POISON=1."""
    x, bad, off, red = cases[name]
    if poison:
        monkeypatch.setenv("CTVIO_POISON", "1")
    iters = 4 if name == "k34" else 8

    def run(s):
        sm = s.solve(iters, writeback=False)
        st = s.get_batch_state()
        s.restore_state()
        return sm, st
    with cv.Solver(deterministic=det) as s:
        s.set_windows([x.copy()])
        s.snapshot_state()
        first = run(s)
        s.set_visual_active(cu.flags(x, off), 0)
        masked = run(s)
        masked2 = run(s)
        s.set_visual_active(None)
        last = run(s)
    assert first[0] == last[0] and qh.same_bits(first[1], last[1])
    assert masked[0] == masked2[0] and qh.same_bits(masked[1], masked2[1])
    assert not qh.same_bits(first[1], masked[1])


def test_degenerate_block_is_not_evaluated(cv, oracle, cases):
    """A landmark whose inverse depth puts its blocks behind the camera (status 3 in the gate, a non-finite or meaningless projection): with its
    blocks switched off, cost, normal equations and a 2-iteration solve are finite and the reduced window's."""
    import visgate_helpers as vg
    x0, bad, _, _ = cases["tiny"]
    x = x0.copy()
    l = 3
    x.rho[l] = -abs(x.rho[l])
    vs = np.nonzero(np.asarray(x.v_lm) == l)[0]
    red = cu.without_blocks(x, vs)
    H, g, cost = oracle.OracleWindow(red.copy()).build_normal()
    wo = red.copy()
    so = oracle.OracleWindow(wo).solve(2)
    with cv.Solver() as s:
        b = [x.copy()]
        s.set_windows(b)
        gate = s.visual_gate(0, cov=False)
        assert (gate.status[vs] == vg.NONE).any(), gate.status[vs]
        s.set_visual_active(cu.flags(x, vs), 0)
        got = s.linearize(0)
        assert all(np.isfinite(a).all() for a in got[:4]) and np.isfinite(got[4]) and np.isfinite(s.cost(0))
        assert_normal_equations(x, got, H, g, cost, "rho < 0")
        assert got[2][l] == 0.0
        sm = s.solve(2)[0]
    assert np.isfinite(sm["final_cost"]) and abs(sm["final_cost"] - so.final_cost) <= 1e-9 * so.final_cost
    assert sm["iterations"] == so.iterations and cv.rel_state_error(b[0], wo)["state"] <= 1e-6


def test_residual_summary_and_marginalisation(cv, cases):
    """counts4[2] is the number of active blocks and the image sums are those of a handle uploaded with the reduced window (rel 1e-12: atomic
    sums); ctvio_marginalize of the masked `tiny` window gives the quadratic form of the reduced upload (test_marginalize_batch_on_device's
    1e-7 bound on J0^T J0 and J0^T r0)."""
    x, bad, off, red = cases["tiny"]
    role = np.zeros(x.N, np.int8)
    role[:6] = 1; role[x.P + 1] = 1
    with cv.Solver() as s:
        s.set_windows([x.copy()])
        whole = s.residual_summary(0)
        s.set_visual_active(cu.flags(x, off), 0)
        rs = s.residual_summary(0)
        km, Jm, rm = s.marginalize(0, role)
    with cv.Solver() as s:
        s.set_windows([red.copy()])
        rr = s.residual_summary(0)
        kr, Jr, r_r = s.marginalize(0, role)
    assert whole["image"][1] == x.V and rs["image"][1] == x.V - off.shape[0] == rr["image"][1]
    assert np.allclose(rs["image"][0], rr["image"][0], rtol=1e-12, atol=0) and (rs["image"][0] < whole["image"][0]).all()
    for k in ("imu", "bias", "prior"):
        assert rs[k][1] == rr[k][1] and np.allclose(rs[k][0], rr[k][0], rtol=1e-12, atol=0)
    assert np.array_equal(km, kr)
    Hm, Hr = Jm.T @ Jm, Jr.T @ Jr
    assert np.abs(Hm - Hr).max() <= 1e-7 * np.abs(Hr).max()
    assert np.abs(Jm.T @ rm - Jr.T @ r_r).max() <= 1e-7 * np.abs(Jr.T @ r_r).max()


def test_gate_on_a_masked_window(cv, cases):
    """`config1` after 15 iterations with the off set switched off.  Active blocks: tests/test_gpu_visual_gate.py's check against references on
    the masked handle's own linearisation.  Inactive blocks: status 5 (2 for the landmark without a factor), weight 0, redundancy exactly 1,
    cov4 within 4 ulp per entry of img_w^2 x ctvio_project_landmarks' cov4 of (l, t_j, row_j) on the same handle, chi2 by the extended-precision
    rule from the returned res2 / cov4.  lm_count / lm_stats run over the active blocks."""
    import test_gpu_visual_gate as tg
    import visgate_helpers as vg
    x, bad, off, red = cases["config1"]
    act = cu.flags(x, off).astype(bool)
    with cv.Solver() as s:
        b = [x.copy()]
        s.set_windows(b)
        s.set_visual_active(act, 0)
        s.solve(15)
        w = b[0]
        ref = qh.device_joint_reference(s, 0, w)
        out = s.visual_gate(0)
        pl = s.project_landmarks(0, w.v_lm, w.v_tj, w.v_rowj)
    # ---- active blocks: as a window of their own (the reduced window at this state has the same H and the same blocks, in order)
    wr = cu.without_blocks(w, off)
    R = [vg.block_reference(wr, ref, v) for v in range(wr.V)]
    sub = tg.take(out, np.nonzero(act)[0], slice(None))
    tg.check(wr, R, sub, "config1 masked, active blocks")
    # ---- inactive blocks
    lm0 = np.asarray(w.v_lm) == 0
    for v in np.nonzero(~act)[0]:
        if lm0[v]:
            assert out.status[v] == vg.NO_INFO and out.chi2[v] == 0.0 and out.redundancy[v] == 0.0, v
            continue
        assert out.status[v] == cu.INACTIVE and out.weight[v] == 0.0 and out.redundancy[v] == 1.0, (v, out.status[v], out.redundancy[v])
        want = w.img_w ** 2 * pl.cov[v]
        assert pl.status[v] == 0 and (np.abs(out.cov[v] - want) <= 4 * np.spacing(np.abs(want))).all(), (v, out.cov[v], want)
        val, k2 = vg.chi2_reference(out.res[v], out.cov[v])
        assert abs(out.chi2[v] - val) <= 16 * k2 * tg.EPS * val, (v, out.chi2[v], val)
    assert out.lm_count[0] == 0 and np.isnan(out.lm_stats[0, 0])
    assert np.array_equal(out.lm_count, np.bincount(np.asarray(w.v_lm)[act], minlength=w.L))
    # the shifted blocks fail the re-admission test, by a wide margin
    assert (out.chi2[bad[~lm0[bad]]] > 100).all()


def test_refusals_leave_the_handle_usable(cv):
    """CTVIO_ERR_STATE before the upload; CTVIO_ERR_INVALID for a bad id, a NULL output; the handle solves like a fresh one afterwards."""
    p = cv.capi._p
    w = cv.synth.make_window("tiny", seed=7)
    with cv.Solver() as s:
        lib, h = s._lib, s._h
        a = np.ones(w.V, np.uint8)
        assert lib.ctvio_set_visual_active_batch(h, p(a)) == 4 and lib.ctvio_get_visual_active_batch(h, p(a)) == 4
        assert lib.ctvio_set_visual_active(h, 0, None) == 4 and lib.ctvio_get_visual_active(h, 0, p(a)) == 4
        s.set_windows([w.copy()])
        for wid in (1, -1):
            assert lib.ctvio_set_visual_active(h, wid, p(a)) == 1 and lib.ctvio_get_visual_active(h, wid, p(a)) == 1
        assert lib.ctvio_get_visual_active(h, 0, None) == 1 and lib.ctvio_get_visual_active_batch(h, None) == 1
        a[::3] = 0
        s.set_visual_active(a, 0)
        qh.check_usable_after(cv, w, s)              # (the upload switches every block on again)
        assert s.visual_active().all()
