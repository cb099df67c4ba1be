"""GPU (-m gpu): the two ends of k_cholesky_flow -- the prologue (every tile, fix-up value and activity byte of a wave in one round trip, the
tiles of rows 0 and 1 handed to the chain wave by flags) and the back-substitution (no workgroup barrier per block: the chain on the chain
wave, the other tiles ordered by LDS counters) -- against k_cholesky_tiles (CTVIO_CHOL_TILES=1: loads, barriers and the back-substitution
as they were), bit for bit in the deterministic mode, and against the oracle's dense step."""
import numpy as np
import pytest

from test_gpu_sparsity import _SIZES

pytestmark = pytest.mark.gpu

NGROUPS = 3


@pytest.fixture(scope="module")
def end_windows(cv):
    """Single windows whose assembly is order-fixed (K <= 25): every size of the size list that qualifies, plus a config-1 window with fixed
    leading knots (plain tiles with fixed unknowns) and one with a fixed line delay and locked gyro biases (a plain diagonal tile whose
    unknowns are partly fixed; the rhs row in a tile of its own kind)."""
    ws = [cv.synth.make_window("config1", seed=1700 + i, F=F, dt_ns=dt * 1_000_000, L=30, M=40 * F) for i, (F, dt) in enumerate(_SIZES)]
    ws = [w for w in ws if w.K <= 25]
    rows = {w.P // 16 + 1 for w in ws}
    offs = {w.P % 16 for w in ws}
    assert {3, 14} <= rows and {1, 15} <= offs, (rows, offs)   # 3 tile rows: most update waves own nothing; 14: every slot of the map
    a = cv.synth.make_window("config1", seed=1301)
    a.fixed_upto = 2
    b = cv.synth.make_window("config1", seed=1302)
    b.fix_ld = True
    b.lock_bg = True
    return ws + [a, b]


def _step(cv, monkeypatch, mode, ws):
    monkeypatch.setenv("CTVIO_CHOL_TILES", mode)
    out = []
    for w in ws:
        with cv.Solver() as s:
            s.set_windows([w.copy()])
            out.append(s.lm_step(0, 1e4))
    return out


@pytest.mark.parametrize("group", range(NGROUPS))
def test_single_window_step_equals_the_barrier_kernel_and_the_oracle(cv, oracle, end_windows, monkeypatch, group):
    """One LM step of each window ALONE in its launch (the deterministic mode): flow and barrier kernels give the same bits, and both are the
    oracle's dense Cholesky step of the un-eliminated system to 1e-8 of its largest entry."""
    ws = end_windows[group::NGROUPS]
    flow = _step(cv, monkeypatch, "3", ws)
    barrier = _step(cv, monkeypatch, "1", ws)
    for w, (d_f, mc_f), (d_b, mc_b) in zip(ws, flow, barrier):
        assert np.array_equal(d_f, d_b) and mc_f == mc_b, (w.P, np.abs(d_f - d_b).max())
        d_o, mc_o = oracle.OracleWindow(w.copy()).lm_step(1e4, use_schur=False)
        assert np.abs(d_f - d_o).max() <= 1e-8 * np.abs(d_o).max(), w.P
        assert mc_f == pytest.approx(mc_o, rel=1e-9), w.P


def test_many_workgroups_in_flight_give_the_same_bits_every_time(cv, monkeypatch):
    """64 windows of mixed sizes in one launch (4 and 14 tile rows, fixed unknowns, no prior), solved three times from a fresh state by the flow
    kernel and once by the barrier kernel: four identical results -- the flag-driven back-substitution does not depend on which wave is early."""
    base = [cv.synth.make_window("tiny", seed=41), cv.synth.make_window("config1", seed=1301), cv.synth.make_window("config2", seed=1002),
            cv.synth.make_window("config3", seed=1003), cv.synth.make_window("tumrs", seed=1004), cv.synth.make_window("tiny", seed=42, with_prior=False),
            cv.synth.make_window("config1", seed=1302)]
    base[1].fixed_upto = 2
    base[6].fix_ld = True
    base[6].lock_bg = True
    runs = []
    for mode in ("3", "3", "3", "1"):
        monkeypatch.setenv("CTVIO_CHOL_TILES", mode)
        with cv.Solver() as s:
            batch = [base[i % len(base)].copy() for i in range(64)]
            s.set_windows(batch)
            runs.append((batch, s.solve(15)))
    ref_batch, ref_sm = runs[0]
    for batch, sm in runs[1:]:
        for i in range(64):
            a, b = ref_sm[i], sm[i]
            assert (a["iterations"], a["num_successful"], a["num_unsuccessful"], a["termination"]) == (b["iterations"], b["num_successful"], b["num_unsuccessful"], b["termination"]), i
            assert a["final_cost"] == b["final_cost"], i
            assert cv.rel_state_error(ref_batch[i], batch[i])["state"] == 0.0, i
