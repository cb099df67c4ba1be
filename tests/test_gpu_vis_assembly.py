"""GPU (-m gpu): the visual assembly (k_assemble_vis_mfma: knot-major local columns, contiguous scatter with the disjoint-ends fast
path, IMU knot tiles from per-lane constants, row-wise flush) against the oracle's dense normal equations, in all three instantiations:
the eight-wave LDS kernel, the global-atomic one for K > 25 and the one-wave store tail of the deterministic mode.

Windows (where the two ends' knot quadruples lie decides the scatter's path):
  K 6   tiny, dt 200 ms   identical quadruples, or 1 / 2 segments apart (3 / 2 shared knots): the doubling rule
  K 12  tiny              2 segments apart (2 shared knots), or 4 / 6 / 8 apart: disjoint, the fast path
  K 33  tiny, dt 15 ms    K > 25: global atomics, all disjoint
  K 24  config1, L 200    frame pairs with more than 8 blocks: runs carried across items and cut at wave boundaries
  K 12  tiny, ends of every other landmark swapped: the i end lies AFTER the j end (validate_window admits it)
Scaling and bounds are those of test_linearize_matches_oracle (tests/test_gpu_parity.py): 1e-10 on the scaled H, W, Hll, g; cost rel 1e-12."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _swapped_ends(cv):
    w = cv.synth.make_window("tiny", seed=1000)
    sw = np.asarray(w.v_lm) % 2 == 1
    for a, b in (("v_ti", "v_tj"), ("v_rowi", "v_rowj")):
        x, y = np.asarray(getattr(w, a)).copy(), np.asarray(getattr(w, b)).copy()
        setattr(w, a, np.where(sw, y, x).astype(x.dtype))
        setattr(w, b, np.where(sw, x, y).astype(y.dtype))
    pi, pj = np.asarray(w.v_pi).copy(), np.asarray(w.v_pj).copy()
    w.v_pi = np.where(sw[:, None], pj, pi)
    w.v_pj = np.where(sw[:, None], pi, pj)
    w.normalize()
    return w


WINDOWS = {
    "k6_shared": lambda cv: cv.synth.make_window("tiny", seed=1000, dt_ns=200_000_000),
    "k12_mixed": lambda cv: cv.synth.make_window("tiny", seed=1000),
    "k33_global": lambda cv: cv.synth.make_window("tiny", seed=1000, dt_ns=15_000_000),
    "k24_long_runs": lambda cv: cv.synth.make_window("config1", seed=1000, L=200),
    "k12_i_after_j": _swapped_ends,
}


@pytest.fixture(scope="module")
def cases(cv, oracle):
    """name -> (window, the oracle's H, g, cost): computed once, never modified (the tests work on copies)."""
    out = {}
    for name, make in WINDOWS.items():
        w = make(cv)
        H, g, cost = oracle.OracleWindow(w.copy()).build_normal()
        assert np.isfinite(H).all() and np.isfinite(g).all() and np.isfinite(cost)
        out[name] = (w, H, g, cost)
    return out


def _check(lin, ref):
    w, H, g, cost = ref
    Hg, Wg, Hllg, gg, costg = lin
    P = w.P
    sc = np.sqrt(np.maximum(np.diag(H), 1e-30))
    errs = (abs(costg / cost - 1),
            np.abs((Hg - H[:P, :P]) / np.outer(sc[:P], sc[:P])).max(),
            np.abs((Wg - H[:P, P:]) / np.outer(sc[:P], sc[P:])).max(),
            np.abs(Hllg / np.diag(H)[P:] - 1).max(),
            np.abs((gg - g) / sc).max() / np.abs(g / sc).max())
    print("K", w.K, "cost, H, W, Hll, g errors:", errs)
    assert costg == pytest.approx(cost, rel=1e-12)
    assert errs[1] < TOL and errs[2] < TOL and errs[3] < TOL and errs[4] < TOL


@pytest.mark.parametrize("det", [1, 0])
@pytest.mark.parametrize("name", ["k6_shared", "k12_mixed", "k33_global", "k24_long_runs", "k12_i_after_j"])
def test_single_window_matches_oracle(cv, cases, name, det):
    """deterministic = 1: one-wave parts with the store tail (K 33 is beyond it: deterministic = 2, where the K <= 25 windows run
    exactly as under 1 and K 33 takes the tile-owner kernel); deterministic = 0: the eight-wave kernels, several parts per window."""
    w = cases[name][0]
    with cv.Solver(deterministic=(2 if w.K > 25 else 1) if det else 0) as s:
        s.set_windows([w.copy()])
        _check(s.linearize(0), cases[name])


def test_batch_launches_both_variants(cv, cases):
    """LDS-resident and K > 25 windows in one batch: both variants are launched, each window is taken by one of them."""
    names = ["k6_shared", "k12_mixed", "k33_global"]
    with cv.Solver(deterministic=0) as s:
        s.set_windows([cases[n][0].copy() for n in names])
        for i, n in enumerate(names):
            _check(s.linearize(i), cases[n])


@pytest.mark.parametrize("det", [1, 0])
def test_one_part_per_window(cv, cases, det):
    """512 windows: one workgroup per window, which flushes its LDS Hessian itself -- the store tail's rows with the prior added on the
    way out (deterministic = 1), the first-writer stores of the accumulate path (0)."""
    names = ["k6_shared", "k12_mixed", "k12_i_after_j"]
    with cv.Solver(deterministic=det) as s:
        s.set_windows([cases[names[i % 3]][0].copy() for i in range(512)])
        for i in (0, 1, 2, 511):
            _check(s.linearize(i), cases[names[i % 3]])


def test_deterministic_is_bitwise_and_throughput_mode_agrees(cv, cases):
    names = ["k6_shared", "k12_mixed", "k24_long_runs", "k12_i_after_j"]
    lins = []
    for rep in range(2):
        with cv.Solver(deterministic=1) as s:
            s.set_windows([cases[n][0].copy() for n in names])
            lins.append([s.linearize(i) for i in range(len(names))])
    for a, b in zip(*lins):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])     # H and g, bit for bit
    # the throughput mode against the deterministic one: the bound of test_deterministic_mode_is_bitwise_reproducible
    solved = {}
    for det in (1, 0):
        with cv.Solver(deterministic=det) as s:
            solved[det] = [cases[n][0].copy() for n in names]
            s.set_windows(solved[det])
            s.solve(15)
    assert max(cv.rel_state_error(x, y)["state"] for x, y in zip(solved[0], solved[1])) < 1e-6
