"""GPU (-m gpu): tests/cull_demo.cpp -- solve, cull, solve on one upload through the C ABI (ctvio_cull_visual_batch, ctvio_solve,
ctvio_get / set_visual_active on the handle the adaptor's Solve uploaded to), and tests/cull_adaptor_check below it for
TrajectoryEstimator::SolveWithCulling.  `config1` seed 1000 with the ten blocks of cull_helpers.corrupted moved by 23 pixel-equivalents: the
demo culls exactly those blocks, the re-solve starts below the cost with the outliers and ends at the oracle's solution of the window without
them (from the state of the first solve: cost rel 1e-9, state <= 1e-6)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


SHIFT = 0.05


@pytest.fixture(scope="module")
def scenario(cv, oracle):
    """(the clean window, the shifted blocks, the oracle's solution: the corrupted window solved, then the window without the shifted blocks
    solved from there, its summary); computed once."""
    import cull_helpers as cu
    w0 = cv.synth.make_window("config1", seed=1000)
    _, bad = cu.corrupted(w0)
    x = w0.copy()
    x.v_pj[bad, 0] += SHIFT; x.v_pj[bad, 1] -= 0.5 * SHIFT
    oracle.OracleWindow(x).solve(15)
    wo = cu.without_blocks(x, bad)
    so = oracle.OracleWindow(wo).solve(15)
    return w0, bad, wo, so


def test_demo_culls_the_shifted_blocks(cv, scenario, tmp_path):
    import query_harness as qh
    w0, bad, wo, so = scenario
    wa, rest = qh.run_demo(qh.build_demo("cull_demo", tmp_path), w0, tmp_path, 15, repr(SHIFT), *bad.tolist())
    n = int(rest[0])
    culled = rest[1:1 + n].astype(int)
    cost_out, c0, c1, inactive_after = rest[1 + n:5 + n]
    print(f"culled {culled.tolist()}; cost with the outliers {cost_out:.6g}, re-solve {c0:.6g} -> {c1:.6g}")
    assert np.array_equal(culled, bad) and inactive_after == n - 1      # (one block re-admitted with ctvio_set_visual_active)
    assert c1 <= c0 < cost_out
    assert abs(c1 - so.final_cost) <= 1e-9 * so.final_cost
    assert cv.rel_state_error(wa, wo)["state"] <= 1e-6


def test_adaptor_solve_with_culling(cv, scenario, tmp_path):
    """TrajectoryEstimator::SolveWithCulling: the same blocks in the order of the AddImageFeatureDelayAnalytic calls, the same solution,
    written back through the caller's pointers."""
    import query_harness as qh
    w0, bad, wo, so = scenario
    wa, rest = qh.run_demo(qh.build_demo("cull_adaptor_demo", tmp_path), w0, tmp_path, 15, repr(SHIFT), *bad.tolist())
    n = int(rest[0])
    assert np.array_equal(rest[1:1 + n].astype(int), bad)
    assert cv.rel_state_error(wa, wo)["state"] <= 1e-6
