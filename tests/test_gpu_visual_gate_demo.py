"""GPU (-m gpu): tests/visual_gate_demo.cpp through the C++ adaptor (include/ctvio_estimator.hpp: GateVisualBlocks).  The demo solves a window,
moves one observation by 30 pixel-equivalents (a wrong match), solves again and runs the leave-one-out test: that block has the largest chi2
of its window, far beyond the 99.9 % point of chi-square with 2 degrees of freedom, and its landmark reports it; per-factor results come in
the order of the AddImageFeatureDelayAnalytic calls, per-landmark results keyed by the inverse-depth pointer."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PIXEL = 1.0 / 460.0      # one pixel in normalised image units at the focal length the row model of the other demos uses


def test_perturbed_observation_has_the_largest_chi2(cv, tmp_path):
    import query_harness as qh
    w0 = cv.synth.make_window("config1", seed=1005)
    L, V = w0.L, w0.V
    counts = np.bincount(w0.v_lm, minlength=L)
    l_bad = int(np.argmax(counts))
    assert counts[l_bad] >= 4
    vs = np.nonzero(w0.v_lm == l_bad)[0]
    bad = int(vs[len(vs) // 2])
    _, arr = qh.run_demo(qh.build_demo("visual_gate_demo", tmp_path), w0, tmp_path, 15, bad, repr(30 * PIXEL), state=False)
    assert arr[1] == V
    chi2 = arr[2:2 + V]; status = arr[2 + V:2 + 2 * V]; res = arr[2 + 2 * V:2 + 4 * V].reshape(V, 2)
    rest = arr[2 + 4 * V:]
    assert rest[0] == L
    lms = rest[1:1 + 4 * L].reshape(L, 4)
    rest = rest[1 + 4 * L:]
    assert rest[1] == V
    res_values = rest[2:2 + 2 * V].reshape(V, 2)
    assert status[bad] == 0 and np.isin(status, (0, 4)).all(), status
    print(f"block {bad} of landmark {l_bad}: chi2 {chi2[bad]:.4g}, |r| {np.linalg.norm(res[bad]):.4g}; the next largest chi2 {np.sort(chi2)[-2]:.4g}")
    assert int(np.argmax(chi2)) == bad and chi2[bad] > 13.8 and chi2[bad] > 4 * np.sort(chi2)[-2]
    assert np.array_equal(lms[:, 0], counts) and lms[l_bad, 2] == chi2[bad] and int(np.argmax(lms[:, 2])) == l_bad
    assert (lms[:, 1] > 0).all() and int(np.argmax(lms[:, 1])) == l_bad
    assert np.array_equal(res_values, res)
