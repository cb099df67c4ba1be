"""GPU: the reference-shaped C++ adaptor (include/ctvio_estimator.hpp) -- pointers in, results written back in
place -- must give the same solve as the index-based C ABI used by the Python host."""
import subprocess

import numpy as np
import pytest
from query_harness import _dump, build_demo, read_state  # noqa: F401  (_dump: other test files take it from here)

pytestmark = pytest.mark.gpu


def test_adaptor_matches_c_abi(cv, tmp_path):
    exe = build_demo("estimator_demo", tmp_path)
    w0 = cv.synth.make_window("config1", seed=1005)
    _dump(w0, str(tmp_path / "in.txt"))
    out = subprocess.check_output([exe, str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), "15", "fp64"], text=True)
    assert "ctvio: iterations" in out
    arr = np.array(open(tmp_path / "out.txt").read().split(), float)
    wa, _ = read_state(w0, arr)
    with cv.Solver(precision="fp64") as s:
        wg = w0.copy()
        s.set_windows([wg])
        sm = s.solve(15)[0]
    assert int(arr[-2]) == sm["iterations"]
    assert cv.rel_state_error(wa, wg)["state"] < 1e-9
