"""CPU: tests/demo_window.hpp, the reader every adaptor demo shares, without a device: tests/demo_window_check.cpp reads a dump, calls
add_factors on an estimator that never solves, and writes the state back.  The state must equal the window's arrays exactly (repr(float) in
the dump and precision(17) in write_state both round-trip a double), and every prior block pointer must resolve to the parameter block the
dump names."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@pytest.fixture(scope="module")
def check_exe(cv, tmp_path_factory):
    import query_harness as qh
    cv.capi.build_library()                      # the adaptor header calls into libctvio.so; this program never reaches a device call
    return qh.build_demo("demo_window_check", tmp_path_factory.mktemp("demo_window"))


@pytest.mark.parametrize("prior", [False, True], ids=["no_prior", "prior"])
def test_dump_round_trips_through_demo_window(cv, check_exe, tmp_path, prior):
    import prior_helpers as ph
    import query_harness as qh
    w = cv.synth.make_window("tiny", seed=7)
    w = ph.with_prior(w, ph.make_prior(w, 3) if prior else None)
    assert (w.pn > 0) == prior
    qh._dump(w, str(tmp_path / "in.txt"))
    subprocess.run([check_exe, str(tmp_path / "in.txt"), str(tmp_path / "out.txt")], check=True, timeout=60)
    wa, rest = qh.read_state(w, np.array(open(tmp_path / "out.txt").read().split(), float))
    for a in qh.STATE_ARRAYS:
        assert np.array_equal(getattr(wa, a), getattr(w, a)), a
    assert wa.ld == float(w.ld)
    nb = len(w.p_kind)
    assert rest.shape == (2 * nb,)
    kind, index = rest.reshape(nb, 2).astype(int).T
    assert np.array_equal(kind, w.p_kind) and np.array_equal(index, w.p_index)
    if prior:
        blocks = list(zip(kind.tolist(), index.tolist()))
        assert len(set(blocks)) == nb                                   # no block resolves to another's pointer
        assert (kind <= 1).any() and np.isin(kind, (2, 3)).any() and (kind == 4).sum() == 1
