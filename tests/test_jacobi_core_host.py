"""CPU: what the two device eigen-solvers of the prior construction share (csrc/jacobi_core.hpp, built with g++) against integer
enumeration and against the NumPy model of tests/marg_blocked_helpers.py, which restates the same rules independently."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import marg_blocked_helpers as mb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("jc") / "libjacobicore.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "host_jacobi_check.cpp")])
    lib = C.CDLL(so)
    lib.jc_tri_decode.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.jc_rr_pair.argtypes = [C.c_int, C.c_void_p]
    lib.jc_cs.argtypes = [C.c_int] + [C.c_void_p] * 5
    lib.jc_converged.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, C.c_double]
    return lib


@pytest.mark.parametrize("dim,strict", [(1024, 0), (16, 1)])   # MARG_MAXD_BLOCKED; npair <= 16 at D = 1024
def test_tri_decode(core, dim, strict):
    rows = np.arange(1, dim) if strict else np.arange(dim)
    cnt = rows if strict else rows + 1                            # entries of row i: j < i, or j <= i
    wi = np.repeat(rows, cnt).astype(np.int32)
    wj = np.concatenate([np.arange(c) for c in cnt]).astype(np.int32)
    n = dim * (dim - 1) // 2 if strict else dim * (dim + 1) // 2
    assert wi.size == n
    i = np.empty(n, np.int32); j = np.empty(n, np.int32)
    core.jc_tri_decode(n, strict, i.ctypes.data, j.ctypes.data)
    assert np.array_equal(i, wi) and np.array_equal(j, wj)


@pytest.mark.parametrize("np_", [2, 4, 6, 32, 64, 92, 180])
def test_rr_pair(core, np_):
    pq = np.empty((np_ - 1, np_ // 2, 2), np.int32)
    core.jc_rr_pair(np_, pq.ctypes.data)
    for s in range(np_ - 1):
        assert np.all(pq[s, :, 0] < pq[s, :, 1])
        assert sorted(pq[s].ravel().tolist()) == list(range(np_))          # a perfect matching
        assert [tuple(x) for x in pq[s].tolist()] == [mb.rr_pair(np_, s, i) for i in range(np_ // 2)]
    seen = sorted(map(tuple, pq.reshape(-1, 2).tolist()))
    assert seen == list(itertools.combinations(range(np_), 2))             # every unordered pair exactly once


def test_jacobi_cs(core):
    rng = np.random.default_rng(11)
    t = rng.standard_normal((10000, 3)) * 10.0 ** rng.integers(-8, 9, (10000, 3))
    big = np.sqrt(np.finfo(np.float64).max) * 4.0                        # theta = +-big / 2: theta^2 overflows, tt = 0
    edges = np.array([[1.0, 2.0, 0.0], [3.0, 3.0, 0.0],                  # apq = 0 (the second: 0 / 0 behind the test)
                      [3.0, 3.0, 0.5], [3.0, 3.0, -0.5],                 # app = aqq: theta = +-0
                      [0.0, big, 1.0], [0.0, big, -1.0], [big, 0.0, 1.0],
                      [1.0, 2.0, 0.25], [2.0, 1.0, 0.25], [1.0, 2.0, -0.25]])   # both signs of theta
    t = np.vstack([t, edges])
    app, aqq, apq = (np.ascontiguousarray(t[:, k]) for k in range(3))
    c = np.empty(len(t)); s = np.empty(len(t))
    core.jc_cs(len(t), app.ctypes.data, aqq.ctypes.data, apq.ctypes.data, c.ctypes.data, s.ctypes.data)
    cm, sm = mb.jacobi_cs(app, aqq, apq)
    assert np.array_equal(c.view(np.int64), cm.view(np.int64)) and np.array_equal(s.view(np.int64), sm.view(np.int64))
    ne = len(edges)
    assert np.all(c[-ne:-ne + 2] == 1.0) and np.all(s[-ne:-ne + 2] == 0.0)
    assert np.all(c[-ne + 4:-ne + 7] == 1.0) and np.all(s[-ne + 4:-ne + 7] == 0.0)   # tt = 0
    assert s[-3] > 0 and s[-2] < 0 and s[-1] < 0                           # the sign of theta


def test_jacobi_converged(core):
    """A grid that straddles every clause: off at 1e-60; off / d2 at 1e-32; sweep 11 and 12; off / d2 at the rounding floor (nd 64 and 180: the n^2
    term, 8.1e-28 and 6.4e-27; nd 16: the fixed 1e-28 exceeds it); off / prev_off on both sides of 0.25."""
    near = lambda x: [np.nextafter(x, 0.0), x, np.nextafter(x, np.inf)]
    cases, hit = 0, {True: 0, False: 0}
    for nd in (16, 64, 180):
        floor_rel = max(1e-28, 4.0 * nd * nd * 4.93e-32)
        assert (floor_rel > 1e-28) == (nd > 16)
        for d2 in (1.0, 3.7e9):
            offs = near(1e-60) + near(1e-32 * d2) + near(floor_rel * d2) + [0.5 * floor_rel * d2, 2.0 * floor_rel * d2, 1e-20 * d2]
            for off, sweep, ratio in itertools.product(offs, (0, 11, 12, 13), (0.2, np.nextafter(0.25, 0.0), 0.25, np.nextafter(0.25, 1.0), 0.9)):
                for prev in (off / ratio, 1e300):
                    want = mb.converged(off, d2, nd, sweep, prev)
                    assert bool(core.jc_converged(off, d2, nd, sweep, prev)) == want, (off, d2, nd, sweep, prev)
                    cases += 1; hit[bool(want)] += 1
    assert hit[True] > 100 and hit[False] > 100, hit
