"""CPU: the walk of the order-fixed wide-window assembly (deterministic = 2; csrc/host_pack.hpp: plan_row_walk, read by
csrc/kernels_assemble.hpp: k_assemble_wide) against its Python mirror (packer.row_walk), and what the kernel relies on: every block slot
exactly once, each row's slots belong to that row's landmark in ascending slot order, and the blocks that can reach a 16-column tile are
inside the contiguous stretch of rows [tl_beg, tl_end) the tile walks -- for the benchmarked shapes, the long windows and a window with
unobserved landmarks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_sparsity_plan import hp, plan  # noqa: F401  (fixture + helper)

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INC = "/opt/rocm/include"


@pytest.fixture(scope="module")
def hw():
    if not os.path.isdir(ROCM_INC):
        pytest.skip("HIP headers not found")
    out = os.path.join(HERE, "_build", "libhostwalk.so")
    src = os.path.join(HERE, "host_walk_check.cpp")
    hdrs = [os.path.join(HERE, "..", "ctrl-vio_amd", "csrc", f) for f in ("host_pack.hpp", "device_types.hpp")] + [os.path.join(HERE, "..", "include", "ctvio.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I", ROCM_INC, "-o", out, src, "-L/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return C.CDLL(out)


def host_walk(hw, cv, w):
    keep = []
    cw = cv.capi.to_cwindow(w, keep)
    cap = w.V + 64 * (w.L + 1)
    lord = np.zeros(cap, np.int32); lm_pos = np.zeros(max(w.L, 1), np.int32); vrow = np.zeros(max(w.V, 1), np.int32); off = np.zeros(w.L + 1, np.int32)
    Vp = C.c_int32()
    err = C.create_string_buffer(256)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = hw.hw_row_walk(C.byref(cw), cap, C.byref(Vp), p(lord), p(lm_pos), p(vrow), p(off), err, 256)
    assert rc == 0, (rc, err.value.decode())
    return lord[:Vp.value], lm_pos[:w.L], vrow[:w.V], off


def unobserved(cv):
    w = cv.synth.make_window("config1", seed=1501)
    keep = np.random.default_rng(5).random(w.V) < 0.6
    keep[w.v_lm == 7] = False
    for a in ("v_lm", "v_ti", "v_tj", "v_rowi", "v_rowj", "v_pi", "v_pj"):
        setattr(w, a, getattr(w, a)[keep])
    return w.normalize()


CASES = [("config5", 1011, {}), ("config5_spread", 1011, {}), ("config2", 1000, {}), ("config2", 1000, dict(dt_ns=10_000_000)),
         ("config5_spread", 1000, dict(dt_ns=23_000_000)), ("tiny", 3, {}), ("unobserved", 0, {})]


@pytest.mark.parametrize("cfg,seed,kw", CASES, ids=[f"{c}-{s}-{len(k)}" for c, s, k in CASES])
def test_row_walk_equals_mirror_and_covers_the_tiles(hw, hp, cv, cfg, seed, kw):
    w = unobserved(cv) if cfg == "unobserved" else cv.synth.make_window(cfg, seed=seed, **kw)
    lord, lm_pos, vrow, off = host_walk(hw, cv, w)
    mv, mo = cv.packer.row_walk(lord, w.v_lm, lm_pos)
    assert np.array_equal(vrow, mv) and np.array_equal(off, mo)
    # every block slot exactly once; row r holds the slots of landmark lm_at[r], ascending
    assert sorted(vrow.tolist()) == np.flatnonzero(lord >= 0).tolist()
    lm_at = np.argsort(lm_pos)
    for r in range(w.L):
        s = vrow[off[r]:off[r + 1]]
        assert np.all(np.diff(s) > 0)
        assert np.all(w.v_lm[lord[s]] == lm_at[r])
    # a block whose landmark's planned span reaches a knot tile lies in that tile's stretch of rows
    pl = plan(hp, cv, w)
    K6 = 6 * w.K
    for c in range(K6 // 16 + (1 if K6 % 16 else 0)):
        if 16 * c + 15 >= K6:
            continue                                            # (k_assemble_wide walks every observed row there)
        kf, kl = 16 * c // 6, (16 * c + 15) // 6
        rows = [r for r in range(pl["Lobs"]) if pl["klo"][r] <= kl and pl["khi"][r] >= kf]
        assert all(pl["tl_beg"][c] <= r < pl["tl_end"][c] for r in rows), c
