"""CPU: the oracle's marginalisation prior (oracle/ctvo.c: ctvo_prior_residual, the prior part of ctvo_build_normal) pinned on the dense,
all-kind priors of tests/prior_helpers.py against np_oracle's restatement (scipy rotations) and a NumPy normal-equation build with its own
column map -- the GPU prior tests (test_gpu_prior.py) compare against this oracle.  Also: the host's validation refuses a prior that lists
the same (kind, index) twice (Ceres refuses duplicate parameter blocks in one residual block)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_oracle
import prior_helpers as ph

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INC = "/opt/rocm/include"


def _windows(cv):
    """(name, window): partial / full priors on tiny and config1, and one over constant blocks."""
    out = []
    for cfg, seed in (("tiny", 3), ("config1", 1000)):
        base = cv.synth.make_window(cfg, seed=seed)
        out.append((f"{cfg}-partial", ph.dense_prior_window(base, seed + 1)))
        out.append((f"{cfg}-full", ph.dense_prior_window(base, seed + 2, full=True)))
    c = cv.synth.make_window("tiny", seed=4)
    c.fixed_upto = 1
    kc = np.zeros(c.K, np.uint8); kc[6] = 1
    c.knot_const = kc
    c.lock_bg = True; c.fix_ld = True
    out.append(("tiny-const", ph.dense_prior_window(c.normalize(), 9, with_const=True)))
    return out


def _prior_only_window(cv, seed, **kw):
    """K knots, F bias states, nothing but the prior (M = V = NB = L = 0)."""
    rng = np.random.default_rng(seed)
    K, F = 6, 3
    q = rng.normal(size=(K, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w = cv.Window(t0_ns=0, dt_ns=50_000_000, quat=q, pos=rng.normal(size=(K, 3)), bias=rng.normal(0.0, 0.01, (F, 6)), rho=np.zeros(0),
                  ld=1.5e-5).normalize()
    return ph.dense_prior_window(w, seed + 1, **kw)


def test_prior_residual_matches_the_numpy_restatement(cv, oracle):
    """ctvo_prior_residual == np_oracle's r0 + J0 dx (scipy rotations, its own sign fix) on non-symmetric J0, shuffled block offsets,
    every block kind and negated-quaternion blocks; negating every ROT x0 leaves dx bit-for-bit unchanged (q and -q: one rotation)."""
    for name, w in _windows(cv):
        assert ph.has_negated_rotation(w), name
        assert not np.allclose(w.pJ0, w.pJ0.T), name
        assert set(w.p_kind.tolist()) == {0, 1, 2, 3, 4}, name
        r, dx = oracle.OracleWindow(w).prior_residual()
        rn = np_oracle.residuals(w)["prior"]
        assert np.abs(r - rn).max() <= 1e-12 * max(np.abs(rn).max(), 1.0), name
        # dx restated here: aligning x0 with the knot's quaternion first is the sign fix (the angle of q0^-1 q is ~1e-3 rad)
        col = ph.prior_columns(w)
        assert np.abs(w.pr0 + w.pJ0 @ dx - r).max() <= 1e-12 * max(np.abs(r).max(), 1.0), name
        for kind, idx, off, x0 in zip(w.p_kind, w.p_index, w.p_off, w.p_x0):
            if kind == ph.PK_ROT:
                q0 = x0 if np.dot(x0, w.quat[idx]) >= 0 else -x0
                assert np.abs(dx[off:off + 3] - 2 * ph._qmul(q0 * [-1, -1, -1, 1], w.quat[idx])[:3]).max() < 1e-15, name
                assert np.abs(dx[off:off + 3]).max() < 1e-2, name
        assert (col >= 0).all() and np.unique(col).size == w.pn, name
        flipped = w.copy()
        flipped.p_x0 = np.where((flipped.p_kind == ph.PK_ROT)[:, None], -flipped.p_x0, flipped.p_x0)
        r2, dx2 = oracle.OracleWindow(flipped).prior_residual()
        assert np.array_equal(dx2, dx) and np.array_equal(r2, r), name


@pytest.mark.parametrize("kw", [dict(), dict(full=True), dict(n_knots=2, n_bias=1, negate=2)])
def test_prior_only_normal_equations(cv, oracle, kw):
    """A prior-only window: OracleWindow.build_normal() == J^T J, J^T r, |r|^2 / 2 with J = J0 placed in the columns of the kept blocks'
    unknowns (column map built here from the unknown ordering, r from np_oracle) -- pins J0's column-major layout and the BG / BA / LD
    unknown indices."""
    w = _prior_only_window(cv, 77, **kw)
    assert w.M == w.V == w.NB == w.L == 0
    H, g, cost = oracle.OracleWindow(w.copy()).build_normal()
    r = np_oracle.residuals(w)["prior"]
    K, F, N = w.K, w.F, w.N
    J = np.zeros((w.pn, N))
    for kind, idx, off in zip(w.p_kind, w.p_index, w.p_off):
        u0 = {0: 6 * idx, 1: 6 * idx + 3, 2: 6 * K + 6 * idx, 3: 6 * K + 6 * idx + 3, 4: 6 * K + 6 * F}[int(kind)]
        n = 1 if kind == 4 else 3
        J[:, u0:u0 + n] += w.pJ0[:, off:off + n]
    Hn, gn, cn = J.T @ J, J.T @ r, 0.5 * float(r @ r)
    assert cost == pytest.approx(cn, rel=1e-12)
    assert np.abs(H - Hn).max() <= 1e-12 * np.abs(Hn).max()
    assert np.abs(g - gn).max() <= 1e-12 * np.abs(gn).max()
    # the same build with J0 read transposed is far off (the comparison above would see a row-major / column-major mix-up)
    Jt = np.zeros_like(J)
    for kind, idx, off in zip(w.p_kind, w.p_index, w.p_off):
        u0 = int(ph.prior_columns(w)[off])
        n = 1 if kind == 4 else 3
        Jt[:, u0:u0 + n] = w.pJ0.T[:, off:off + n]
    assert np.abs(Jt.T @ Jt - H).max() > 1e-3 * np.abs(H).max()
    # the columns outside the prior are empty; those inside are exactly the kept blocks' unknowns
    used = np.zeros(N, bool); used[ph.prior_columns(w)] = True
    assert not H[~used].any() and not g[~used].any()
    assert used.sum() == w.pn


@pytest.fixture(scope="module")
def hp():
    if not os.path.isdir(ROCM_INC):
        pytest.skip("HIP headers not found")
    out = os.path.join(HERE, "_build", "libhostplan.so")
    src = os.path.join(HERE, "host_plan_check.cpp")
    hdrs = [os.path.join(HERE, "..", "ctrl-vio_amd", "csrc", f) for f in ("host_pack.hpp", "device_types.hpp")] + [os.path.join(HERE, "..", "include", "ctvio.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I", ROCM_INC, "-o", out, src, "-L/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return C.CDLL(out)


def _validate(hp, cv, w):
    """host_pack.hpp validate_window (through the plan shim): (rc, message)."""
    keep = []
    cw = cv.capi.to_cwindow(w, keep)
    ntr = w.P // 16 + 1
    a = [np.zeros(max(n, 1), np.int32) for n in (w.L,) * 4 + (ntr,) * 4]
    Lobs, ms, nt = C.c_int32(), C.c_int32(), C.c_int32()
    err = C.create_string_buffer(256)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = hp.hp_sparsity(C.byref(cw), 0, 0, *[p(x) for x in a], C.byref(Lobs), C.byref(ms), C.byref(nt), err, 256)
    return rc, err.value.decode()


def test_host_validation_refuses_duplicate_prior_blocks(cv, hp):
    """Two kept blocks with the same (kind, index) at different offsets are refused (the store-semantics tail keeps one prior column per
    unknown while the atomic path and the oracle sum both; and only duplicates let pn exceed P); an LD block with index != 0 too.  The
    valid windows pass."""
    for name, w in _windows(cv):
        assert _validate(hp, cv, w)[0] == 0, name
        for kind in (ph.PK_ROT, ph.PK_POS, ph.PK_BG, ph.PK_BA, ph.PK_LD):
            rc, msg = _validate(hp, cv, ph.duplicate_block(w, kind))
            assert rc == 1 and "duplicate" in msg, (name, kind, msg)
    bad = _windows(cv)[0][1].copy()
    bad.p_index = bad.p_index.copy(); bad.p_index[bad.p_kind == ph.PK_LD] = 1
    rc, msg = _validate(hp, cv, bad)
    assert rc == 1 and "out of range" in msg, msg
