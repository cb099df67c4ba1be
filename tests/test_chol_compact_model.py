"""CPU: a NumPy model of the SLOT-INDEXED variant of k_cholesky_solve (csrc/kernels_solve.hpp, COMPACT = true): the it-th tile that takes
part in a panel is staged at LDS slot it; tiles beyond the slot budget overflow -- the L21 step reads A21 from S / y and the trailing update
reads the L21 rows back from S / y (columns jb .. jb + nb), masked like the LDS path.  Run on the reduced system of windows beyond 591
unknowns with every entry OUTSIDE the planned envelope set to NaN and the LDS panel starting as NaN: a NaN in the solution means the kernel
would read something nobody wrote.  The solution must equal the dense solve, and a budget that overflows must give the same bits as one that
does not.  Also: the host's slot count (host_pack.hpp: chol_panel_slots) equals its Python mirror (packer.chol_panel_slots)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_sparsity_plan import hp, plan  # noqa: F401  (fixture + helper)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
ROCM_INC = "/opt/rocm/include"


@pytest.fixture(scope="module")
def hs():
    if not os.path.isdir(ROCM_INC):
        pytest.skip("HIP headers not found")
    out = os.path.join(HERE, "_build", "libhostslots.so")
    src = os.path.join(HERE, "host_slots_check.cpp")
    hdrs = [os.path.join(HERE, "..", "ctrl-vio_amd", "csrc", f) for f in ("host_pack.hpp", "device_types.hpp")] + [os.path.join(HERE, "..", "include", "ctvio.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I", ROCM_INC, "-o", out, src, "-L/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    lib = C.CDLL(out)
    lib.hs_chol_slots.restype = C.c_int
    return lib


def host_slots(hs, env, P):
    e = np.ascontiguousarray(env, np.int32)
    return hs.hs_chol_slots(e.ctypes.data_as(C.c_void_p), int(P))


def long_window(cv, which):
    if which == "config2@10ms":
        return cv.synth.make_window("config2", seed=1000, dt_ns=10_000_000)        # K 107, P 709
    if which == "config5_spread@25ms":
        return cv.synth.make_window("config5_spread", seed=1000, dt_ns=25_000_000)  # K 125, P 937
    if which == "config2@10ms+prior":
        import prior_helpers as ph
        w = cv.synth.make_window("config2", seed=1000, dt_ns=10_000_000)
        return ph.dense_prior_window(w, 7, n_knots=w.K - 20, n_bias=w.F)          # the prior's kept blocks couple mutually: a dense envelope
    raise KeyError(which)


def slot_panel_cholesky_model(S, rhs, ef, slots):
    """S: (P, P) lower triangle used (NaN outside the envelope), rhs (P,), ef per 16-row tile (P // 16 + 1 entries), slots: the LDS budget in
    16-row tiles.  Returns (x, the most tiles that overflowed in one panel)."""
    S = S.copy(); y = rhs.copy()
    P = S.shape[0]
    Linv_blocks = {}
    most_over = 0
    for jb in range(0, P, 32):
        nb = min(32, P - jb); r0 = jb + nb; nt = P - r0; ntr = nt + 1
        ntile = (ntr + 15) // 16
        R0 = r0 >> 4
        plist = [t for t in range(ntile) if ef[min(R0 + t, P // 16)] <= (jb >> 4) + 1]
        most_over = max(most_over, len(plist) - slots)

        def from_S(t):                               # a tile's rows, columns jb .. jb + 32, as the kernel reads them from S / y (masked)
            out = np.zeros((16, 32))
            for i in range(16):
                r = 16 * t + i
                if r < ntr:
                    out[i, :nb] = S[r0 + r, jb:jb + nb] if r < nt else y[jb:jb + nb]
            return out

        A11 = np.tril(S[jb:jb + nb, jb:jb + nb])
        A11 = A11 + np.tril(A11, -1).T
        Linv = np.linalg.inv(np.linalg.cholesky(A11))
        Linv_blocks[jb // 32] = Linv
        lds = np.full((16 * slots, 32), np.nan)     # the slot-indexed panel (rows; the kernel keeps it k-major)
        for it, t in enumerate(plist[:slots]):       # staging: overflow tiles are not staged
            lds[16 * it:16 * it + 16] = from_S(t)
        for it, t in enumerate(plist):               # L21 = A21 L11^-T, into the slot (if any) and into S / y
            a = lds[16 * it:16 * it + 16].copy() if it < slots else from_S(t)
            l21 = np.zeros((16, 32))
            l21[:, :nb] = a[:, :nb] @ Linv.T
            if it < slots:
                lds[16 * it:16 * it + 16] = l21
            for i in range(16):
                r = 16 * t + i
                if r < nt:
                    S[r0 + r, jb:jb + nb] = l21[i, :nb]
                elif r == nt:
                    y[jb:jb + nb] = l21[i, :nb]
        if nt == 0:
            continue
        assert plist[:2] == [0, 1][:min(2, ntile)], (jb, plist)      # the next diagonal block takes part (look-ahead)
        # trailing update: operands from the slot, or (overflow) the L21 rows just stored into S / y -- read after every L21 store
        ops = [np.ascontiguousarray(lds[16 * it:16 * it + 16] if it < slots else from_S(t)) for it, t in enumerate(plist)]
        ii, jj = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
        for a in range(len(plist)):
            for b in range(a + 1):
                ti, tj = plist[a], plist[b]
                c = (ops[a][:, None, :] * ops[b][None, :, :]).sum(-1)   # (fixed summation order: the same operand bits give the same result)
                row, col = 16 * ti + ii, 16 * tj + jj
                m = (col < nt) & (((row < nt) & (col <= row)) | (row == nt))
                ms = m & (row < nt)
                S[r0 + row[ms], r0 + col[ms]] -= c[ms]
                my = m & (row == nt)
                y[r0 + col[my]] -= c[my]
    xs = y.copy()
    for b in range((P + 31) // 32 - 1, -1, -1):
        jb = 32 * b; nb = min(32, P - jb)
        ca = 16 * ef[2 * b]; cb = 16 * ef[min(2 * b + 1, P // 16)]
        xb = Linv_blocks[b].T @ xs[jb:jb + nb]
        xs[jb:jb + nb] = xb
        for j in range(min(ca, cb), jb):
            s = 0.0
            for ii_ in range(nb):
                if j >= (ca if ii_ < 16 else cb):
                    s += S[jb + ii_, j] * xb[ii_]
            xs[j] -= s
    return xs, most_over


@pytest.mark.parametrize("which", ["config2@10ms", "config2@10ms+prior"])
def test_slot_indexed_panel_with_overflow(hp, cv, oracle, which):
    w = long_window(cv, which)
    P = w.P
    assert 591 < P <= 1024                           # the slot-indexed variant's territory
    ef = plan(hp, cv, w)["env"]
    H, g, cost = oracle.OracleWindow(w.copy()).build_normal()
    Hpp, W, Hll = H[:P, :P], H[:P, P:], np.diag(H)[P:]
    D = 1e-4 * np.diag(Hpp) + 1e-6
    dl = 1e-4 * Hll + 1e-6
    S = Hpp + np.diag(D) - (W / (Hll + dl)) @ W.T
    rhs = -g[:P] + (W / (Hll + dl)) @ g[P:]
    Sm = np.full((P, P), np.nan)
    for i in range(P):
        c0 = 16 * ef[i // 16]
        Sm[i, c0:i + 1] = S[i, c0:i + 1]
        assert np.all(S[i, :c0] == 0.0)              # (what the plan drops is structurally zero)
    need = cv.packer.chol_panel_slots(P, ef)
    x_full, over_full = slot_panel_cholesky_model(Sm, rhs, ef, 64)
    x_small, over_small = slot_panel_cholesky_model(Sm, rhs, ef, 8)
    assert over_full <= 0 and over_small == need - 8 > 0
    assert np.all(np.isfinite(x_full)) and np.all(np.isfinite(x_small))
    xd = np.linalg.solve(S, rhs)
    assert np.abs(x_full - xd).max() <= 1e-9 * np.abs(xd).max()
    assert np.array_equal(x_small, x_full)           # the overflow route reads the same operand bits
    if which.endswith("+prior"):
        assert need > 35                             # a dense envelope over the prior: more tiles than 160 KB of LDS hold


@pytest.mark.parametrize("which", ["config2@10ms", "config5_spread@25ms", "config2@10ms+prior"])
def test_host_slot_count_equals_mirror(hp, hs, cv, which):
    w = long_window(cv, which)
    P = w.P
    env_host = plan(hp, cv, w)["env"]
    env_py = cv.packer.reduced_system_envelope(w)
    assert np.array_equal(env_host, env_py)
    n = host_slots(hs, env_host, P)
    assert n == cv.packer.chol_panel_slots(P, env_py)
    dense = np.zeros(P // 16 + 1, np.int32)          # CTVIO_DENSE=1: every tile below the panel takes part
    assert host_slots(hs, dense, P) == cv.packer.chol_panel_slots(P, dense) == (P - 32 + 1 + 15) // 16
    expected = {"config2@10ms": 31, "config5_spread@25ms": 23}   # (the sizes quoted for the planner's shapes at seed 1000)
    if which in expected:
        assert n == expected[which]


def test_slot_count_of_todays_largest_window(hs, cv):
    w = cv.synth.make_window("config5", seed=1000)   # K 64, P 571: the largest shape of the full-height panel
    env = cv.packer.reduced_system_envelope(w)
    assert host_slots(hs, env, w.P) == cv.packer.chol_panel_slots(w.P, env) == 14
