"""Test-only access to the case bodies of tests/math_cases.hpp in both builds: `Device` runs them on the GPU through
tests/_build/libdevprobe.so (tests/device_math_probe.hip, compiled with the product's hipcc line), `Host` through the g++ libraries of
tests/host_math_check.cpp and tests/host_lspoly_check.cpp.  Both take and return arrays with one case per row, so a check written once runs
on either.  The product never loads any of this."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
PROBE_SRC = os.path.join(HERE, "device_math_probe.hip")
PROBE_LIB = os.path.join(BUILD, "libdevprobe.so")
CASES_HDR = os.path.join(HERE, "math_cases.hpp")
BATCHES = (1, 64, 65, 130)   # one thread; one full block; a second block of one thread; two blocks and a ragged third


def _capi():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("ctrl-vio_amd").capi


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in deps)


def build_probe(force=False, verbose=False):
    """Cross-compiles the probe for gfx950 (no GPU needed) with exactly the command of libctvio.so: capi.hipcc_command."""
    capi = _capi()
    hdrs = [f for f in capi.SRC if f.endswith(".hpp")]
    os.makedirs(BUILD, exist_ok=True)
    if force or _stale(PROBE_LIB, [PROBE_SRC, CASES_HDR] + hdrs):
        cmd = capi.hipcc_command(PROBE_LIB, PROBE_SRC)
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return PROBE_LIB


def load_probe():
    """dlopen the probe (raises if it has not been built: the GPU test compiles nothing)."""
    if not os.path.exists(PROBE_LIB):
        raise RuntimeError(f"{PROBE_LIB} missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    return C.CDLL(PROBE_LIB)


def host_lib(name, src):
    """g++ -O2 build of one tests/host_*_check.cpp, as the fixtures of the host tests build theirs."""
    out = os.path.join(BUILD, name)
    srcp = os.path.join(HERE, src)
    hdrs = [os.path.join(ROOT, "ctrl-vio_amd", "csrc", f) for f in ("so3.hpp", "factors.hpp", "ls_poly.hpp")] + [CASES_HDR]
    os.makedirs(BUILD, exist_ok=True)
    if _stale(out, [srcp] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, srcp])
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _rows(a, n, width):
    """n cases x width doubles, C-contiguous; a single case's values are repeated for every case"""
    a = np.asarray(a, np.float64)
    if a.size == width:
        a = np.broadcast_to(a.reshape(1, width), (n, width))
    return np.array(a.reshape(n, width), dtype=np.float64, order="C", copy=True)   # (a copy: a broadcast view is read-only)


class Device:
    """Each method: one launch per batch of BATCHES (then batches of 130), every HIP status checked.  A family with fewer than
    sum(BATCHES) = 260 cases is sent with its cases repeated cyclically up to 260 rows, so that every entry runs a full block, a second
    block of one thread and a ragged third block; a repeated case must come back with the bits of its first copy."""

    def __init__(self):
        self.lib = load_probe()
        self.launches = 0

    def _run(self, name, n, args):
        """args: 2-D arrays with one case per row (sliced per batch; written in place where the entry writes) or ctypes scalars (passed
        to every batch)"""
        fn = getattr(self.lib, name)
        fn.restype = C.c_int
        N = max(n, sum(BATCHES))
        rows = np.arange(N) % n
        sent = [np.ascontiguousarray(a[rows]) if isinstance(a, np.ndarray) else a for a in args]
        lo, k = 0, 0
        while lo < N:
            hi = min(N, lo + (BATCHES[k] if k < len(BATCHES) else BATCHES[-1]))
            call = [C.c_int(hi - lo)] + [_p(a[lo:hi]) if isinstance(a, np.ndarray) else a for a in sent]
            st = fn(*call)
            if st != 0:
                raise RuntimeError(f"{name}: HIP status {st} on cases [{lo}, {hi})")
            self.launches += 1
            lo, k = hi, k + 1
        for a, t in zip(args, sent):
            if isinstance(a, np.ndarray):
                if not np.array_equal(t, t[:n][rows], equal_nan=True):
                    raise AssertionError(f"{name}: a repeated case differs from its first copy (thread or batch dependence)")
                a[...] = t[:n]

    # ---- Lie primitives
    def so3(self, phi):
        n = len(phi); phi = _rows(phi, n, 3)
        q, Jr, Ji, lg = np.zeros((n, 4)), np.zeros((n, 9)), np.zeros((n, 9)), np.zeros((n, 3))
        self._run("dp_so3", n, [phi, q, Jr, Ji, lg])
        return q, Jr.reshape(n, 3, 3), Ji.reshape(n, 3, 3), lg

    def so3_small(self, phi):
        n = len(phi); phi = _rows(phi, n, 3)
        q, Jr = np.zeros((n, 4)), np.zeros((n, 9))
        self._run("dp_so3_small", n, [phi, q, Jr])
        return q, Jr.reshape(n, 3, 3)

    def so3_log(self, q):
        n = len(q); q = _rows(q, n, 4)
        lg = np.zeros((n, 3))
        self._run("dp_so3_log", n, [q, lg])
        return lg

    def qmul(self, a, b):
        n = len(a); a = _rows(a, n, 4); b = _rows(b, n, 4)
        o, ou = np.zeros((n, 4)), np.zeros((n, 4))
        self._run("dp_qmul", n, [a, b, o, ou])
        return o, ou

    def basis(self, u, idt):
        n = len(u)
        c = np.zeros((n, 24))
        self._run("dp_basis", n, [_rows(u, n, 1), _rows(idt, n, 1), c])
        return c.reshape(n, 6, 4)

    def ls_minimize(self, ns, x, v, g, lo, hi, coef=False):
        """the step; with coef also the 6 coefficients of the interpolating polynomial (highest power first, zeros behind the 2 ns)"""
        n = len(lo)
        step, cf = np.full((n, 1), np.nan), np.full((n, 6), np.nan)
        self._run("dp_ls_minimize", n, [C.c_int(ns), _rows(x, n, ns), _rows(v, n, ns), _rows(g, n, ns), _rows(lo, n, 1), _rows(hi, n, 1), step, cf])
        return (step[:, 0], cf) if coef else step[:, 0]

    def ls_roots(self, p):
        """p: n polynomials of the same number of coefficients (<= 5), highest power first -> (count, real parts; nan where none)"""
        p = np.ascontiguousarray(p, np.float64)
        n, m = p.shape
        re, cnt = np.full((n, 4), np.nan), np.full((n, 1), np.nan)
        self._run("dp_ls_roots", n, [C.c_int(m), p, re, cnt])
        return cnt[:, 0].astype(int), re

    # ---- blocks and query Jacobians (arguments as the hm_* wrappers of the host checks, one case per row)
    def imu_eval(self, q, p, u, idt, g, bias, gyro, acc, w):
        n = len(u)
        r, J = np.zeros((n, 6)), np.zeros((n, 180))
        self._run("dp_imu_eval", n, [_rows(q, n, 16), _rows(p, n, 12), _rows(u, n, 1), _rows(idt, n, 1), _rows(g, n, 3), _rows(bias, n, 6),
                                     _rows(gyro, n, 3), _rows(acc, n, 3), _rows(w, n, 6), r, J])
        return r, J.reshape(n, 6, 30)

    def visual_eval(self, small, qi, pi, qj, pj, sc, q_CI, p_CI, obs):
        """sc: (ui, uj, idt, img_w, cauchy_a, rowi, rowj, d_inv) per case"""
        n = len(sc)
        r, J, cost = np.zeros((n, 2)), np.zeros((n, 100)), np.zeros((n, 1))
        self._run("dp_visual_eval", n, [C.c_int(int(small)), _rows(qi, n, 16), _rows(pi, n, 12), _rows(qj, n, 16), _rows(pj, n, 12), _rows(sc, n, 8),
                                        _rows(q_CI, n, 4), _rows(p_CI, n, 3), _rows(obs, n, 4), r, J, cost])
        return r, J.reshape(n, 2, 50), cost[:, 0]

    def pose_jac(self, q, u, ext, q_SI, p_SI):
        n = len(u)
        jt = np.zeros((n, 144))
        self._run("dp_pose_jac", n, [_rows(q, n, 16), _rows(u, n, 1), C.c_int(int(ext)), _rows(q_SI, n, 4), _rows(p_SI, n, 3), jt])
        return jt.reshape(n, 24, 6)

    def nav_jac(self, q, u, idt):
        n = len(u)
        jt, cv = np.zeros((n, 144)), np.zeros((n, 4))
        self._run("dp_nav_jac", n, [_rows(q, n, 16), _rows(u, n, 1), _rows(idt, n, 1), jt, cv])
        return jt.reshape(n, 24, 6), cv

    def rates_jac(self, q, p, u, idt, g):
        n = len(u)
        jt = np.full((n, 216), np.nan)
        self._run("dp_rates_jac", n, [_rows(q, n, 16), _rows(p, n, 12), _rows(u, n, 1), _rows(idt, n, 1), _rows(g, n, 3), jt])
        return jt.reshape(n, 24, 9)

    def rel_pose_jac(self, qa, pa, ua, qb, pb, ub, ext, q_SI, p_SI):
        n = len(ua)
        jt_a, jt_b, rel7 = np.zeros((n, 144)), np.zeros((n, 144)), np.zeros((n, 7))
        self._run("dp_rel_pose_jac", n, [_rows(qa, n, 16), _rows(pa, n, 12), _rows(ua, n, 1), _rows(qb, n, 16), _rows(pb, n, 12), _rows(ub, n, 1),
                                         C.c_int(int(ext)), _rows(q_SI, n, 4), _rows(p_SI, n, 3), jt_a, jt_b, rel7])
        return jt_a.reshape(n, 24, 6), jt_b.reshape(n, 24, 6), rel7

    def proj_jac(self, qa, pa, ua, qq, pq, uq, idt, q_CI, p_CI, obs3, rows):
        n = len(ua)
        jt_a, jt_q, out7 = np.zeros((n, 48)), np.zeros((n, 48)), np.zeros((n, 7))
        self._run("dp_proj_jac", n, [_rows(qa, n, 16), _rows(pa, n, 12), _rows(ua, n, 1), _rows(qq, n, 16), _rows(pq, n, 12), _rows(uq, n, 1),
                                     _rows(idt, n, 1), _rows(q_CI, n, 4), _rows(p_CI, n, 3), _rows(obs3, n, 3), _rows(rows, n, 2), jt_a, jt_q, out7])
        return jt_a.reshape(n, 24, 2), jt_q.reshape(n, 24, 2), out7

    def pred_jac(self, q_e, p_e, v_e, w_e, delta, X, q_CI, p_CI):
        n = len(delta)
        pose7, proj3, B, Cx, A = np.zeros((n, 7)), np.zeros((n, 3)), np.zeros((n, 90)), np.zeros((n, 36)), np.zeros((n, 30))
        self._run("dp_pred_jac", n, [_rows(q_e, n, 4), _rows(p_e, n, 3), _rows(v_e, n, 3), _rows(w_e, n, 3), _rows(delta, n, 1), _rows(X, n, 3),
                                     _rows(q_CI, n, 4), _rows(p_CI, n, 3), pose7, proj3, B, Cx, A])
        return pose7, proj3, B.reshape(n, 6, 15), Cx.reshape(n, 6, 6), A.reshape(n, 2, 15)

    def imu_step(self, x, meas, g, dt, want_blocks=True):
        """returns (x advanced, blocks or None)"""
        n = len(dt)
        x = _rows(x, n, 16).copy()
        blocks = np.zeros((n, 63)) if want_blocks else None
        self._run("dp_imu_step", n, [x, _rows(meas, n, 12), _rows(g, n, 3), _rows(dt, n, 1), blocks if want_blocks else C.c_void_p(None)])
        return x, (blocks.reshape(n, 7, 3, 3) if want_blocks else None)


class Host:
    """The Lie primitives and the line-search step of the g++ build, case by case, in the batch interface of Device."""

    def __init__(self):
        self.hm = host_lib("libhostmath.so", "host_math_check.cpp")
        self.hl = host_lib("libhostlspoly.so", "host_lspoly_check.cpp")
        self.hl.hl_ls_minimize.restype = C.c_double
        self.hl.hl_ls_minimize.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_double] * 2 + [C.c_void_p]
        self.hl.hl_ls_roots.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        self.hm.hm_basis.argtypes = [C.c_double, C.c_double, C.c_void_p]

    def so3(self, phi):
        n = len(phi); phi = _rows(phi, n, 3)
        q, Jr, Ji, lg = np.zeros((n, 4)), np.zeros((n, 9)), np.zeros((n, 9)), np.zeros((n, 3))
        for i in range(n):
            self.hm.hm_so3(_p(phi[i]), _p(q[i]), _p(Jr[i]), _p(Ji[i]), _p(lg[i]))
        return q, Jr.reshape(n, 3, 3), Ji.reshape(n, 3, 3), lg

    def so3_small(self, phi):
        n = len(phi); phi = _rows(phi, n, 3)
        q, Jr = np.zeros((n, 4)), np.zeros((n, 9))
        for i in range(n):
            self.hm.hm_so3_small(_p(phi[i]), _p(q[i]), _p(Jr[i]))
        return q, Jr.reshape(n, 3, 3)

    def so3_log(self, q):
        n = len(q); q = _rows(q, n, 4)
        lg = np.zeros((n, 3))
        for i in range(n):
            self.hm.hm_so3_log(_p(q[i]), _p(lg[i]))
        return lg

    def qmul(self, a, b):
        n = len(a); a = _rows(a, n, 4); b = _rows(b, n, 4)
        o, ou = np.zeros((n, 4)), np.zeros((n, 4))
        for i in range(n):
            self.hm.hm_qmul(_p(a[i]), _p(b[i]), _p(o[i]), _p(ou[i]))
        return o, ou

    def basis(self, u, idt):
        n = len(u)
        c = np.zeros((n, 24))
        for i in range(n):
            self.hm.hm_basis(float(u[i]), float(idt[i]), _p(c[i]))
        return c.reshape(n, 6, 4)

    def ls_minimize(self, ns, x, v, g, lo, hi, coef=False):
        n = len(lo)
        x, v, g = _rows(x, n, ns), _rows(v, n, ns), _rows(g, n, ns)
        cf = np.full((n, 6), np.nan)
        step = np.array([self.hl.hl_ls_minimize(ns, _p(x[i]), _p(v[i]), _p(g[i]), float(lo[i]), float(hi[i]), _p(cf[i])) for i in range(n)])
        return (step, cf) if coef else step

    def ls_roots(self, p):
        p = np.ascontiguousarray(p, np.float64)
        n, m = p.shape
        re = np.full((n, 4), np.nan)
        cnt = np.array([self.hl.hl_ls_roots(m, _p(p[i]), _p(re[i])) for i in range(n)])
        return cnt, re
