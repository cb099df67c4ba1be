"""NumPy restatement of landmark triangulation and anchor shift (the reference for tests/test_tri_reference.py and
tests/test_gpu_triangulate.py): what ctvio_triangulate(_batch) and ctvio_shift_anchor_batch (include/ctvio.h) compute, from a Window.

Poses come from ctrl-vio_amd/splines.py:eval_spline at integer-ns times formed as the factors form them (truncated integer-ns line delay,
times relative to t0_ns); the depth comes from np.linalg.svd.  hestenes_depth is a model of the device kernel's iteration (same pair order,
rotation formula and stop rule; csrc/kernels_tri.hpp) for the CPU tests.
"""
import importlib

import numpy as np

cv = importlib.import_module("ctrl-vio_amd")
sp = cv.splines

SKIPPED, OK, INIT, NONE = 0, 1, 2, 3
ORTH_TOL, MAX_SWEEPS = 1e-15, 30          # csrc/kernels_tri.hpp: TRI_ORTH_TOL, TRI_MAX_SWEEPS
MARGIN = 1e-3                             # no triangulated depth of a fixture may lie this close to min_depth: its flag would be a coin toss


def cam_poses(w, t_ns, rows, row_times):
    """Camera poses (R (n,3,3), p (n,3), inside (n,)) of observations (absolute t_ns, rows) at w's state."""
    t_rel = np.asarray(t_ns, np.int64) - np.int64(w.t0_ns)
    tau = t_rel + (np.asarray(rows, np.int64) * np.int64(int(w.ld * 1e9)) if row_times else 0)
    inside = (tau >= 0) & (tau // np.int64(w.dt_ns) <= w.K - 4)
    e = sp.eval_spline(w.quat, w.pos, 0, w.dt_ns, np.where(inside, tau, 0), want=("q", "p"))
    p = e["p"] + sp.qrot(e["q"], w.p_CI[None, :])
    q = sp.qmul(e["q"], w.q_CI[None, :])
    return sp.quat_to_R(q), p, inside


def landmark_observations(w, l):
    """Blocks of landmark l in the caller's order -> (block indices, True if they name exactly one anchor observation)."""
    idx = np.flatnonzero(w.v_lm == l)
    if idx.size == 0:
        return idx, False
    a = idx[0]
    one = all(w.v_ti[v] == w.v_ti[a] and w.v_rowi[v] == w.v_rowi[a] and np.array_equal(w.v_pi[v], w.v_pi[a]) for v in idx)
    return idx, one


def build_A(w, l, row_times):
    """The 2 (n + 1) x 4 matrix of landmark l (rows: anchor first, then the blocks in the caller's order), or None when it is not triangulable."""
    idx, one = landmark_observations(w, l)
    if not one:
        return None
    a = idx[0]
    t = np.concatenate([[w.v_ti[a]], w.v_tj[idx]]); rows = np.concatenate([[w.v_rowi[a]], w.v_rowj[idx]])
    pts = np.vstack([w.v_pi[a][None, :], w.v_pj[idx]])
    R, p, inside = cam_poses(w, t, rows, row_times)
    if not inside.all():
        return None
    A = np.zeros((2 * t.shape[0], 4))
    R0, t0 = R[0], p[0]
    for k in range(t.shape[0]):
        tk = R0.T @ (p[k] - t0)
        Rk = R0.T @ R[k]
        P = np.hstack([Rk.T, (-Rk.T @ tk)[:, None]])
        f = np.array([pts[k, 0], pts[k, 1], 1.0]); f /= np.linalg.norm(f)
        A[2 * k] = f[0] * P[2] - f[2] * P[0]
        A[2 * k + 1] = f[1] * P[2] - f[2] * P[1]
    return A


def svd_depth(A):
    v = np.linalg.svd(A)[2][-1]
    return v[2] / v[3]


def singular_values(A):
    return np.linalg.svd(A, compute_uv=False)


def hestenes_depth(A, tol=ORTH_TOL, max_sweeps=MAX_SWEEPS):
    """One-sided Jacobi on the columns of A as k_triangulate runs it -> (depth, sweeps used)."""
    A = np.array(A, np.float64)
    V = np.eye(4)
    sweeps = 0
    for sweeps in range(1, max_sweeps + 1):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                al, be, ga = A[:, p] @ A[:, p], A[:, q] @ A[:, q], A[:, p] @ A[:, q]
                if abs(ga) > tol * np.sqrt(al * be):
                    rotated = True
                    zeta = (be - al) / (2.0 * ga)
                    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / np.sqrt(1.0 + t * t); s = c * t
                    for M in (A, V):
                        mp, mq = M[:, p].copy(), M[:, q].copy()
                        M[:, p] = c * mp - s * mq; M[:, q] = s * mp + c * mq
        if not rotated:
            break
    j = int(np.argmin((A * A).sum(0)))
    return V[2, j] / V[3, j], sweeps


def normal_eig_depth(A):
    """The depth from the eigenvectors of A^T A (what the kernel deliberately does not do)."""
    v = np.linalg.eigh(A.T @ A)[1][:, 0]
    return v[2] / v[3]


def triangulate_ref(w, row_times=1, only_unset=0, min_depth=0.1, init_depth=5.0, depth_of=svd_depth):
    """-> (depth (L,), flag (L,), raw (L,): the triangulated value before the min_depth test, NaN where there is none).  Asserts that no
    triangulated value lies within MARGIN of min_depth."""
    L = w.L
    depth = np.zeros(L); flag = np.zeros(L, np.int32); raw = np.full(L, np.nan)
    with np.errstate(divide="ignore"):
        inv = 1.0 / w.rho
    for l in range(L):
        if only_unset and w.rho[l] > 0:
            depth[l], flag[l] = inv[l], SKIPPED
            continue
        A = build_A(w, l, row_times)
        if A is None:
            depth[l], flag[l] = inv[l], NONE
            continue
        d = depth_of(A)
        raw[l] = d
        assert not np.isfinite(d) or abs(d - min_depth) > MARGIN, f"landmark {l}: triangulated depth {d} is borderline against min_depth"
        if np.isfinite(d) and d >= min_depth:
            depth[l], flag[l] = d, OK
        else:
            depth[l], flag[l] = init_depth, INIT
    return depth, flag, raw


def shift_ref(w, lm, t_new, row_new, row_times, init_depth=5.0):
    """Depths of landmarks lm (n,) in the frame of new anchor observations (absolute t_new, row_new) -> (depth_new, flag, raw: the value
    before the sign test).  Asserts that no shifted depth lies within MARGIN of zero."""
    lm = np.asarray(lm); n = lm.shape[0]
    row_new = np.zeros(n, np.int64) if row_new is None else np.asarray(row_new)
    depth = np.full(n, np.nan); flag = np.full(n, NONE, np.int32); raw = np.full(n, np.nan)
    for i in range(n):
        l = int(lm[i])
        idx, one = landmark_observations(w, l)
        if not one or not w.rho[l] > 0:
            continue
        a = idx[0]
        R, p, inside = cam_poses(w, [w.v_ti[a], t_new[i]], [w.v_rowi[a], row_new[i]], row_times)
        if not inside.all():
            continue
        z = 1.0 / w.rho[l]
        pts = np.array([w.v_pi[a, 0] * z, w.v_pi[a, 1] * z, z])
        d = (R[1].T @ (R[0] @ pts + p[0] - p[1]))[2]
        raw[i] = d
        assert abs(d) > MARGIN, f"query {i}: shifted depth {d} is borderline against zero"
        depth[i], flag[i] = (d, OK) if d > 0 else (init_depth, INIT)
    return depth, flag, raw


def rel_err(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))
