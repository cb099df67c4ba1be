"""Python host side above the C ABI: a batch of sliding windows solved on one MI355X.

Mirrors the call pattern of the reference's TrajectoryManager::UpdateTrajectory
(src/estimator/trajectory_manager.cpp:350-463): build an estimator, add the window's factors,
Solve(max_iterations), copy the state back -- except that many independent windows are solved per call.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import capi
from .window import Window


def _arr(a, dtype, cols=None):
    """None stays None; anything else becomes a contiguous array of dtype, flat or with `cols` columns."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype)
    return a.reshape(-1) if cols is None else a.reshape(-1, cols)


_ptr = capi._p   # None (and an empty array) -> NULL


def _out(n, *shape, dtype=float, want=True):
    """The output array of n records, never empty (the entries take no NULL for a required output); want=False: None."""
    return np.zeros((max(n, 1),) + shape, dtype) if want else None


def _cut(a, n):
    return a[:n].copy() if a is not None else None


def _row_model(rm):
    """(fy, cy, rows, iterations) or capi.RowModel or None -> the pointer argument."""
    if rm is None:
        return None
    return C.byref(rm if isinstance(rm, capi.RowModel) else capi.RowModel(float(rm[0]), float(rm[1]), int(rm[2]), int(rm[3])))


def _gate_options(lib, min_redundancy):
    o = capi.GateOptions()
    lib.ctvio_default_gate_options(C.byref(o))
    if min_redundancy is not None:
        o.min_redundancy = float(min_redundancy)
    return o


def _imu_samples(imu_t, gyro, acc):
    t, g, a = _arr(imu_t, np.int64), _arr(gyro, np.float64, 3), _arr(acc, np.float64, 3)
    assert g.shape[0] == t.shape[0] and a.shape[0] == t.shape[0]
    return t, g, a


class Solver:
    """One handle = one HIP stream + the HBM buffers of a batch of windows."""

    def __init__(self, device: int = 0, precision: str = "fp64", use_mfma: bool = True, check_every: int = 4,
                 deterministic: int = -1, host_threads: int = 0, use_graph: bool = True, line_search: bool = True,
                 **tolerances):
        """All-fp64, like the reference (`precision` is kept for call compatibility: only "fp64" exists).  deterministic: 1 = order-fixed
        accumulation (bitwise reproducible) for batches whose every window has K <= 25 (others are refused), 2 = order-fixed accumulation
        for every batch the solver accepts (windows up to P = 1024; the K <= 25 windows run exactly as under 1), 0 = off, -1 = on for batches
        of <= 64 windows where 1 applies."""
        if precision not in ("fp64", capi.FP64):
            raise ValueError("only precision='fp64' exists (the mixed fp32 mode was removed: it missed the 1e-4 contract)")
        self._lib = capi.load_library()
        if self._lib.ctvio_device_count() <= 0:
            raise capi.CtvioError("no HIP device: ctrl-vio_amd has no CPU fallback")
        opt = capi.Options()
        self._lib.ctvio_default_options(C.byref(opt))
        opt.device = device
        opt.precision = capi.FP64
        opt.use_mfma = int(use_mfma)   # 0 / 1 / 2 (include/ctvio.h)
        opt.check_every = int(check_every)
        opt.deterministic = int(deterministic)
        opt.host_threads = int(host_threads)
        opt.use_graph = int(bool(use_graph))
        opt.line_search = int(bool(line_search))
        for k, v in tolerances.items():
            if not hasattr(opt, k):
                raise TypeError(f"unknown option {k}")
            setattr(opt, k, v)
        self._h = C.c_void_p()
        capi.check(self._lib.ctvio_create(C.byref(opt), C.byref(self._h)))
        self.windows: list[Window] = []

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ctvio_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- batch construction
    def clear(self):
        capi.check(self._lib.ctvio_clear(self._h))
        self.windows = []

    def add_window(self, w: Window) -> int:
        keep = []
        cw = capi.to_cwindow(w, keep)
        wid = C.c_int32(-1)
        capi.check(self._lib.ctvio_add_window(self._h, C.byref(cw), C.byref(wid)))
        self.windows.append(w)
        return wid.value

    def upload(self):
        capi.check(self._lib.ctvio_upload(self._h))

    def set_windows(self, windows):
        """ctvio_set_batch: validate + pack (C++ host threads) + one H2D copy of the whole batch."""
        windows = list(windows)
        keep = []
        arr = (capi.CWindow * len(windows))()
        for i, w in enumerate(windows):
            arr[i] = capi.to_cwindow(w, keep)
        capi.check(self._lib.ctvio_set_batch(self._h, len(windows), C.cast(arr, C.c_void_p)))
        self.windows = windows

    def set_cbatch(self, arr, n, windows=None):
        """Same from a prebuilt (CWindow * n) array (bench.py keeps the ctypes marshalling out of the timed region)."""
        capi.check(self._lib.ctvio_set_batch(self._h, int(n), C.cast(arr, C.c_void_p)))
        self.windows = list(windows) if windows is not None else []

    def get_batch_state(self):
        """Every window's state with one D2H copy: (quat (sumK,4), pos (sumK,3), bias (sumF,6), rho (sumL,), ld (n,))."""
        K = sum(w.K for w in self.windows); F = sum(w.F for w in self.windows); L = sum(w.L for w in self.windows); n = len(self.windows)
        q = np.zeros((K, 4)); p = np.zeros((K, 3)); b = np.zeros((F, 6)); r = np.zeros(max(L, 1)); ld = np.zeros(n)
        capi.check(self._lib.ctvio_get_batch_state(self._h, capi._p(q), capi._p(p), capi._p(b), capi._p(r), capi._p(ld)))
        return q, p, b, r[:L], ld

    def writeback_all(self):
        """get_batch_state scattered into the Window objects of the batch (in place, like Ceres updates its double*)."""
        q, p, b, r, ld = self.get_batch_state()
        k = f = l = 0
        for i, w in enumerate(self.windows):
            w.quat[:] = q[k:k + w.K]; w.pos[:] = p[k:k + w.K]; w.bias[:] = b[f:f + w.F]; w.rho[:] = r[l:l + w.L]; w.ld = float(ld[i])
            k += w.K; f += w.F; l += w.L

    @property
    def n(self) -> int:
        return int(self._lib.ctvio_num_windows(self._h))

    # ---- solve
    def solve(self, max_iterations: int = 15, writeback: bool = True):
        """Solve every window of the batch; returns list of summary dicts.  With writeback the
        Window objects passed to add_window are updated in place (Ceres updates double* in place)."""
        n = self.n
        sm = (capi.Summary * n)()
        capi.check(self._lib.ctvio_solve(self._h, int(max_iterations), C.cast(sm, C.c_void_p)))
        if writeback:
            self.writeback_all()
        return [s.as_dict() for s in sm]

    # ---- IMU-only predict (reference TrajectoryManager::InitTrajectory, src/estimator/trajectory_manager.cpp:288-315)
    @staticmethod
    def predict_window(w: Window, fixed_upto: int = -1) -> Window:
        """The factor set of InitTrajectory for window w: IMU blocks only (no visual blocks, bias chain or prior), both biases
        locked (option.lock_ab / lock_wb), knots 0..fixed_upto constant.  NB: the reference calls SetFixedIndex(max_bef_idx)
        AFTER its AddIMUMeasurementAnalytic loop, and constancy is decided when a knot is added
        (trajectory_estimator.cpp:134-138), so in the reference as written no knot is constant: pass fixed_upto = -1 for
        that behaviour, max_bef_idx for what the call order suggests was intended.  The per-block Cauchy widths go with the visual
        blocks; per-knot constancy (knot_const) is a property of the caller's window and is KEPT: a knot the caller holds constant
        stays constant in the predict as well."""
        p = w.copy()
        p.v_cauchy = None
        z = lambda a: a[:0]
        p.v_lm, p.v_ti, p.v_tj, p.v_rowi, p.v_rowj, p.v_pi, p.v_pj = z(p.v_lm), z(p.v_ti), z(p.v_tj), z(p.v_rowi), z(p.v_rowj), z(p.v_pi), z(p.v_pj)
        p.bc_i, p.bc_j, p.bc_w = z(p.bc_i), z(p.bc_j), z(p.bc_w)
        p.pJ0 = np.zeros((0, 0)); p.pr0 = np.zeros(0)
        p.p_kind, p.p_index, p.p_off, p.p_x0 = z(p.p_kind), z(p.p_index), z(p.p_off), z(p.p_x0)
        p.lock_bg = p.lock_ba = True
        p.fixed_upto = int(fixed_upto)
        return p.normalize()

    def predict(self, windows, fixed_upto=None, max_iterations: int = 8):
        """InitTrajectory for a batch: Solve(8) of the IMU-only problems; the knots of `windows` are updated in place."""
        fixed_upto = [-1] * len(windows) if fixed_upto is None else list(fixed_upto)
        pw = [self.predict_window(w, f) for w, f in zip(windows, fixed_upto)]
        self.set_windows(pw)
        sms = self.solve(max_iterations)
        for w, p in zip(windows, pw):
            w.quat[:] = p.quat; w.pos[:] = p.pos
        return sms

    def solve_raw(self, max_iterations: int = 15):
        """Solve without any host-side copy besides the summaries (used by bench.py)."""
        capi.check(self._lib.ctvio_solve(self._h, int(max_iterations), None))

    def get_state(self, wid: int, into: Window | None = None) -> Window:
        w = into if into is not None else self.windows[wid].copy()
        ld = C.c_double()
        capi.check(self._lib.ctvio_get_state(self._h, wid, capi._p(w.quat), capi._p(w.pos), capi._p(w.bias), capi._p(w.rho),
                                             C.cast(C.byref(ld), C.c_void_p)))
        w.ld = float(ld.value)
        return w

    def set_state(self, wid: int, w: Window):
        w.normalize()
        capi.check(self._lib.ctvio_set_state(self._h, wid, capi._p(w.quat), capi._p(w.pos), capi._p(w.bias), capi._p(w.rho), float(w.ld)))

    def snapshot_state(self):
        capi.check(self._lib.ctvio_snapshot_state(self._h))

    def restore_state(self):
        capi.check(self._lib.ctvio_restore_state(self._h))

    # ---- diagnostics
    def linearize(self, wid: int):
        w = self.windows[wid]
        P, L, N = w.P, w.L, w.N
        H = np.zeros((P, P)); W = np.zeros((P, max(L, 1))); Hll = np.zeros(max(L, 1)); g = np.zeros(N); cost = C.c_double()
        capi.check(self._lib.ctvio_linearize(self._h, wid, capi._p(H), capi._p(W), capi._p(Hll), capi._p(g),
                                             C.cast(C.byref(cost), C.c_void_p)))
        return H, W[:, :L], Hll[:L], g, float(cost.value)

    def cost(self, wid: int) -> float:
        c = C.c_double()
        capi.check(self._lib.ctvio_cost(self._h, wid, C.cast(C.byref(c), C.c_void_p)))
        return float(c.value)

    def lm_step(self, wid: int, mu: float = 1e4):
        w = self.windows[wid]
        d = np.zeros(w.N); mc = C.c_double()
        capi.check(self._lib.ctvio_lm_step(self._h, wid, float(mu), capi._p(d), C.cast(C.byref(mc), C.c_void_p)))
        return d, float(mc.value)

    def residual_summary(self, wid: int):
        """ResidualSummary of window wid at its current state: dict type -> (sum |r_i| per component, block count)."""
        w = self.windows[wid]
        sums = np.zeros(14 + w.pn); cnt = np.zeros(4, np.int32)
        capi.check(self._lib.ctvio_residual_summary(self._h, wid, capi._p(sums), capi._p(cnt)))
        return {"imu": (sums[:6].copy(), int(cnt[0])), "bias": (sums[6:12].copy(), int(cnt[1])), "image": (sums[12:14].copy(), int(cnt[2])),
                "prior": (sums[14:].copy(), int(cnt[3]))}

    def marginalize(self, wid: int, role, eps: float = 1e-8):
        """Prior construction from window `wid` (ctvio_marginalize): role[N] 1 = marginalise, 0 = keep, -1 = not involved.
        Returns (kept indices, J0 (n, n), r0 (n))."""
        N = self.windows[wid].N
        role = np.ascontiguousarray(role, np.int8)
        assert role.shape == (N,)
        kept = np.zeros(N, np.int32); J0 = np.zeros(N * N); r0 = np.zeros(N); n = C.c_int32(0)
        capi.check(self._lib.ctvio_marginalize(self._h, wid, capi._p(role), float(eps), C.byref(n), capi._p(kept), capi._p(J0), capi._p(r0)))
        n = n.value
        return kept[:n].copy(), J0[: n * n].reshape(n, n).copy(), r0[:n].copy()

    def marginalize_ran_on_host(self) -> bool:
        """Whether the last marginalize / marginalize_batch call factored on the host cores (ctvio_marginalize_ran_on_host)."""
        return bool(self._lib.ctvio_marginalize_ran_on_host(self._h))

    def marginalize_batch(self, roles, eps: float = 1e-8):
        """ctvio_marginalize_batch: roles = list of per-window role arrays.  Returns a list of (kept, J0, r0) per window."""
        Ns = [w.N for w in self.windows]
        role = np.ascontiguousarray(np.concatenate([np.asarray(r, np.int8) for r in roles]), np.int8)
        assert role.shape[0] == sum(Ns)
        nk = np.zeros(len(Ns), np.int32); kept = np.zeros(sum(Ns), np.int32)
        nkeep = [int((np.asarray(r) == 0).sum()) for r in roles]
        J0 = np.zeros(max(sum(k * k for k in nkeep), 1)); r0 = np.zeros(max(sum(nkeep), 1))
        capi.check(self._lib.ctvio_marginalize_batch(self._h, capi._p(role), float(eps), capi._p(nk), capi._p(kept), capi._p(J0), capi._p(r0)))
        out, u, oj, orr = [], 0, 0, 0
        for N, n in zip(Ns, nk):
            n = int(n)
            out.append((kept[u:u + n].copy(), J0[oj:oj + n * n].reshape(n, n).copy(), r0[orr:orr + n].copy()))
            u += N; oj += n * n; orr += n
        return out

    def covariance_batch(self, sels, rho: bool = False):
        """ctvio_covariance_batch: marginal covariances of every window at its current state.  sels = one index list per window
        (trajectory unknowns in [0, P), at most 64, may be empty).  Returns (list of n x n arrays in the order of each selection,
        list of per-landmark inverse-depth variances or None, singular flags (n windows))."""
        assert len(sels) == len(self.windows)
        sels = [_arr(s, np.int32) for s in sels]
        ns = np.array([s.shape[0] for s in sels], np.int32)
        sel = _arr(np.concatenate(sels) if len(sels) else np.zeros(0, np.int32), np.int32)
        cov = _out(int((ns.astype(np.int64) ** 2).sum()))
        Ls = [w.L for w in self.windows]
        var = _out(sum(Ls), want=rho)
        sing = np.zeros(len(sels), np.int32)
        capi.check(self._lib.ctvio_covariance_batch(self._h, _ptr(ns), _ptr(sel), _ptr(cov), _ptr(var), _ptr(sing)))
        covs, vars_, oc, ov = [], [], 0, 0
        for n, L in zip(ns, Ls):
            n = int(n)
            covs.append(cov[oc:oc + n * n].reshape(n, n).copy()); oc += n * n
            if rho:
                vars_.append(var[ov:ov + L].copy()); ov += L
        return covs, (vars_ if rho else None), sing

    def covariance(self, wid: int, sel, rho: bool = False):
        """ctvio_covariance: the same for window wid alone (same bits as the batch entry).  Returns (n x n array, inverse-depth
        variances (L,) or None, singular flag)."""
        sel = _arr(sel, np.int32)
        n, L = int(sel.shape[0]), self.windows[wid].L
        cov = _out(n * n); var = _out(L, want=rho); sing = np.zeros(1, np.int32)
        capi.check(self._lib.ctvio_covariance(self._h, int(wid), n, _ptr(sel), _ptr(cov), _ptr(var), _ptr(sing)))
        return cov[:n * n].reshape(n, n).copy(), _cut(var, L), int(sing[0])

    @staticmethod
    def _extrinsic(q_SI, p_SI):
        if (q_SI is None) != (p_SI is None):
            raise ValueError("q_SI and p_SI come together (both None: the body pose)")
        if q_SI is None:
            return None, None
        return np.ascontiguousarray(q_SI, np.float64).reshape(4), np.ascontiguousarray(p_SI, np.float64).reshape(3)

    def pose_covariance_batch(self, win, t_ns, q_SI=None, p_SI=None):
        """ctvio_pose_covariance_batch: the 6 x 6 covariance of the pose at absolute time t_ns[i] of window win[i], at the current state, in the
        tangent (theta, p) of R(t) <- R(t) exp(dtheta), p(t) <- p(t) + dp.  q_SI = (x,y,z,w), p_SI: a sensor extrinsic (None: the body pose).
        Returns (cov (n, 6, 6), status (n,)): 0 ok, 1 singular window (NaN), 2 an untouched knot (+inf diagonal), 3 time outside the spline (NaN)."""
        wi = _arr(win, np.int32); t = _arr(t_ns, np.int64)
        n = int(t.shape[0])
        assert wi.shape[0] == n
        q, p = self._extrinsic(q_SI, p_SI)
        cov = _out(n, 6, 6); st = _out(n, dtype=np.int32)
        capi.check(self._lib.ctvio_pose_covariance_batch(self._h, C.c_int64(n), _ptr(wi), _ptr(t), _ptr(q), _ptr(p), _ptr(cov), _ptr(st)))
        return _cut(cov, n), _cut(st, n)

    def pose_covariance(self, wid: int, t_ns, q_SI=None, p_SI=None):
        """ctvio_pose_covariance: the same for the times t_ns of window wid alone (same bits as the batch entry)."""
        t = _arr(t_ns, np.int64)
        n = int(t.shape[0])
        q, p = self._extrinsic(q_SI, p_SI)
        cov = _out(n, 6, 6); st = _out(n, dtype=np.int32)
        capi.check(self._lib.ctvio_pose_covariance(self._h, int(wid), n, _ptr(t), _ptr(q), _ptr(p), _ptr(cov), _ptr(st)))
        return _cut(cov, n), _cut(st, n)

    def _landmark_points(self, call, L, cov):
        pts = _out(L, 3); c9 = _out(L, 3, 3, want=cov); st = _out(L, dtype=np.int32)
        capi.check(call(_ptr(pts), _ptr(c9), _ptr(st)))
        return _cut(pts, L), _cut(c9, L), _cut(st, L)

    def landmark_points_batch(self, cov: bool = True):
        """ctvio_landmark_points_batch: the world point X = R_C (p_i / rho) + p_C of every landmark of the batch at the current state (camera
        pose at the anchor's row time) and, with cov, its 3 x 3 covariance (trajectory, inverse depth and their cross terms).  Returns (points
        (sum L, 3), cov (sum L, 3, 3) or None, status (sum L,)) in window order, the caller's landmark order: 0 ok, 1 singular window (cov NaN),
        2 no information on the inverse depth (+inf diagonal), 3 not computable (NaN).  cov=False: one kernel, nothing is linearised."""
        return self._landmark_points(lambda p, c, s: self._lib.ctvio_landmark_points_batch(self._h, p, c, s), sum(w.L for w in self.windows), cov)

    def landmark_points(self, wid: int, cov: bool = True):
        """ctvio_landmark_points: the same for window wid alone (same bits as the batch entry).  Returns (points (L, 3), cov (L, 3, 3) or None,
        status (L,))."""
        if not 0 <= int(wid) < len(self.windows):
            capi.check(self._lib.ctvio_landmark_points(self._h, int(wid), None, None, None))
        return self._landmark_points(lambda p, c, s: self._lib.ctvio_landmark_points(self._h, int(wid), p, c, s), self.windows[int(wid)].L, cov)

    def _nav_state(self, call, t_ns, frame, cov, n_win=None):
        t = _arr(t_ns, np.int64); fr = _arr(frame, np.int32)
        n = int(t.shape[0])
        assert (fr is None or fr.shape[0] == n) and (n_win is None or n_win == n)
        state = _out(n, 16); c = _out(n, 15, 15, want=cov); st = _out(n, dtype=np.int32)
        capi.check(call(n, _ptr(t), _ptr(fr), _ptr(state), _ptr(c), _ptr(st)))
        return _cut(state, n), _cut(c, n), _cut(st, n)

    def nav_state_batch(self, win, t_ns, frame=None, cov: bool = True):
        """ctvio_nav_state_batch: the navigation state (px, py, pz, qx, qy, qz, qw, world velocity, bg, ba of bias state frame[i]; frame None:
        the newest frame) at absolute time t_ns[i] of window win[i], at the current state, and with cov its 15 x 15 covariance in the tangent
        (dtheta, dp, dv, dbg, dba) of R(t) <- R(t) exp(dtheta), the rest additive.  Returns (state (n, 16), cov (n, 15, 15) or None, status
        (n,)): 0 ok, 1 singular window (cov NaN), 2 an untouched knot or bias state (+inf diagonal), 3 time outside the spline (NaN).
        cov=False: one kernel, nothing is linearised."""
        wi = _arr(win, np.int32)
        return self._nav_state(lambda n, t, f, s, c, st: self._lib.ctvio_nav_state_batch(self._h, C.c_int64(n), _ptr(wi), t, f, s, c, st), t_ns,
                               frame, cov, int(wi.shape[0]))

    def nav_state(self, wid: int, t_ns, frame=None, cov: bool = True):
        """ctvio_nav_state: the same for the times t_ns of window wid alone (same bits as the batch entry)."""
        return self._nav_state(lambda n, t, f, s, c, st: self._lib.ctvio_nav_state(self._h, int(wid), n, t, f, s, c, st), t_ns, frame, cov)

    def _body_rates(self, call, t_ns, frame, meas, noise, cov, n_win=None):
        t = _arr(t_ns, np.int64); fr = _arr(frame, np.int32); z = _arr(meas, np.float64, 6)
        n = int(t.shape[0])
        sg = None if noise is None else _arr(noise, np.float64).reshape(6)
        assert (fr is None or fr.shape[0] == n) and (z is None or z.shape[0] == n) and (n_win is None or n_win == n)
        if z is not None and not cov:
            raise ValueError("meas needs cov=True: the gate is formed from the covariance")
        rates = _out(n, 9); c = _out(n, 15, 15, want=cov); chi = _out(n, want=z is not None); st = _out(n, dtype=np.int32)
        capi.check(call(n, _ptr(t), _ptr(fr), _ptr(z), _ptr(sg), _ptr(rates), _ptr(c), _ptr(chi), _ptr(st)))
        return _cut(rates, n), _cut(c, n), _cut(chi, n), _cut(st, n)

    def body_rates_batch(self, win, t_ns, frame=None, cov: bool = True, meas=None, noise=None):
        """ctvio_body_rates_batch: the body angular velocity, the specific force f = R(t)^T (p''(t) + g) and the body-frame velocity
        v_B = R(t)^T v_W(t) at absolute time t_ns[i] of window win[i], at the current state, and with cov their 15 x 15 covariance with the
        biases of state frame[i] (None: the newest) in the additive tangent (domega, df, dv_B, dbg, dba).  meas (n, 6): candidate IMU samples
        (gyro, then accelerometer) for the gate chi2 = e^T (A C A^T + diag(sigma^2))^-1 e, e = meas - (omega + bg, f + ba); noise: the six
        standard deviations (None: 1 / imu_w of the window).  Returns (rates (n, 9), cov (n, 15, 15) or None, chi2 (n,) or None, status
        (n,)): 0 ok, 1 singular window (cov, chi2 NaN), 2 an untouched knot or bias state (+inf diagonal, chi2 0), 3 time outside the spline
        (NaN).  cov=False: one kernel, nothing is linearised."""
        wi = _arr(win, np.int32)
        return self._body_rates(lambda n, *a: self._lib.ctvio_body_rates_batch(self._h, C.c_int64(n), _ptr(wi), *a), t_ns, frame, meas, noise,
                                cov, int(wi.shape[0]))

    def body_rates(self, wid: int, t_ns, frame=None, cov: bool = True, meas=None, noise=None):
        """ctvio_body_rates: the same for the times t_ns of window wid alone (same bits as the batch entry)."""
        return self._body_rates(lambda n, *a: self._lib.ctvio_body_rates(self._h, int(wid), n, *a), t_ns, frame, meas, noise, cov)

    def _relative_pose(self, call, t_a, t_b, q_SI, p_SI, cov, n_win=None):
        ta = _arr(t_a, np.int64); tb = _arr(t_b, np.int64)
        n = int(ta.shape[0])
        assert tb.shape[0] == n and (n_win is None or n_win == n)
        q, p = self._extrinsic(q_SI, p_SI)
        rel = _out(n, 7); c = _out(n, 6, 6, want=cov); st = _out(n, dtype=np.int32)
        capi.check(call(n, _ptr(ta), _ptr(tb), _ptr(q), _ptr(p), _ptr(rel), _ptr(c), _ptr(st)))
        return _cut(rel, n), _cut(c, n), _cut(st, n)

    def relative_pose_batch(self, win, t_a, t_b, q_SI=None, p_SI=None, cov: bool = True):
        """ctvio_relative_pose_batch: the pose increment T(t_a[i])^-1 T(t_b[i]) of window win[i] at the current state, as (p_ab, q_ab as
        x, y, z, w), and with cov its 6 x 6 covariance in the tangent (dtheta, dp) of R_ab <- R_ab exp(dtheta), p_ab <- p_ab + dp (dp in frame
        a).  q_SI = (x,y,z,w), p_SI: a sensor extrinsic (None: body poses).  Returns (rel7 (n, 7), cov (n, 6, 6) or None, status (n,)): 0 ok,
        1 singular window (cov NaN), 2 an untouched knot (+inf diagonal), 3 a time outside the spline (NaN).  cov=False: one kernel, nothing
        is linearised."""
        wi = _arr(win, np.int32)
        return self._relative_pose(lambda n, ta, tb, q, p, r, c, st: self._lib.ctvio_relative_pose_batch(self._h, C.c_int64(n), _ptr(wi), ta, tb, q, p, r, c, st),
                                   t_a, t_b, q_SI, p_SI, cov, int(wi.shape[0]))

    def relative_pose(self, wid: int, t_a, t_b, q_SI=None, p_SI=None, cov: bool = True):
        """ctvio_relative_pose: the same for the pairs of times of window wid alone (same bits as the batch entry)."""
        return self._relative_pose(lambda n, ta, tb, q, p, r, c, st: self._lib.ctvio_relative_pose(self._h, int(wid), n, ta, tb, q, p, r, c, st),
                                   t_a, t_b, q_SI, p_SI, cov)

    def _project_landmarks(self, call, lm, t_ns, row, row_model, obs, cov, n_win=None):
        li = _arr(lm, np.int32); t = _arr(t_ns, np.int64); r = _arr(row, np.int32); o = _arr(obs, np.float64, 2)
        n = int(li.shape[0])
        assert t.shape[0] == n and r.shape[0] == n and (o is None or o.shape[0] == n) and (n_win is None or n_win == n)
        if o is not None and not cov:
            raise ValueError("obs needs cov=True: the gate is formed from the covariance")
        proj = _out(n, 3); c = _out(n, 2, 2, want=cov); chi = _out(n, want=o is not None)
        ro = _out(n, dtype=np.int32); st = _out(n, dtype=np.int32)
        capi.check(call(n, _ptr(li), _ptr(t), _ptr(r), _row_model(row_model), _ptr(o), _ptr(proj), _ptr(c), _ptr(chi), _ptr(ro), _ptr(st)))
        return SimpleNamespace(proj=_cut(proj, n), cov=_cut(c, n), chi2=_cut(chi, n), row=_cut(ro, n), status=_cut(st, n))

    def project_landmarks_batch(self, win, lm, t_ns, row, cov: bool = True, obs=None, row_model=None):
        """ctvio_project_landmarks_batch: where landmark lm[i] of window win[i] falls in the camera at frame time t_ns[i], image row row[i], at the
        current state: proj (n, 3) = the normalised image point and the depth in the query camera; with cov the 2 x 2 covariance of the point
        (trajectory, inverse depth and their cross terms); with obs (n, 2) the gate chi2 = e^T (Cov + I / img_w^2)^-1 e of the candidate points.
        row_model = (fy, cy, rows, iterations) or capi.RowModel: row[i] is the first guess of a pinhole row iteration, the final row comes
        back in .row.  Returns a namespace (proj, cov or None, chi2 or None, row, status): 0 ok, 1 singular window (cov, chi2 NaN), 2 no
        information (+inf diagonal, chi2 0), 3 not computable (NaN, row -1).  cov=False: one kernel, nothing is linearised."""
        wi = _arr(win, np.int32)
        return self._project_landmarks(lambda n, *a: self._lib.ctvio_project_landmarks_batch(self._h, C.c_int64(n), _ptr(wi), *a),
                                       lm, t_ns, row, row_model, obs, cov, int(wi.shape[0]))

    def project_landmarks(self, wid: int, lm, t_ns, row, cov: bool = True, obs=None, row_model=None):
        """ctvio_project_landmarks: the same for queries of window wid alone (same bits as the batch entry)."""
        return self._project_landmarks(lambda n, *a: self._lib.ctvio_project_landmarks(self._h, int(wid), n, *a), lm, t_ns, row, row_model, obs, cov)

    def _visual_gate(self, call, wids, cov, min_redundancy):
        o = _gate_options(self._lib, min_redundancy)
        V = sum(int(self.windows[w].V) for w in wids); L = sum(int(self.windows[w].L) for w in wids)
        res = _out(V, 2); wgt = _out(V); dep = _out(V); st = _out(V, dtype=np.int32); cnt = _out(L, dtype=np.int32)
        red = _out(V, want=cov); c = _out(V, 2, 2, want=cov); chi = _out(V, want=cov); lms = _out(L, 3, want=cov)
        capi.check(call(C.byref(o), _ptr(res), _ptr(wgt), _ptr(dep), _ptr(red), _ptr(c), _ptr(chi), _ptr(st), _ptr(lms), _ptr(cnt)))
        return SimpleNamespace(res=_cut(res, V), weight=_cut(wgt, V), depth=_cut(dep, V), redundancy=_cut(red, V), cov=_cut(c, V), chi2=_cut(chi, V),
                               status=_cut(st, V), lm_stats=_cut(lms, L), lm_count=_cut(cnt, L))

    def visual_gate_batch(self, cov: bool = True, min_redundancy=None):
        """ctvio_visual_gate_batch: the leave-one-out test of every visual block of the uploaded windows at the current state, window after
        window in the caller's block order.  Returns a namespace: res (V, 2) the whitened residual before the loss, weight the loss weight
        rho', depth, redundancy = lambda_min(I - A), cov (V, 2, 2) the whitened leave-one-out prediction covariance, chi2 = r^T (cov + I)^-1 r
        (2 degrees of freedom), status (0 ok, 1 singular window, 2 no information, 3 not computable, 4 redundancy < min_redundancy),
        lm_stats (L, 3) = (mean |proj - p_j|, largest chi2, smallest redundancy) and lm_count per landmark.  cov=False: values only
        (redundancy, cov, chi2 and lm_stats None), nothing is linearised or factored."""
        return self._visual_gate(lambda *a: self._lib.ctvio_visual_gate_batch(self._h, *a), range(len(self.windows)), cov, min_redundancy)

    def visual_gate(self, wid: int, cov: bool = True, min_redundancy=None):
        """ctvio_visual_gate: the same for window wid alone (same bits as the batch entry)."""
        return self._visual_gate(lambda *a: self._lib.ctvio_visual_gate(self._h, int(wid), *a), [int(wid)], cov, min_redundancy)

    def _block_count(self, wid):
        return sum(int(w.V) for w in self.windows) if wid is None else int(self.windows[int(wid)].V)

    def set_visual_active(self, active, wid=None):
        """ctvio_set_visual_active(_batch): switch visual blocks on (non-zero) and off (0), one entry per block in the caller's block order --
        of window wid, or of every window one after the other.  None: every block active.  An inactive block is not a factor of the window;
        the slot order, the sparsity plan and the captured graph stay the upload's."""
        a = None if active is None else np.ascontiguousarray(np.asarray(active) != 0, dtype=np.uint8)
        if a is not None and a.shape != (self._block_count(wid),):
            raise ValueError("active: one entry per visual block")
        if wid is None:
            capi.check(self._lib.ctvio_set_visual_active_batch(self._h, _ptr(a) if a is not None else None))
        else:
            capi.check(self._lib.ctvio_set_visual_active(self._h, int(wid), _ptr(a) if a is not None else None))

    def visual_active(self, wid=None):
        """ctvio_get_visual_active(_batch): the flags as a uint8 array (1 active, 0 inactive), the caller's block order."""
        a = np.zeros(max(self._block_count(wid), 1), dtype=np.uint8)
        if wid is None:
            capi.check(self._lib.ctvio_get_visual_active_batch(self._h, _ptr(a)))
        else:
            capi.check(self._lib.ctvio_get_visual_active(self._h, int(wid), _ptr(a)))
        return a[:self._block_count(wid)]

    def cull_visual(self, wid=None, **options):
        """ctvio_cull_visual(_batch): gate, decision and flag update on the device at the current state.  options: the fields of
        ctvio_cull_options (min_redundancy, chi2_max, mean_error_max, worst_only, drop_uncomputable) over its defaults.  Returns a namespace:
        n_culled (blocks switched off by this call, per window) and active (the flags after the call)."""
        o = capi.CullOptions()
        self._lib.ctvio_default_cull_options(C.byref(o))
        for k, v in options.items():
            if k not in dict(capi.CullOptions._fields_):
                raise TypeError(f"unknown cull option {k!r}")
            setattr(o, k, v)
        nw = len(self.windows) if wid is None else 1
        nc = np.zeros(nw, dtype=np.int32); a = np.zeros(max(self._block_count(wid), 1), dtype=np.uint8)
        if wid is None:
            capi.check(self._lib.ctvio_cull_visual_batch(self._h, C.byref(o), _ptr(nc), _ptr(a)))
        else:
            capi.check(self._lib.ctvio_cull_visual(self._h, int(wid), C.byref(o), _ptr(nc), _ptr(a)))
        return SimpleNamespace(n_culled=nc, active=a[:self._block_count(wid)])

    def _imu_gate(self, call, wids, cov, min_redundancy):
        o = _gate_options(self._lib, min_redundancy)
        M = sum(int(self.windows[w].M) for w in wids); F = sum(int(self.windows[w].F) for w in wids)
        res = _out(M, 6); st = _out(M, dtype=np.int32)
        red = _out(M, want=cov); c = _out(M, 6, 6, want=cov); chi = _out(M, want=cov); fs = _out(F, 4, want=cov)
        capi.check(call(C.byref(o), _ptr(res), _ptr(red), _ptr(c), _ptr(chi), _ptr(st), _ptr(fs)))
        return SimpleNamespace(res=_cut(res, M), redundancy=_cut(red, M), cov=_cut(c, M), chi2=_cut(chi, M), status=_cut(st, M), frame_stats=_cut(fs, F))

    def imu_gate_batch(self, cov: bool = True, min_redundancy=None):
        """ctvio_imu_gate_batch: the leave-one-out test of every IMU sample of the uploaded windows at the current state, window after window
        in the caller's sample order.  Returns a namespace: res (M, 6) the whitened residual, redundancy = lambda_min(I - A), cov (M, 6, 6) the
        whitened leave-one-out prediction covariance (I - A)^-1 - I, chi2 = r^T (I - A)^-1 r (6 degrees of freedom), status (0 ok, 1 singular
        window, 2 no information, 4 redundancy < min_redundancy) and frame_stats (F, 4) = (status-0 samples, their mean chi2, largest chi2,
        smallest redundancy) per bias state.  cov=False: values only (redundancy, cov, chi2 and frame_stats None), nothing is linearised or
        factored."""
        return self._imu_gate(lambda *a: self._lib.ctvio_imu_gate_batch(self._h, *a), range(len(self.windows)), cov, min_redundancy)

    def imu_gate(self, wid: int, cov: bool = True, min_redundancy=None):
        """ctvio_imu_gate: the same for window wid alone (same bits as the batch entry)."""
        return self._imu_gate(lambda *a: self._lib.ctvio_imu_gate(self._h, int(wid), *a), [int(wid)], cov, min_redundancy)

    def _imu_noise(self, noise):
        o = capi.ImuNoise()
        self._lib.ctvio_default_imu_noise(C.byref(o))
        if noise is None:
            return o
        if isinstance(noise, dict):
            for k, v in noise.items():
                if not hasattr(o, k):
                    raise KeyError(k)
                setattr(o, k, float(v))
            return o
        o.gyr_n, o.acc_n, o.gyr_w, o.acc_w = (float(x) for x in noise)
        return o

    def _imu_predict(self, call, m, imu_t, gyro, acc, noise, last_only, cov):
        """m: samples per query (n,); the concatenated samples.  Returns (state (E, 16), cov (E, 15, 15) or None, status (n,)), E = sum m, or n
        with last_only."""
        t, g, a = _imu_samples(imu_t, gyro, acc)
        n = int(m.shape[0])
        ns = int(t.shape[0])
        assert n == 0 or int(np.clip(m, 0, None).sum()) <= ns
        ne = n if last_only else ns
        state = _out(ne, 16); c = _out(ne, 15, 15, want=cov); st = _out(n, dtype=np.int32)
        capi.check(call(_ptr(t), _ptr(g), _ptr(a), C.byref(self._imu_noise(noise)), 1 if last_only else 0, _ptr(state), _ptr(c), _ptr(st)))
        return _cut(state, ne), _cut(c, ne), _cut(st, n)

    def imu_predict_batch(self, win, frame, n_imu, imu_t, gyro, acc, noise=None, last_only: bool = False, cov: bool = True):
        """ctvio_imu_predict_batch: IMU dead reckoning (midpoint rule) from the navigation state of window win[i] at the first of its n_imu[i]
        samples, with bias state frame[i] (frame None: the newest), through the samples -- concatenated in query order: absolute times imu_t
        (ns), gyro and acc (.., 3) -- and with cov the 15 x 15 covariance P_j = F P F^T + G Q G^T in the tangent of nav_state.  noise: (gyr_n,
        acc_n, gyr_w, acc_w), a dict of some of them, or None for the reference's defaults.  Returns (state (E, 16), cov (E, 15, 15) or None,
        status (n,)): E = sum n_imu entries in query then sample order (sample 0 = nav_state's output), or, last_only, one per query: its last
        sample.  Statuses as nav_state's, per query."""
        wi = _arr(win, np.int32)
        m = _arr(n_imu, np.int32); fr = _arr(frame, np.int32)
        assert m.shape[0] == wi.shape[0] and (fr is None or fr.shape[0] == wi.shape[0])
        return self._imu_predict(lambda t, g, a, nz, lo, s, c, st: self._lib.ctvio_imu_predict_batch(
            self._h, C.c_int64(int(wi.shape[0])), _ptr(wi), _ptr(fr), _ptr(m), t, g, a, nz, lo, s, c, st), m, imu_t, gyro, acc, noise,
            last_only, cov)

    def imu_predict(self, wid: int, frame, imu_t, gyro, acc, noise=None, last_only: bool = False, cov: bool = True):
        """ctvio_imu_predict: one query of window wid (frame None or -1: the newest bias state) with len(imu_t) samples; the batch entry's bits."""
        m = np.array([np.asarray(imu_t).reshape(-1).shape[0]], np.int32)
        f = -1 if frame is None else int(frame)
        return self._imu_predict(lambda t, g, a, nz, lo, s, c, st: self._lib.ctvio_imu_predict(self._h, int(wid), f, int(m[0]), t, g, a, nz, lo, s, c, st),
                                 m, imu_t, gyro, acc, noise, last_only, cov)

    def _predict_landmarks(self, call, n_pred, imu_t, gyro, acc, noise, lm, row, row_model, obs, cov, n_pts_expected=None):
        t, g, a = _imu_samples(imu_t, gyro, acc)
        li = _arr(lm, np.int32); r = _arr(row, np.int32); o = _arr(obs, np.float64, 2)
        n = int(li.shape[0])
        assert r.shape[0] == n and (o is None or o.shape[0] == n)
        assert n_pts_expected is None or n_pts_expected == n
        if o is not None and not cov:
            raise ValueError("obs needs cov=True: the gate is formed from the covariance")
        state = _out(n_pred, 16); proj = _out(n, 3); c = _out(n, 2, 2, want=cov); chi = _out(n, want=o is not None)
        ro = _out(n, dtype=np.int32); st = _out(n, dtype=np.int32)
        capi.check(call(_ptr(t), _ptr(g), _ptr(a), C.byref(self._imu_noise(noise)), n, _ptr(li), _ptr(r), _row_model(row_model), _ptr(o),
                        _ptr(state), _ptr(proj), _ptr(c), _ptr(chi), _ptr(ro), _ptr(st)))
        return SimpleNamespace(state=_cut(state, n_pred), proj=_cut(proj, n), cov=_cut(c, n), chi2=_cut(chi, n), row=_cut(ro, n), status=_cut(st, n))

    def predict_landmarks_batch(self, win, frame, n_imu, imu_t, gyro, acc, pred, lm, row, noise=None, cov: bool = True, obs=None, row_model=None):
        """ctvio_predict_landmarks_batch: where landmarks fall in the camera at IMU-predicted poses BEYOND the spline.  Predictions are the queries
        of imu_predict_batch (win, frame or None, n_imu, the concatenated samples); point i = (prediction pred[i], landmark lm[i] of that
        prediction's window, image row row[i]).  Returns a namespace like project_landmarks' (proj (n, 3), cov (n, 2, 2) or None, chi2 or None,
        row, status) plus state (n_pred, 16): the end state of every prediction (imu_predict's with last_only).  The covariance carries the
        window's uncertainty through the propagation (cross terms with the landmark included) plus the IMU process noise.  cov=False: values
        only, nothing is linearised."""
        wi = _arr(win, np.int32)
        m = _arr(n_imu, np.int32); fr = _arr(frame, np.int32)
        pi = _arr(pred, np.int32)
        assert m.shape[0] == wi.shape[0] and (fr is None or fr.shape[0] == wi.shape[0])
        npred = int(wi.shape[0])
        return self._predict_landmarks(lambda t, g, a, nz, n, li, r, *rest: self._lib.ctvio_predict_landmarks_batch(
            self._h, C.c_int64(npred), _ptr(wi), _ptr(fr), _ptr(m), t, g, a, nz, C.c_int64(n), _ptr(pi), li, r, *rest),
            npred, imu_t, gyro, acc, noise, lm, row, row_model, obs, cov, int(pi.shape[0]))

    def predict_landmarks(self, wid: int, frame, imu_t, gyro, acc, lm, row, noise=None, cov: bool = True, obs=None, row_model=None):
        """ctvio_predict_landmarks: one prediction of window wid (frame None or -1: the newest bias state) with len(imu_t) samples and every
        point under it; the batch entry's bits."""
        m = int(np.asarray(imu_t).reshape(-1).shape[0])
        f = -1 if frame is None else int(frame)
        return self._predict_landmarks(lambda t, g, a, nz, n, li, r, *rest: self._lib.ctvio_predict_landmarks(
            self._h, int(wid), f, m, t, g, a, nz, n, li, r, *rest), 1, imu_t, gyro, acc, noise, lm, row, row_model, obs, cov)

    def _tri_options(self, opts):
        o = capi.TriangulateOptions()
        self._lib.ctvio_default_triangulate_options(C.byref(o))
        for k, v in opts.items():
            if k not in ("row_times", "only_unset", "apply", "min_depth", "init_depth"):
                raise TypeError(f"unknown triangulation option {k}")
            setattr(o, k, float(v) if k.endswith("depth") else int(v))
        return o

    def triangulate_batch(self, **opts):
        """ctvio_triangulate_batch: landmark depths of every window at the current device state (options: the fields of
        ctvio_triangulate_options; defaults row_times=1, only_unset=1, apply=1, min_depth=0.1, init_depth=5.0).  Returns (list of depth
        arrays, list of flag arrays), one per window, in the caller's landmark order."""
        o = self._tri_options(opts)
        Ls = [w.L for w in self.windows]
        depth = np.zeros(max(sum(Ls), 1)); flag = np.zeros(max(sum(Ls), 1), np.int32)
        capi.check(self._lib.ctvio_triangulate_batch(self._h, C.byref(o), capi._p(depth), capi._p(flag)))
        cut = np.cumsum([0] + Ls)
        return [depth[a:b].copy() for a, b in zip(cut[:-1], cut[1:])], [flag[a:b].copy() for a, b in zip(cut[:-1], cut[1:])]

    def triangulate(self, wid: int, **opts):
        """ctvio_triangulate: the same for window wid alone (same bits as the batch entry).  Returns (depth (L,), flag (L,))."""
        o = self._tri_options(opts)
        L = self.windows[wid].L
        depth = np.zeros(max(L, 1)); flag = np.zeros(max(L, 1), np.int32)
        capi.check(self._lib.ctvio_triangulate(self._h, int(wid), C.byref(o), capi._p(depth), capi._p(flag)))
        return depth[:L].copy(), flag[:L].copy()

    def shift_anchor(self, win, lm, t_new, row_new=None, **opts):
        """ctvio_shift_anchor_batch: the depth of landmark lm[i] of window win[i] in the frame of a new anchor observation at absolute time
        t_new[i], row row_new[i] (None: frame times, row_times=0).  Returns (depth_new (n,), flag (n,)); the state is not modified."""
        if row_new is None:
            opts.setdefault("row_times", 0)
        o = self._tri_options(opts)
        wi = np.ascontiguousarray(win, np.int32).reshape(-1); li = np.ascontiguousarray(lm, np.int32).reshape(-1)
        t = np.ascontiguousarray(t_new, np.int64).reshape(-1)
        r = np.ascontiguousarray(row_new, np.int32).reshape(-1) if row_new is not None else None
        n = int(wi.shape[0])
        assert li.shape[0] == n and t.shape[0] == n and (r is None or r.shape[0] == n)
        depth = np.zeros(max(n, 1)); flag = np.zeros(max(n, 1), np.int32)
        capi.check(self._lib.ctvio_shift_anchor_batch(self._h, C.byref(o), C.c_int64(n), capi._p(wi), capi._p(li), capi._p(t),
                                                      capi._p(r) if r is not None else None, capi._p(depth), capi._p(flag)))
        return depth[:n].copy(), flag[:n].copy()

    def gauge_restore(self, wids, knots, q0, t0):
        """4-DoF gauge restore (reference double2vector): windows `wids`, reference knot index per window, its pre-solve
        quaternion (n,4) (x,y,z,w) and position (n,3).  Acts on the device state; read it back with get_state."""
        ids = np.ascontiguousarray(wids, np.int32); kn = np.ascontiguousarray(knots, np.int32)
        q = np.ascontiguousarray(q0, np.float64).reshape(-1, 4); t = np.ascontiguousarray(t0, np.float64).reshape(-1, 3)
        assert ids.shape[0] == kn.shape[0] == q.shape[0] == t.shape[0]
        capi.check(self._lib.ctvio_gauge_restore(self._h, int(ids.shape[0]), capi._p(ids), capi._p(kn), capi._p(q), capi._p(t)))

    def spline_eval(self, wid: int, t_ns):
        t = np.ascontiguousarray(t_ns, np.int64)
        n = t.shape[0]
        pose = np.zeros((n, 7)); vel = np.zeros((n, 3)); om = np.zeros((n, 3)); acc = np.zeros((n, 3))
        capi.check(self._lib.ctvio_spline_eval(self._h, wid, n, capi._p(t), capi._p(pose), capi._p(vel), capi._p(om), capi._p(acc)))
        return pose, vel, om, acc

    def spline_eval_batch(self, win, t_ns, want=("pose", "vel", "omega")):
        """Queries of any windows of the batch in one launch (ctvio_spline_eval_batch): query i = (window win[i], absolute time
        t_ns[i]).  Returns (dict of the requested outputs, device milliseconds of the evaluation kernel alone)."""
        t = np.ascontiguousarray(t_ns, np.int64); wi = np.ascontiguousarray(win, np.int32)
        n = int(t.shape[0])
        out = {"pose": np.zeros((n, 7)) if "pose" in want else None, "vel": np.zeros((n, 3)) if "vel" in want else None,
               "omega": np.zeros((n, 3)) if "omega" in want else None, "acc": np.zeros((n, 3)) if "acc" in want else None}
        ms = C.c_double()
        ptr = lambda a: capi._p(a) if a is not None else None
        capi.check(self._lib.ctvio_spline_eval_batch(self._h, C.c_int64(n), capi._p(wi), capi._p(t), ptr(out["pose"]), ptr(out["vel"]),
                                                     ptr(out["omega"]), ptr(out["acc"]), C.cast(C.byref(ms), C.c_void_p)))
        return {k: v for k, v in out.items() if v is not None}, float(ms.value)

    def sensor_pose(self, wid: int, t_ns, q_SI, p_SI):
        """Trajectory::GetSensorPose (reference src/spline/trajectory.cpp:39-56): poseNs(t) * T_StoI, evaluated on the device.
        q_SI = (x,y,z,w).  Returns (n,7) = (p, q)."""
        t = np.ascontiguousarray(t_ns, np.int64)
        q = np.ascontiguousarray(q_SI, np.float64).reshape(4); p = np.ascontiguousarray(p_SI, np.float64).reshape(3)
        pose = np.zeros((t.shape[0], 7))
        capi.check(self._lib.ctvio_sensor_pose(self._h, wid, int(t.shape[0]), capi._p(t), capi._p(q), capi._p(p), capi._p(pose)))
        return pose

    PHASES = ("k_imu_linearize", "k_vis_eval", "k_assemble_vis", "assemble_rest", "k_schur_mfma", "k_cholesky_solve", "rest", "solve")

    def set_profiling(self, on: bool):
        capi.check(self._lib.ctvio_set_profiling(self._h, int(bool(on))))

    def last_timing(self):
        """(ms[8], launches[8]) of the last solve; see include/ctvio.h ctvio_last_timing."""
        ms = np.zeros(8); n = np.zeros(8, np.int32)
        capi.check(self._lib.ctvio_last_timing(self._h, capi._p(ms), capi._p(n)))
        return ms, n

    @property
    def graph_captures(self) -> int:
        """hipGraph captures of the LM pass so far (a stream of equally shaped batches captures once)."""
        return int(self._lib.ctvio_graph_captures(self._h))

    @property
    def stream(self) -> int:
        return int(self._lib.ctvio_stream(self._h) or 0)
