"""GPU (-m gpu): the per-block device math (ctrl-vio_amd/csrc/so3.hpp, factors.hpp, ls_poly.hpp) AS BUILT FOR gfx950 -- contraction into
fma, the device library's sin / cos / atan / sqrt, the device inliner -- against the references the g++ build of the same headers is held to
in tests/test_device_math_host.py, tests/test_*jac_host.py, tests/test_imustep_host.py and tests/test_ls_poly_host.py, at the same bounds.
The case bodies are tests/math_cases.hpp, compiled once by g++ for those tests and once by hipcc into tests/_build/libdevprobe.so
(tests/device_math_probe.hip: one thread per case, blocks of 64; built by __graft_entry__.build() with the library's hipcc line).  Every
family runs in batches of 1, 64, 65, 130 and then 130 cases: a lone thread, a full block, a second block of one thread, a ragged third
block.  A family with fewer than 260 cases is sent with its cases repeated cyclically up to 260 rows (tests/devprobe.py: Device), and a
repeated case must return the bits of its first copy.

Every test prints its worst error over its bound.  Measured on an MI355X (worst error / bound; DESIGN.md section 6 has the table):
  Lie primitives   exp 2.2e-3, Jr 1.1e-3, Jr^-1 1.4e-3, log(exp) 5.6e-4, exp_small 1.1e-3, Jr_small 5.6e-4, log 7.1e-4, qmul 2.0e-3,
                   qmul_unit 2.0e-3, basis 4.4e-3                              (absolute: 2.2e-16 ... 5.4e-16)
  IMU block        2.4e-4 (config1), 9.2e-5 (large rotation)                   visual block   6.4e-3 (both forms), 7.0e-4 (large rotation)
  pose / nav       1.8e-4          rates   8.9e-5          proj   1.2e-3          pred   6.0e-5
  rel              3.5e-4          imu_step   3.4e-2;   |q| - 1 = 1.1e-16 against 1e-15 in both
  line search      1.1e-7 (2 samples), 2.0e-6 (3 samples), 3.2e-7 (edges); ls_root_real_parts 9.6e-3 of 1e-12
The device build sits where the g++ build does: a factor of 100 or more inside every bound.
Angles within 0.1 of pi are out of scope (tests/lie_fixture.py says why)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@pytest.fixture(scope="module")
def dev():
    import devprobe
    return devprobe.Device()          # raises with "run __graft_entry__.build()" if the probe is missing: nothing is compiled here


@pytest.fixture(scope="module")
def win(cv):
    return cv.synth.make_window("config1", seed=1003)


def _report(name, worst):
    print(f"{name}: worst error / bound {worst:.3g}")
    assert worst <= 1.0, (name, worst)


def _large_rotation(w):
    """q_k <- q_k * exp(k * 0.7 e_z): consecutive knots 0.7 rad further apart (tests/test_gpu_parity.py: test_imu_linearize_general_body
    [large_rotation]), so every knot-pair log is beyond the series' range and the closed-form branches run"""
    from scipy.spatial.transform import Rotation as R
    w = w.copy()
    for k in range(w.quat.shape[0]):
        w.quat[k] = (R.from_quat(w.quat[k]) * R.from_rotvec([0.0, 0.0, 0.7 * k])).as_quat()
    return w


# ------------------------------------------------------------------------------------------------ Lie primitives
def test_lie_primitives_match_high_precision_fixture(dev):
    """so3_exp / Jr / Jr_inv / log(exp), the series-only forms, so3_log on quaternions (other cover, both thresholds), qmul / qmul_unit and
    the spline basis against mpmath at 50 digits (tests/golden/lie_edge_grid.npz), at the bounds of test_lie_primitives."""
    import devprobe
    import lie_fixture
    fx = lie_fixture.load()
    assert len(fx["phi"]) == sum(devprobe.BATCHES) + 39          # the grid runs as batches of 1, 64, 65, 130 and 39 cases
    lie_fixture.check(fx, dev, "device")


# ------------------------------------------------------------------------------------------------ IMU and visual blocks against the oracle
def _imu_cases(w, ms):
    st = w.imu_t[ms].astype(np.int64) - w.t0_ns
    s, u = st // w.dt_ns, (st % w.dt_ns) / w.dt_ns
    q = np.stack([w.quat[k:k + 4].ravel() for k in s]); p = np.stack([w.pos[k:k + 4].ravel() for k in s])
    return q, p, u, np.full(len(ms), 1e9 / w.dt_ns), w.gravity, w.bias[w.imu_bias[ms]], w.imu_gyro[ms], w.imu_acc[ms], w.imu_w


@pytest.mark.parametrize("rotation", ["config1", "large_rotation"])
def test_imu_block_matches_oracle(cv, oracle, dev, win, rotation):
    """The cases and the bound of tests/test_device_math_host.py::test_imu_block_matches_oracle on the device build; large_rotation: the
    same samples on a spline whose knot-pair logs exceed 0.5 rad."""
    rtol = 1e-11
    w = win if rotation == "config1" else _large_rotation(win)
    o = oracle.OracleWindow(w)
    ms = np.arange(0, w.M, 37)
    r, J = dev.imu_eval(*_imu_cases(w, ms))
    worst = 0.0
    for i, m in enumerate(ms):
        r0, J0, _ = o.imu_block(int(m))
        worst = max(worst, np.abs(r[i] - r0).max() / (rtol * max(np.abs(r0).max(), 1.0)), np.abs(J[i] - J0).max() / (rtol * np.abs(J0).max()))
    _report(f"imu block, {rotation}", worst)


def _vis_cases(w, vs):
    ld_ns = int(w.ld * 1e9)
    ti = w.v_ti[vs].astype(np.int64) + w.v_rowi[vs].astype(np.int64) * ld_ns - w.t0_ns
    tj = w.v_tj[vs].astype(np.int64) + w.v_rowj[vs].astype(np.int64) * ld_ns - w.t0_ns
    si, ui = ti // w.dt_ns, (ti % w.dt_ns) / w.dt_ns
    sj, uj = tj // w.dt_ns, (tj % w.dt_ns) / w.dt_ns
    n = len(vs)
    qi = np.stack([w.quat[k:k + 4].ravel() for k in si]); pi = np.stack([w.pos[k:k + 4].ravel() for k in si])
    qj = np.stack([w.quat[k:k + 4].ravel() for k in sj]); pj = np.stack([w.pos[k:k + 4].ravel() for k in sj])
    sc = np.stack([ui, uj, np.full(n, 1e9 / w.dt_ns), np.full(n, w.img_w), np.full(n, w.cauchy_a), w.v_rowi[vs].astype(float),
                   w.v_rowj[vs].astype(float), w.rho[w.v_lm[vs]]], axis=1)
    obs = np.concatenate([w.v_pi[vs], w.v_pj[vs]], axis=1)
    return qi, pi, qj, pj, sc, w.q_CI, w.p_CI, obs


@pytest.mark.parametrize("small,rotation", [(0, "config1"), (1, "config1"), (0, "large_rotation")])
def test_visual_block_matches_oracle(cv, oracle, dev, win, small, rotation):
    """The cases and the bounds of tests/test_device_math_host.py::test_visual_block_matches_oracle on the device build: the general form
    and the series-only form (its contract: knot-pair logs below 0.5 rad), and the general form on the large-rotation spline."""
    from test_device_math_host import _corrected
    rtol = 1e-10
    w = (win if rotation == "config1" else _large_rotation(win)).copy()
    w.ld = 1.7e-5
    o = oracle.OracleWindow(w)
    vs = np.arange(0, w.V, 7)
    r, J, cost = dev.visual_eval(small, *_vis_cases(w, vs))
    worst = 0.0
    for i, v in enumerate(vs):
        r0, J0, si, sj = o.visual_block(int(v))
        rc, Jc, cost0 = _corrected(w, r0, J0)
        colscale = np.maximum(np.abs(Jc).max(0), 1e-3 * np.abs(Jc).max())
        worst = max(worst, np.abs(r[i] - rc).max() / (rtol * max(np.abs(rc).max(), 1.0)), (np.abs(J[i] - Jc) / colscale).max() / rtol,
                    abs(cost[i] - cost0) / (1e-10 * abs(cost0) + 1e-12))
        assert cost[i] == pytest.approx(cost0, rel=1e-10, abs=1e-12)
    _report(f"visual block, small={small}, {rotation}", worst)


# ------------------------------------------------------------------------------------------------ query Jacobians against NumPy
def _knots(w, segs):
    return np.stack([w.quat[s:s + 4].ravel() for s in segs]), np.stack([w.pos[s:s + 4].ravel() for s in segs])


def _seg_u(w):
    return [(s, u) for s in range(0, w.K - 3, 2) for u in (0.0, 0.25, 0.9)]


@pytest.mark.parametrize("cam", [False, True], ids=["body", "camera"])
def test_pose_jacobian_matches_numpy(cv, dev, win, cam):
    """tests/test_posejac_host.py on the device build: rtol 1e-11; the last knot's blocks are exact zeros at u = 0."""
    import posecov_helpers as ph
    rtol = 1e-11
    w = win
    q_SI = np.ascontiguousarray(w.q_CI / np.linalg.norm(w.q_CI)); p_SI = np.ascontiguousarray(w.p_CI)
    cases = _seg_u(w)
    jacs = [ph.pose_jacobian(w, ph.time_of(w, s, u), *((q_SI, p_SI) if cam else (None, None))) for s, u in cases]
    jt = dev.pose_jac(_knots(w, [s for s, _ in cases])[0], np.array([j.u for j in jacs]), cam, q_SI, p_SI)
    worst = 0.0
    for i, ((s, u), jac) in enumerate(zip(cases, jacs)):
        ref = jac.J[:, 6 * s:6 * s + 24]
        worst = max(worst, np.abs(jt[i].T - ref).max() / (rtol * np.abs(ref).max()))
        if u == 0.0:
            assert not jt[i, 18:].any()
    _report(f"pose_jac_T, {'camera' if cam else 'body'}", worst)


def test_nav_jacobian_matches_numpy(cv, dev, win):
    """tests/test_navjac_host.py on the device build: rtol 1e-11; the last knot's blocks and c'_3 are exact zeros at u = 0."""
    import navstate_helpers as nh
    rtol = 1e-11
    w = win
    cases = _seg_u(w)
    jacs = [nh.nav_jacobian(w, nh.time_of(w, s, u)) for s, u in cases]
    jt, cv4 = dev.nav_jac(_knots(w, [s for s, _ in cases])[0], np.array([j.u for j in jacs]), np.full(len(cases), 1e9 / w.dt_ns))
    worst = 0.0
    for i, ((s, u), jac) in enumerate(zip(cases, jacs)):
        ref = jac.J[:6, 6 * s:6 * s + 24]
        vel = np.zeros((3, 24))
        for k in range(len(jac.knots)):
            vel[:, 6 * k + 3:6 * k + 6] = cv4[i, k] * np.eye(3)
        worst = max(worst, np.abs(jt[i].T - ref).max() / (rtol * np.abs(ref).max()), np.abs(cv4[i] - jac.cv).max() / (rtol * np.abs(jac.cv).max()),
                    np.abs(vel - jac.J[6:9, 6 * s:6 * s + 24]).max() / (rtol * np.abs(jac.cv).max()))
        if u == 0.0:
            assert not jt[i, 18:].any() and cv4[i, 3] == 0.0
    _report("nav_jac_T", worst)


@pytest.mark.parametrize("cfg, seed", [("tiny", 7), ("config1", 1003)])
def test_rates_jacobian_matches_numpy(cv, dev, cfg, seed):
    """tests/test_ratesjac_host.py on the device build: every row block (omega, f, v_B) at rtol 1e-11 of its largest entry; at u = 0 the
    last knot's rows are exact zeros."""
    import rates_helpers as rh
    rtol = 1e-11
    w = cv.synth.make_window(cfg, seed=seed)
    cases = _seg_u(w)
    jacs = [rh.rates_jacobian(w, rh.time_of(w, s, u)) for s, u in cases]
    q, p = _knots(w, [s for s, _ in cases])
    jt = dev.rates_jac(q, p, np.array([j.u for j in jacs]), np.full(len(cases), 1e9 / w.dt_ns), np.ascontiguousarray(w.gravity, dtype=np.float64))
    worst = 0.0
    for i, ((s, u), jac) in enumerate(zip(cases, jacs)):
        ref = jac.J[:9, 6 * s:6 * s + 24]
        for blk in (rh.OMEGA, rh.FORCE, rh.VELB):
            worst = max(worst, np.abs(jt[i].T[blk] - ref[blk]).max() / np.abs(ref[blk]).max() / rtol)
        if u == 0.0:
            assert not jt[i, 18:].any()
    _report(f"rates_jac_T, {cfg}", worst)


@pytest.mark.parametrize("ext", [False, True], ids=["body", "extrinsic"])
def test_rel_jacobian_matches_numpy(cv, dev, win, ext):
    """tests/test_relpose_host.py on the device build: both 24 x 6 blocks at rtol 1e-11, the value, exact zeros at u = 0."""
    import relpose_helpers as rh
    from test_relpose_host import EXT, PAIRS
    rtol = 1e-11
    w = win
    q_SI, p_SI = EXT if ext else (None, None)
    qe, pe = (np.ascontiguousarray(EXT[0]), np.ascontiguousarray(EXT[1])) if ext else (np.array([0.0, 0, 0, 1]), np.zeros(3))
    times = [(rh.time_of(w, sa, ua), rh.time_of(w, sb, ub)) for (sa, ua), (sb, ub) in PAIRS]
    jacs = [rh.rel_jacobian(w, ta, tb, q_SI, p_SI) for ta, tb in times]
    qa, pa = _knots(w, [a[0] for a, _ in PAIRS]); qb, pb = _knots(w, [b[0] for _, b in PAIRS])
    jt_a, jt_b, rel7 = dev.rel_pose_jac(qa, pa, np.array([j.a.u for j in jacs]), qb, pb, np.array([j.b.u for j in jacs]), ext, qe, pe)
    worst = 0.0
    unit = 0.0
    for i, (((sa, ua), (sb, ub)), jac) in enumerate(zip(PAIRS, jacs)):
        J = np.zeros((6, w.P))
        J[:, 6 * sa:6 * sa + 24] += jt_a[i].T          # a-term + b-term, the kernel's order
        J[:, 6 * sb:6 * sb + 24] += jt_b[i].T
        scale = max(np.abs(jt_a[i]).max(), np.abs(jt_b[i]).max())
        R, p = rh.rel_numpy(w, *times[i], q_SI, p_SI)
        worst = max(worst, np.abs(J - jac.J).max() / scale / rtol, (rh.Rot.from_quat(rel7[i, 3:]).inv() * R).magnitude() / 1e-12,
                    np.abs(rel7[i, :3] - p).max() / (1e-12 * max(1.0, np.abs(p).max())))
        unit = max(unit, abs(np.linalg.norm(rel7[i, 3:]) - 1.0) / 1e-15)
        if ua == 0.0:
            assert not jt_a[i, 18:].any()
        if ub == 0.0:
            assert not jt_b[i, 18:].any()
    _report(f"rel_pose_jac_T, {'extrinsic' if ext else 'body'}", worst)
    _report("rel_pose_jac_T, |q_ab| - 1 against 1e-15", unit)


def test_projection_jacobian_matches_numpy(cv, dev, win):
    """tests/test_projjac_host.py on the device build: both 24 x 2 blocks, the inverse-depth and line-delay columns and the value at rtol
    1e-11; exact zeros at u = 0 and, on row 0 of both ends, in the line-delay column."""
    import posecov_helpers as ph
    import projection_helpers as pr
    from test_projjac_host import CASES
    rtol = 1e-11
    w0 = win.copy()
    w0.ld = 2.0e-5                                # the row time is not the frame time
    ld_ns = int(np.int64(w0.ld * 1e9))
    l = int(w0.v_lm[0])
    pjs, ua_l, obs = [], [], []
    for (sa, ua, ra), (sq, uq, rq) in CASES:
        w = w0.copy()
        tau_a, tau_q = ph.time_of(w, sa, ua), ph.time_of(w, sq, uq)
        mine = w.v_lm == l
        w.v_ti[mine] = tau_a - ra * ld_ns          # the landmark re-anchored at (segment sa, u ua) on row ra
        w.v_rowi[mine] = ra
        pj = pr.projection_jacobian(w, l, tau_q - rq * ld_ns, rq)
        assert pj is not None and (pj.s_a, pj.s_q) == (sa, sq) and pj.tau_q == tau_q
        u_a = ph.segment(w, tau_a)[1]
        assert (u_a == 0.0) == (ua == 0.0) and (pj.u_q == 0.0) == (uq == 0.0)
        pjs.append(pj); ua_l.append(u_a)
        obs.append([w.v_pi[mine][0, 0], w.v_pi[mine][0, 1], w.rho[l]])
    w = w0
    qa, pa = _knots(w, [a[0] for a, _ in CASES]); qq, pq = _knots(w, [b[0] for _, b in CASES])
    jt_a, jt_q, out7 = dev.proj_jac(qa, pa, np.array(ua_l), qq, pq, np.array([pj.u_q for pj in pjs]), np.full(len(CASES), 1e9 / w.dt_ns),
                                    np.ascontiguousarray(w.q_CI, float), np.ascontiguousarray(w.p_CI, float), np.array(obs),
                                    np.array([[float(a[2]), float(b[2])] for a, b in CASES]))
    worst = 0.0
    for i, (((sa, ua, ra), (sq, uq, rq)), pj) in enumerate(zip(CASES, pjs)):
        J = np.zeros((2, w.P))
        J[:, 6 * sa:6 * sa + 24] += jt_a[i].T          # anchor term + query term, the kernel's order
        J[:, 6 * sq:6 * sq + 24] += jt_q[i].T
        J[:, w.P - 1] = out7[i, 5:7]
        scale = max(np.abs(jt_a[i]).max(), np.abs(jt_q[i]).max())
        d = float(np.abs(J[:, :6 * w.K] - pj.Jp[:, :6 * w.K]).max() / scale)
        d = max(d, float(np.abs(out7[i, 3:5] - pj.j).max() / max(1.0, np.abs(pj.j).max())))
        d = max(d, float(np.abs(out7[i, 5:7] - pj.Jp[:, w.P - 1]).max() / max(1.0, np.abs(pj.Jp[:, w.P - 1]).max())))
        d = max(d, float(np.abs(out7[i, :3] - pj.proj).max() / max(1.0, np.abs(pj.proj).max())))
        worst = max(worst, d / rtol)
        if ua == 0.0:
            assert not jt_a[i, 18:].any()
        if uq == 0.0:
            assert not jt_q[i, 18:].any()
        if ra == 0 and rq == 0:
            assert not out7[i, 5:7].any()
    _report("proj_jac_T / proj_cols", worst)


def test_prediction_maps_match_numpy(dev):
    """tests/test_predjac_host.py on the device build: the pose at the row time, the value, B, C_ext and A at rtol 1e-11; at delta = 0 the
    velocity and gyro-bias columns of A are exact zeros and B's rotation block is the identity to the bit."""
    import imuprop_helpers as ih
    import predproj_helpers as pp
    from scipy.spatial.transform import Rotation as Rot
    from test_predjac_host import CASES
    rtol = 1e-11
    rows, refs = [], []
    for rate, delta in CASES:
        rng = np.random.default_rng(int(1000 * rate) + 7)
        for _ in range(4):
            q_e = Rot.from_rotvec(rng.normal(0, 1.0, 3)).as_quat()
            p_e, v_e = rng.normal(0, 1.0, 3), rng.normal(0, 1.5, 3)
            w_e = rng.normal(0, 1.0, 3); w_e *= rate / np.linalg.norm(w_e)
            q_CI = Rot.from_rotvec(rng.normal(0, 0.3, 3)).as_quat()
            p_CI = rng.normal(0, 0.1, 3)
            w = SimpleNamespace(q_CI=q_CI, p_CI=p_CI)
            R_e = Rot.from_quat(q_e).as_matrix()
            RI, pI = pp.row_pose((R_e, p_e, v_e), w_e, delta)
            RC = RI @ Rot.from_quat(q_CI).as_matrix()
            y = np.array([rng.normal(0, 0.5), rng.normal(0, 0.5), rng.uniform(2.0, 8.0)])          # in front of the camera
            X = RC @ y + pI + RI @ p_CI
            rows.append((q_e, p_e, v_e, w_e, [delta], X, q_CI, p_CI))
            refs.append((rate, delta, w_e, RI, pI, y, pp.A_matrix(w, y, RI, w_e, delta)[0], pp.B_matrix(w_e, delta), pp.C_ext(w, RI)))
    pose7, proj3, B, Cx, A = dev.pred_jac(*[np.array([r[k] for r in rows]) for k in range(8)])
    worst = 0.0
    for i, (rate, delta, w_e, RI, pI, y, An, Bn, Cn) in enumerate(refs):
        worst = max(worst, np.abs(pose7[i, :3] - pI).max() / (rtol * max(1.0, np.abs(pI).max())),
                    (Rot.from_quat(pose7[i, 3:]).inv() * Rot.from_matrix(RI)).magnitude() / rtol,
                    np.abs(proj3[i] - np.array([y[0] / y[2], y[1] / y[2], y[2]])).max() / (rtol * max(1.0, np.abs(y).max())))
        for got, want in ((B[i], Bn), (Cx[i], Cn), (A[i], An)):
            worst = max(worst, np.abs(got - want).max() / (rtol * max(1.0, np.abs(want).max())))
        if delta == 0.0:
            assert not A[i][:, 6:].any() and np.array_equal(B[i][:3, :3], np.eye(3)) and not B[i][:, 6:].any()
        else:
            assert A[i][:, 6:12].any()
        assert not A[i][:, 12:].any()
        if rate * delta == 1e-9:                       # the series branch: Jr = I - [phi]x / 2 to rounding
            assert np.abs(B[i][:3, 9:12] + delta * (np.eye(3) - 0.5 * ih.hat(w_e * delta))).max() <= 1e-16 * delta
    _report("pred_row_pose / pred_B / pred_Cext / pred_A", worst)


def test_imu_step_matches_numpy(dev):
    """tests/test_imustep_host.py on the device build: the mean and the seven blocks at rtol 1e-11 (the rotation at 1e-14), w = 0 exactly
    and |w dt| = 1e-9 included; the mean does not depend on the request for blocks."""
    import imuprop_helpers as ih
    from scipy.spatial.transform import Rotation as Rot
    from test_imustep_host import _cases
    rtol = 1e-11
    g = np.array([0.0, 0.0, 9.81])
    xs, meas, dts, meta = [], [], [], []
    for ci, (name, rate, dt) in enumerate(_cases()):
        for seed in range(4):
            rng = np.random.default_rng(100 * ci + seed)
            q = Rot.from_rotvec(rng.normal(0, 1.0, 3)).as_quat()
            R = Rot.from_quat(q).as_matrix()
            p, v, bg, ba = rng.normal(0, 2.0, 3), rng.normal(0, 1.0, 3), rng.normal(0, 1e-2, 3), rng.normal(0, 1e-1, 3)
            axis = rng.normal(0, 1.0, 3)
            w = rate * axis / np.linalg.norm(axis)
            half = rng.normal(0, 0.05, 3) if rate >= 0.1 else np.zeros(3)
            w0, w1 = (w + bg) + half, (w + bg) - half            # the midpoint minus bg is w (to rounding; exactly for w = 0: bg - bg)
            if rate == 0.0:
                w0 = w1 = bg.copy()
            a0, a1 = R.T @ g + rng.normal(0, 1.0, 3), R.T @ g + rng.normal(0, 1.0, 3)
            xs.append(np.concatenate([q, p, v, bg, ba])); meas.append(np.concatenate([w0, a0, w1, a1])); dts.append(dt)
            meta.append((name, rate, dt, (R, p, v, bg, ba), w0, a0, w1, a1))
    xs, meas, dts = np.array(xs), np.array(meas), np.array(dts)
    x, blocks = dev.imu_step(xs, meas, g, dts, want_blocks=True)
    xm, _ = dev.imu_step(xs, meas, g, dts, want_blocks=False)
    assert np.array_equal(x, xm)                                  # the mean does not depend on the request for blocks
    worst = 0.0
    unit = 0.0
    for i, (name, rate, dt, st, w0, a0, w1, a1) in enumerate(meta):
        R, p, v, bg, ba = st
        R1, p1, v1, _, _ = ih.step(st, w0, a0, w1, a1, dt, g)
        F, G = ih.jacobians(st, w0, a0, w1, a1, dt)
        worst = max(worst, (Rot.from_quat(x[i, 0:4]).inv() * Rot.from_matrix(R1)).magnitude() / 1e-14)
        unit = max(unit, abs(np.linalg.norm(x[i, 0:4]) - 1.0) / 1e-15)
        for got, ref in ((x[i, 4:7], p1), (x[i, 7:10], v1)):
            worst = max(worst, np.abs(got - ref).max() / (rtol * max(1.0, np.abs(ref).max())))
        assert np.array_equal(x[i, 10:], np.concatenate([bg, ba]))
        refs = [F[ih.TH, ih.TH], F[ih.TH, ih.BG], F[ih.VV, ih.TH], F[ih.VV, ih.BG], F[ih.VV, ih.BA], R, R1]
        for b, ref in zip(blocks[i], refs):
            worst = max(worst, np.abs(b - ref).max() / (rtol * np.abs(ref).max()))
        if rate == 0.0:                                           # Exp(0) = I and Jr(0) = I exactly
            assert np.array_equal(blocks[i, 0], np.eye(3)) and np.array_equal(blocks[i, 1], -dt * np.eye(3))
            assert np.abs(blocks[i, 5] - blocks[i, 6]).max() <= 1e-15
    _report("imu_step", worst)
    _report("imu_step, |q| - 1 against 1e-15", unit)


# ------------------------------------------------------------------------------------------------ the line-search interpolation
@pytest.mark.parametrize("ns", [2, 3])
def test_interpolating_minimiser_matches_numpy(dev, ns):
    """ls_minimize_interpolating as built for the device (lm_decide's step on one lane of k_pass_end): 300 seeded cases, lo <= x <= hi and
    |p(x) - best| <= 1e-9 max(1, |best|) against NumPy's solve / roots, as tests/test_ls_poly_host.py asks of the g++ build."""
    import ls_cases
    ls_cases.check_against_reference(dev, ns, *ls_cases.random_cases(ns), label=f"device, {ns} samples")


def test_interpolating_minimiser_edges(dev):
    """Coincident abscissae (the midpoint exactly), lo == hi, constant data, a nearly degenerate quadratic derivative, a derivative with a
    complex pair, a quintic with four real critical points inside the interval: tests/ls_cases.py."""
    import ls_cases
    ls_cases.check_edges(dev, "device")


def test_exactly_quadratic_data_trims_the_derivative(dev):
    """The device build's elimination leaves an exact zero in front of exactly quadratic data (the data are dyadic: also under fma), the
    derivative is trimmed to a line and the result is that line's root, to the bit."""
    import ls_cases
    ls_cases.check_trimming(dev, "device")


def test_root_real_parts(dev):
    """ls_root_real_parts as built for the device, directly: trimming, deg == 1, both orders of the quadratic formula, Durand-Kerner,
    against numpy.roots (tests/ls_cases.py: check_roots)."""
    import ls_cases
    ls_cases.check_roots(dev, "device")
