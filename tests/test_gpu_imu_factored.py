"""GPU (-m gpu): the fast body of the IMU linearisation (k_imu_linearize_f64 / k_linearize_f64: Gram matrices in pair-log coordinates,
world-frame accelerometer rows, the 4x4x4 product with the position weights, one T^T G^ T per group) against the fp64 oracle and against
the general body, on `tiny` and `config1` windows whose IMU samples are re-cut so that the groups have the sizes at which the body changes
its path: a partial first pass (1, 3, 4, 5: the K-steps round to 4 and 8 rows), a full pass and one around it (63, 64, 65), and second passes
with many and with one live lane (100, 128, 129).  Bounds: test_gpu_parity.py's for test_linearize_matches_oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 63, 64, 65, 100, 128, 129]


def _scaled(H):
    return np.sqrt(np.maximum(np.diag(H), 1e-30))


def _recut(w, sizes):
    """The window with group g (the samples of one (segment, bias state) pair, in time order) re-cut to sizes[g % len(sizes)] samples spread
    over the group's time span; every new sample takes the measurement of the group's original sample nearest in time."""
    w = w.copy()
    seg = (w.imu_t - w.t0_ns) // w.dt_ns
    key = seg * 1000 + w.imu_bias
    t_new, src = [], []
    for g, kv in enumerate(np.unique(key)):
        idx = np.flatnonzero(key == kv)
        n = sizes[g % len(sizes)]
        lo, hi = int(w.imu_t[idx[0]]), int(w.imu_t[idx[-1]])
        t = lo + (np.arange(n, dtype=np.int64) * (hi - lo + 1)) // n
        t_new.append(t)
        src.append(idx[np.abs(w.imu_t[idx][None, :] - t[:, None]).argmin(axis=1)])
    src = np.concatenate(src)
    w.imu_t = np.concatenate(t_new)
    w.imu_gyro, w.imu_acc, w.imu_bias = w.imu_gyro[src].copy(), w.imu_acc[src].copy(), w.imu_bias[src].copy()
    w.normalize()
    return w


def _group_sizes(w):
    key = ((w.imu_t - w.t0_ns) // w.dt_ns) * 1000 + w.imu_bias
    return sorted(np.unique(key, return_counts=True)[1].tolist())


@pytest.fixture(scope="module")
def recut(cv, oracle):
    """name -> (window, the oracle's H, g, cost): computed once, shared by the tests below and never modified (they copy the window)."""
    tiny = _recut(cv.synth.make_window("tiny", seed=3), SIZES[:8])              # 8 groups
    cfg1 = cv.synth.make_window("config1", seed=1000)
    cfg1.ld = 1.1e-5
    cfg1 = _recut(cfg1, SIZES)                                                   # 20 groups: every size twice
    assert _group_sizes(tiny) == sorted(SIZES[:8]) and _group_sizes(cfg1) == sorted(SIZES + SIZES)
    fixed = cfg1.copy()
    fixed.knot_const = np.zeros(fixed.K, np.uint8)
    fixed.knot_const[[0, 1, 5, 9]] = 1
    near = cfg1.copy()                                                           # every knot-pair log 0.49 rad long: the series' last groups
    rng = np.random.default_rng(5)
    from scipy.spatial.transform import Rotation as R
    for k in range(near.K - 1):
        d = rng.normal(0.0, 1.0, 3)
        near.quat[k + 1] = (R.from_quat(near.quat[k]) * R.from_rotvec(0.49 * d / np.linalg.norm(d))).as_quat()
    near.normalize()
    aniso = cfg1.copy()
    aniso.imu_w = np.array([250.0, 250.0, 250.0, 12.5, 10.0, 15.0])
    out = {}
    for name, w in (("tiny", tiny), ("config1", cfg1), ("fixed_knots", fixed), ("logs_0.49", near), ("anisotropic_accel", aniso)):
        out[name] = (w,) + tuple(oracle.OracleWindow(w.copy()).build_normal())
    return out


def _check(name, got, H, g, cost, P):
    Hg, Wg, Hllg, gg, costg = got
    sc = _scaled(H)
    eH = np.abs((Hg - H[:P, :P]) / np.outer(sc[:P], sc[:P])).max()
    eg = np.abs((gg - g) / sc).max() / np.abs(g / sc).max()
    print(f"{name}: cost rel {abs(costg / cost - 1):.3g}, Hpp scaled {eH:.3g}, g scaled {eg:.3g}")
    assert costg == pytest.approx(cost, rel=1e-12)
    assert eH < 1e-10
    assert eg < 1e-10


@pytest.mark.parametrize("name", ["tiny", "config1", "fixed_knots", "logs_0.49", "anisotropic_accel"])
def test_fast_body_matches_oracle(cv, recut, name):
    """Solver.linearize(0) against the oracle's dense normal equations.  (anisotropic_accel: the accelerometer weights differ per axis, the
    rows may not be rotated: imu_fast_pred sends every group to the general body, which must still match.)"""
    w, H, g, cost = recut[name]
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        got = s.linearize(0)
    _check(name, got, H, g, cost, w.P)


@pytest.mark.parametrize("name", ["tiny", "config1", "logs_0.49"])
def test_fast_body_matches_general_body(cv, recut, name):
    """The same windows with every group through the general body (use_mfma = 2, the independent cross-check: local frame, closed forms,
    Jr^-1 applied per sample, 32-column accelerometer rows)."""
    w, H, _, _ = recut[name]
    P = w.P
    sc = _scaled(H)
    res = []
    for mfma in (1, 2):
        with cv.Solver(use_mfma=mfma) as s:
            s.set_windows([w.copy()])
            res.append(s.linearize(0))
    (Hf, _, _, gf, cf), (Hq, _, _, gq, cq) = res
    eH = np.abs((Hf - Hq) / np.outer(sc[:P], sc[:P])).max()
    eg = np.abs((gf - gq) / sc).max() / np.abs(gq / sc).max()
    print(f"{name}: fast against general: cost rel {abs(cf / cq - 1):.3g}, Hpp scaled {eH:.3g}, g scaled {eg:.3g}")
    assert cf == pytest.approx(cq, rel=1e-12)
    assert eH < 1e-10 and eg < 1e-10


def test_batch_of_130_takes_the_walking_kernel(cv, oracle):
    """More than 128 windows: k_imu_linearize_f64's waves walk the groups (up to 128 the merged k_linearize_f64 runs the same body).  130 tiny
    windows (5 distinct ones, 26 copies each): every window's normal equations equal its single-window ones, and the 15-iteration solve
    keeps the oracle's iteration counts and state."""
    base = [_recut(cv.synth.make_window("tiny", seed=30 + i), SIZES[i:] + SIZES[:i]) for i in range(4)] + [cv.synth.make_window("tiny", seed=34)]
    with cv.Solver() as s:
        singles = []
        for w in base:
            s.set_windows([w.copy()])
            singles.append(s.linearize(0))
        s.set_windows([base[i % 5].copy() for i in range(130)])
        worst = [0.0, 0.0, 0.0]
        for i in range(130):
            Hs, _, Hlls, gs, cs = singles[i % 5]
            Hb, _, _, gb, cb = s.linearize(i)
            sc = _scaled(Hs)
            sg = np.concatenate([sc, np.sqrt(np.maximum(Hlls, 1e-30))])      # (g runs over the trajectory unknowns and the landmarks)
            e = (abs(cb / cs - 1), np.abs((Hb - Hs) / np.outer(sc, sc)).max(), np.abs((gb - gs) / sg).max() / np.abs(gs / sg).max())
            worst = [max(a, b) for a, b in zip(worst, e)]
        print(f"batch against single: cost rel {worst[0]:.3g}, Hpp scaled {worst[1]:.3g}, g scaled {worst[2]:.3g}")
        assert worst[0] <= 1e-12 and worst[1] < 1e-10 and worst[2] < 1e-10
        refs = [w.copy() for w in base]
        sms_o = [oracle.OracleWindow(r).solve(15) for r in refs]
        batch = [base[i % 5].copy() for i in range(130)]
        s.set_windows(batch)
        sms = s.solve(15)
    for i in range(130):
        so = sms_o[i % 5]
        assert (sms[i]["iterations"], sms[i]["num_successful"], sms[i]["num_unsuccessful"]) == (so.iterations, so.num_successful, so.num_unsuccessful), i
        assert sms[i]["final_cost"] == pytest.approx(so.final_cost, rel=1e-9), i
        assert cv.rel_state_error(batch[i], refs[i % 5])["state"] < 1e-6, i
