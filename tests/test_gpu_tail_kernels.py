"""GPU (-m gpu): the three per-window tail kernels of a pass against the oracle -- k_misc's IMU share (assemble_imu_window: bias rows, bias
block and gradient of the group tiles, lanes along global columns), k_step_finish (landmark back-substitution over each row's own span, the
candidate) and k_pass_end (cost, gradient norm, line search, accept / reject).

The accumulate path needs a throughput-mode batch of more than 128 windows (one visual-assembly part per window, k_misc with the IMU share in
front), so every test runs a batch of 130 made of a handful of distinct small windows; the landmark step also runs at 200 windows, where
k_step_finish takes its 256-thread shape.

Windows:
  cut      tiny, IMU samples re-assigned and removed so that the biases own 3, 2, 2 and 1 groups (a frame boundary inside a segment), prior
  noprior  tiny without a prior
  k33      tiny, dt 15 ms: K = 33, the Hessian is not LDS-resident -- the LDS band in front of the bias rows
  k6_hole  tiny, dt 200 ms: K = 6, spans of one knot quadruple and of the whole window in one 8-row trip; landmark 5 has no observation
           (klo = K, khi = -1, a fixed unknown); its solve has rejected steps and line searches of several trial steps
  l13      tiny with 13 landmarks, l201 with 201 (not multiples of 8, one and many trips per wave)
  ld_hi    tiny, the line delay starts on its upper bound: the projected line search runs in seven iterations
Bounds are those of tests/test_gpu_parity.py: test_linearize_matches_oracle (1e-10 on the scaled H, W, Hll, g; cost rel 1e-12),
test_lm_step_matches_oracle (1e-8 of max |delta|, model change rel 1e-9) and the solve tests (decisions equal, cost rel 1e-9, state 1e-6).

Not covered as the issue words it: ctvio_lm_step hands out delta and the model change only, so ls_gd0, ls_dmax, step2 and cand_xnorm2 are
checked through what they decide (the line-search and termination records of the solves below); and no synthetic window was found whose
FIRST step is rejected -- k6_hole rejects five later ones."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-10
NBATCH = 130
DECISIONS = ("iterations", "num_successful", "num_unsuccessful", "num_line_search_steps", "num_line_search_reduced")


def _cut(cv):
    w = cv.synth.make_window("tiny", seed=1000)
    t = np.asarray(w.imu_t)
    ib = np.asarray(w.imu_bias).copy()
    ib[(t >= 100_000_000) & (t < 125_000_000)] = 0           # the first half of segment 2 still belongs to bias 0: three groups
    keep = ~((ib == 3) & (t >= 350_000_000))                  # bias 3 keeps the samples of one segment: one group
    w.imu_t = t[keep]; w.imu_gyro = np.asarray(w.imu_gyro)[keep]; w.imu_acc = np.asarray(w.imu_acc)[keep]; w.imu_bias = ib[keep]
    w.normalize()
    seg = (np.asarray(w.imu_t) - w.t0_ns) // w.dt_ns
    assert [len(np.unique(seg[w.imu_bias == b])) for b in range(4)] == [3, 2, 2, 1]
    return w


def _k6_hole(cv):
    w = cv.synth.make_window("tiny", seed=1004, dt_ns=200_000_000)
    keep = np.asarray(w.v_lm) != 5
    for n in ("v_lm", "v_ti", "v_tj", "v_rowi", "v_rowj", "v_pi", "v_pj"):
        setattr(w, n, np.asarray(getattr(w, n))[keep])
    w.normalize()
    return w


def _ld_hi(cv):
    w = cv.synth.make_window("tiny", seed=1007)
    w.ld = w.ld_hi
    return w


WINDOWS = {
    "cut": _cut,
    "noprior": lambda cv: cv.synth.make_window("tiny", seed=1001, with_prior=False),
    "k33": lambda cv: cv.synth.make_window("tiny", seed=1002, dt_ns=15_000_000),
    "k6_hole": _k6_hole,
    "l13": lambda cv: cv.synth.make_window("tiny", seed=1003, L=13),
    "l201": lambda cv: cv.synth.make_window("tiny", seed=1003, L=201),
    "ld_hi": _ld_hi,
}
NAMES = list(WINDOWS)


@pytest.fixture(scope="module")
def wins(cv):
    """name -> window; never modified (the tests work on copies)."""
    out = {n: make(cv) for n, make in WINDOWS.items()}
    assert out["cut"].pn > 0 and out["noprior"].pn == 0 and out["k33"].K > 24 and out["k6_hole"].K == 6
    assert out["l13"].L == 13 and out["l201"].L == 201
    return out


def _batch(wins, n=NBATCH):
    return [wins[NAMES[i % len(NAMES)]].copy() for i in range(n)]


@pytest.fixture(scope="module")
def normal_refs(wins, oracle):
    return {n: oracle.OracleWindow(wins[n].copy()).build_normal() for n in ("cut", "noprior", "k33", "k6_hole")}


@pytest.fixture(scope="module")
def step_refs(wins, oracle):
    return {n: oracle.OracleWindow(wins[n].copy()).lm_step(1e4, use_schur=False) for n in ("l13", "l201", "k6_hole", "cut")}


@pytest.fixture(scope="module")
def solve_refs(wins, oracle):
    out = {}
    for n in NAMES:
        ref = wins[n].copy()
        out[n] = (ref, oracle.OracleWindow(ref).solve(15))
    return out


def test_normal_equations_after_one_linearisation(cv, wins, normal_refs):
    """Dense H and g of the accumulate path: every bias row against the knots, the bias block, the line-delay row and all of g, for one, two
    and three groups per bias, with and without a prior, LDS-resident and K > 24."""
    with cv.Solver(deterministic=0) as s:
        s.set_windows(_batch(wins))
        for name, (H, g, cost) in normal_refs.items():
            for i in (NAMES.index(name), NAMES.index(name) + 119):
                w = wins[name]
                assert NAMES[i % len(NAMES)] == name and i < NBATCH
                Hg, Wg, Hllg, gg, costg = s.linearize(i)
                P, K6 = w.P, 6 * w.K
                sc = np.sqrt(np.maximum(np.diag(H), 1e-30))
                eH = np.abs((Hg - H[:P, :P]) / np.outer(sc[:P], sc[:P]))
                live = np.diag(H) > 0                                     # (a landmark without observations has no row, column or gradient)
                obs = live[P:]
                errs = (abs(costg / cost - 1), eH.max(), eH[K6:P - 1, :K6].max(), eH[K6:P - 1, K6:P - 1].max(), eH[P - 1, K6:P - 1].max(),
                        np.abs((Wg - H[:P, P:])[:, obs] / np.outer(sc[:P], sc[P:][obs])).max(), np.abs(Hllg[obs] / np.diag(H)[P:][obs] - 1).max(),
                        np.abs((gg - g)[live] / sc[live]).max() / np.abs(g[live] / sc[live]).max())
                print(name, i, "cost, H, bias rows, bias block, line-delay row, W, Hll, g errors:", errs)
                assert costg == pytest.approx(cost, rel=1e-12)
                assert all(e < TOL for e in errs[1:]), (name, i, errs)


@pytest.mark.parametrize("nbatch", [130, 200])
def test_landmark_step(cv, wins, step_refs, nbatch):
    """delta of every unknown (the landmarks' from k_step_finish) and the model change after one step at mu = 1e4."""
    with cv.Solver(deterministic=0) as s:
        s.set_windows(_batch(wins, nbatch))
        for name, (d_o, mc_o) in step_refs.items():
            for i in (NAMES.index(name), NAMES.index(name) + 7 * ((nbatch - 7) // 7)):
                assert NAMES[i % len(NAMES)] == name and i < nbatch
                d_g, mc_g = s.lm_step(i, 1e4)
                P = wins[name].P
                print(name, i, "delta error (poses, landmarks):", np.abs(d_g - d_o)[:P].max() / np.abs(d_o).max(),
                      np.abs(d_g - d_o)[P:].max() / np.abs(d_o).max(), "model change:", mc_g / mc_o - 1)
                assert np.abs(d_g - d_o).max() <= 1e-8 * np.abs(d_o).max()
                assert mc_g == pytest.approx(mc_o, rel=1e-9)
        if "k6_hole" in step_refs:
            assert s.lm_step(NAMES.index("k6_hole"), 1e4)[0][wins["k6_hole"].P + 5] == 0.0     # the fixed landmark does not move


def test_line_search_and_rejection_records(cv, wins, solve_refs):
    """15-iteration solves of the whole batch: iteration, accept / reject, line-search and termination records equal the oracle's.
    k33 rides along (its band branch runs in every pass) but is not compared: its 15-iteration solve is not reproducible to the bound by the
    oracle itself -- the final cost moves by 5.6 % between the oracle's Schur and dense solves and by 6 % when the positions are scaled by
    1 + 1e-15 (every other window here: <= 4e-10) -- and the device's throughput mode lands 2e-4 (parent commit) / 2.7e-3 (this one) away."""
    assert solve_refs["ld_hi"][1].num_line_search_reduced > 0 and solve_refs["k6_hole"][1].num_unsuccessful > 0
    assert solve_refs["k6_hole"][1].num_line_search_steps > 2 * solve_refs["k6_hole"][1].num_line_search_reduced   # searches of several trial steps
    with cv.Solver(deterministic=0) as s:
        batch = _batch(wins)
        s.set_windows(batch)
        sms = s.solve(15)
    for i, (w, sm) in enumerate(zip(batch, sms)):
        if NAMES[i % len(NAMES)] == "k33":
            continue
        ref, so = solve_refs[NAMES[i % len(NAMES)]]
        assert tuple(sm[k] for k in DECISIONS) == tuple(getattr(so, k) for k in DECISIONS), (i, sm)
        assert sm["termination"] == cv.capi.TERMINATION[so.termination], (i, sm)
        assert sm["final_cost"] == pytest.approx(so.final_cost, rel=1e-9), i
        assert cv.rel_state_error(w, ref)["state"] < 1e-6, i


def test_deterministic_mode_is_bitwise(cv, wins):
    """deterministic = 2 (K = 33 is beyond 1) on the same batch: two solves on one handle and one on a fresh handle, bit for bit."""
    runs = []
    for rep in range(2):
        with cv.Solver(deterministic=2) as s:
            for again in range(2 if rep == 0 else 1):
                batch = _batch(wins)
                s.set_windows(batch)
                runs.append((s.solve(15), batch))
    sm0, b0 = runs[0]
    for sm, b in runs[1:]:
        assert sm == sm0
        for x, y in zip(b, b0):
            assert np.array_equal(x.quat, y.quat) and np.array_equal(x.pos, y.pos) and np.array_equal(x.bias, y.bias)
            assert np.array_equal(x.rho, y.rho) and x.ld == y.ld
