"""GPU (-m gpu): a reused solver handle gives the answers of a fresh one.

The first upload into a fresh handle grows its work arena and clears all of it; later uploads clear only the per-upload zero region
(ctvio.hip: pack_and_upload, [o_zero0, o_zero1)).  Everything else -- Hpp, S, rhs, the Cholesky inverses, the IMU tiles, the
marginalisation scratch, the query outputs -- holds the previous call's numbers in another layout.  A kernel that reads an entry it
never wrote is right only if a select masks it: a product with zero hides the defect on a fresh handle (0 * 0) and not on a reused one
(0 * NaN, 0 * 1e151).

CTVIO_POISON=1 / 2 (read once, in ctvio_create) makes every upload and every call start that reused double scratch as a quiet NaN /
as 2.6e151, and makes the upload check that the packer writes every staged input byte.  (a) a poisoned handle equals an unpoisoned one
on every device path; (b) one handle driven through a sequence of batches that shrinks, grows and reallocates its arenas equals a
fresh handle at every step; (c) the C++ adaptor (one cached handle per thread for solve, query, marginalisation and summary) writes the
same bytes with and without the switch.  Bitwise wherever the batch runs in the deterministic mode (the handle is created with
deterministic = 1, which refuses a batch it cannot honour), otherwise to the tolerance of the path's own test with identical LM
decisions."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import marg_blocked_helpers as mb

pytestmark = pytest.mark.gpu



@contextlib.contextmanager
def _env(**kv):
    """CTVIO_* switches for the handles created inside (None: unset)."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------ batches (the builders of the path tests)

def _ragged7(cv):
    """test_flow_cholesky_equals_the_barrier_cholesky's seven windows: tiny (4 tile rows), config 1 with fixed unknowns / a fixed line delay,
    config 2 / 3 / tumrs (14 tile rows, the rhs row at different offsets), a prior-free tiny window."""
    base = [cv.synth.make_window("tiny", seed=41), cv.synth.make_window("config1", seed=1301), cv.synth.make_window("config2", seed=1002),
            cv.synth.make_window("config3", seed=1003), cv.synth.make_window("tumrs", seed=1004), cv.synth.make_window("tiny", seed=42, with_prior=False),
            cv.synth.make_window("config1", seed=1302)]
    base[1].fixed_upto = 2
    base[6].fix_ld = True
    base[6].lock_bg = True
    return base


# (frames, knot spacing in ms): test_flow_cholesky_every_tile_count_and_rhs_offset's 26 sizes, P from 43 to 223
_SIZES = [(2, 75), (2, 50), (2, 40), (3, 60), (3, 50), (3, 40), (4, 60), (4, 50), (6, 100), (4, 40), (5, 50), (6, 60), (5, 40), (6, 50), (7, 60),
          (6, 40), (8, 60), (11, 100), (7, 40), (11, 75), (9, 50), (8, 40), (10, 50), (9, 40), (11, 50), (10, 40)]


def _sizes26(cv):
    return [cv.synth.make_window("config1", seed=1700 + i, F=F, dt_ns=dt * 1_000_000, L=30, M=40 * F) for i, (F, dt) in enumerate(_SIZES)]


def _prior_batch(cv):
    """tests/test_gpu_prior.py's dense-prior batch (every block kind, shuffled offsets, constant blocks, priors over every pose unknown)."""
    import test_gpu_prior as tp
    return tp._ragged_batch(cv), tp._band_window(cv)


def _query_window(cv, seed=5):
    """The shape of Trajectory::QueryNs (include/ctvio_estimator.hpp): one bias state, no factors, fixed line delay."""
    rng = np.random.default_rng(seed)
    K = 9
    q = rng.normal(size=(K, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return cv.Window(t0_ns=1_000_000_123, dt_ns=50_000_000, quat=q, pos=rng.normal(size=(K, 3)), bias=np.zeros((1, 6)), rho=np.zeros(0),
                     fix_ld=True).normalize()


def _slide_marg():
    import slide_helpers as sh
    world = sh.make_world()
    st = sh.State(world)
    w, info = sh.window_of(world, st, 0, sh.initial_prior(world))
    return sh.marg_window_of(world, st, 0, w, info)


def _c5_marg():
    w = mb.config5_window(1500)
    return w, mb.drop_roles(w, [0, 1])


# ------------------------------------------------------------------------------------------------ what a handle computes

def _solver(cv, det):
    return cv.Solver() if det is None else cv.Solver(deterministic=det)


def _run_windows(cv, s, ws, lin_ids=(0,), steps=True, iters=8):
    """Outputs of one batch on handle s: linearize / cost / residual_summary of lin_ids, lm_step of every window, then the solve."""
    batch = [w.copy() for w in ws]
    s.set_windows(batch)
    out = {"lin": [s.linearize(i) for i in lin_ids], "cost": [s.cost(i) for i in lin_ids],
           "rs": [s.residual_summary(i) for i in lin_ids]}
    if steps:
        out["step"] = [s.lm_step(i, 1e4) for i in range(len(batch))]
    if iters:
        out["solve"] = s.solve(iters)
        out["state"] = _per_window(batch, s.get_batch_state())
    return out


def _per_window(ws, st):
    """get_batch_state split into the windows (quat, pos, bias, rho, ld per window)."""
    q, p, b, r, ld = st
    out, k, f, l = [], 0, 0, 0
    for i, w in enumerate(ws):
        out.append((q[k:k + w.K], p[k:k + w.K], b[f:f + w.F], r[l:l + w.L], ld[i]))
        k += w.K; f += w.F; l += w.L
    return out


def _run_steps(cv, s, ws):
    s.set_windows([w.copy() for w in ws])
    return {"step": [s.lm_step(i, 1e4) for i in range(len(ws))]}


def _run_queries(cv, s, ws):
    """spline_eval / spline_eval_batch / sensor_pose / gauge_restore on test_spline_eval_batch_all_windows_one_launch's batch."""
    s.set_windows([w.copy() for w in ws])
    rng = np.random.default_rng(4)
    win = rng.integers(0, len(ws), 4000).astype(np.int32)
    t = np.array([rng.integers(ws[i].t0_ns, ws[i].max_time_ns()) for i in win], np.int64)
    out = {"batch": s.spline_eval_batch(win, t, want=("pose", "vel", "omega", "acc"))[0]}
    out["one"] = [s.spline_eval(i, t[win == i]) for i in range(len(ws))]
    out["sensor"] = s.sensor_pose(1, t[win == 1], np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9]), np.array([0.05, 0.0, -0.02]))
    s.gauge_restore([0, 2], [2, 5], np.stack([ws[0].quat[2], ws[2].quat[5]]), np.stack([ws[0].pos[2], ws[2].pos[5] + 0.3]))
    out["state"] = s.get_batch_state()
    return out


def _run_marg(cv, s, ws, roles, single=None, form=False):
    """form: the prior as its quadratic form (kept, J0^T J0, J0^T r0, rank) -- for windows whose normal equations are assembled with
    atomics (K > 25), where run-to-run rounding rotates the eigenvectors of near-equal eigenvalues inside J0."""
    s.set_windows([w.copy() for w in ws])
    out = {"marg": s.marginalize_batch(roles)}
    if form:
        out["marg"] = [(k, J.T @ J, J.T @ r, np.linalg.matrix_rank(J)) for k, J, r in out["marg"]]
    if single is not None:
        out["single"] = s.marginalize(single, roles[single])
        out["host"] = s.marginalize_ran_on_host()
    return out


def _cov_windows(cv):
    """`tiny` (P = 103) and `config1` (P = 211) with selections of 20 and 17 unknowns, none of them on the two newest knots (an
    unknown that no factor touches has an infinite variance, and the comparison asks for finite numbers)."""
    ws = [cv.synth.make_window("tiny", seed=7), cv.synth.make_window("config1", seed=1000)]
    rng = np.random.default_rng(11)
    sels = [[int(x) for x in rng.permutation(np.r_[0:6 * (w.K - 2), 6 * w.K:w.P])[:n]] for w, n in zip(ws, (20, 17))]
    return ws, sels


def _run_cov(cv, s, ws, sels):
    """covariance_batch with the landmark variances, then the single-window entry alone."""
    s.set_windows([w.copy() for w in ws])
    covs, var, sing = s.covariance_batch(sels, rho=True)
    return {"cov": covs, "var": var, "singular": sing, "one": s.covariance(1, sels[1], rho=True)}


def _spline_windows(cv):
    ws = [cv.synth.make_window("tiny", seed=21), cv.synth.make_window("config1", seed=1004), cv.synth.make_window("config3", seed=1005)]
    ws[1].t0_ns = 1_000_000_007
    ws[1].imu_t = ws[1].imu_t + 1_000_000_007
    ws[1].v_ti = ws[1].v_ti + 1_000_000_007
    ws[1].v_tj = ws[1].v_tj + 1_000_000_007
    return ws


# ------------------------------------------------------------------------------------------------ comparison

def _leaves(x, path=""):
    """(path, value) of every number / array in a nested output."""
    if isinstance(x, dict):
        for k in sorted(x):
            yield from _leaves(x[k], f"{path}.{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _leaves(v, f"{path}[{i}]")
    else:
        yield path, x


# summary fields that are LM decisions (equal on every path) and the floating-point ones (bitwise or to the tolerance)
_DECISIONS = ("iterations", "num_successful", "num_unsuccessful", "termination", "num_line_search_steps", "num_line_search_reduced")


def assert_same(a, b, tol=None, skip=(), what=""):
    """tol None: bitwise.  Otherwise every array within tol of its largest entry, every scalar within rel tol, LM decisions and the
    validity of every step identical.  Finite everywhere (a step's model change of -1 marks an invalid step).  skip: window indices
    whose floating-point results are not compared under a tolerance (noise amplifiers), decisions still are."""
    la, lb = list(_leaves(a)), list(_leaves(b))
    assert [p for p, _ in la] == [p for p, _ in lb], what
    for (p, x), (_, y) in zip(la, lb):
        if isinstance(x, (bool, np.bool_, str)) or x is None:
            assert x == y, (what, p, x, y)
            continue
        xa, ya = np.asarray(x), np.asarray(y)
        assert xa.shape == ya.shape, (what, p)
        if xa.dtype.kind in "iu" or p.split(".")[-1] in _DECISIONS:
            assert np.array_equal(xa, ya), (what, p, x, y)
            continue
        assert np.isfinite(xa).all() and np.isfinite(ya).all(), (what, p, "non-finite")
        t = tol
        if p.startswith(".rs"):     # (k_residual_summary sums with LDS atomics: its last bits are not fixed in any mode)
            t = max(t or 0.0, 1e-13)
        if t is None:
            assert np.array_equal(xa, ya), (what, p, np.abs(xa - ya).max())
            continue
        if p.startswith(".step[") and p.endswith("[1]"):      # model change: step validity is a decision
            assert (xa == -1.0) == (ya == -1.0), (what, p, x, y)
        if p.startswith((".step[", ".solve[", ".state[")) and int(p.split("[")[1].split("]")[0]) in skip:
            continue
        scale = max(np.abs(xa).max(initial=0.0), np.abs(ya).max(initial=0.0), 1e-300)
        assert np.abs(xa - ya).max(initial=0.0) <= t * scale, (what, p, np.abs(xa - ya).max(initial=0.0) / scale)


# ------------------------------------------------------------------------------------------------ (a) poison changes nothing

_TABLE = {}


def _case_table(cv):
    """name -> (env, deterministic, runner(s), tolerance, skip)."""
    if not _TABLE:
        _TABLE.update(_build_table(cv))
    return _TABLE


def _build_table(cv):
    r7 = _ragged7(cv)
    r200 = [r7[i % 7] for i in range(200)]
    c1 = [cv.synth.make_window("config1", seed=1600 + i, F=16, L=60, M=750) for i in range(4)]
    c5 = [cv.synth.make_window("config5", seed=1011)]
    pb, band = _prior_batch(cv)
    tiny = cv.synth.make_window("tiny", seed=11)
    big = cv.synth.make_window("config1", seed=1200, F=10, dt_ns=40_000_000, with_prior=False)
    mixed = [tiny, cv.Solver.predict_window(big, fixed_upto=-1)]
    sw = _spline_windows(cv)
    sm, srole = _slide_marg()
    c5m, c5role = _c5_marg()
    cw, csel = _cov_windows(cv)
    W = _run_windows
    return {
        "ragged7": ({}, 1, lambda s: W(cv, s, r7, lin_ids=range(7)), None, ()),
        "ragged7_n200": ({}, None, lambda s: W(cv, s, r200, lin_ids=(0, 2, 199)), 1e-7, set(range(5, 200, 7))),
        "ragged7_chol0": ({"CTVIO_CHOL_TILES": 0}, 1, lambda s: W(cv, s, r7, lin_ids=(1, 4)), None, ()),
        "ragged7_chol1": ({"CTVIO_CHOL_TILES": 1}, 1, lambda s: W(cv, s, r7, lin_ids=(1, 4)), None, ()),
        "sizes26": ({}, None, lambda s: _run_steps(cv, s, _sizes26(cv)), 1e-9, ()),
        "p301": ({}, None, lambda s: W(cv, s, c1, lin_ids=(0, 3)), 1e-7, ()),
        "p301_tile2": ({"CTVIO_SCHUR_TILE2": 1}, None, lambda s: W(cv, s, c1, lin_ids=(0, 3)), 1e-7, ()),
        "config5": ({}, None, lambda s: W(cv, s, c5, iters=4), 1e-7, ()),
        "prior_merged_store": ({}, 1, lambda s: W(cv, s, pb, lin_ids=range(len(pb))), None, ()),
        "prior_split_store": ({"CTVIO_SPLIT_LINEARIZE": 1}, 1, lambda s: W(cv, s, pb, lin_ids=range(len(pb))), None, ()),
        "prior_accumulate": ({}, 0, lambda s: W(cv, s, pb, lin_ids=(0, 4, 11)), 1e-9, ()),
        "prior_accumulate_band": ({}, 0, lambda s: W(cv, s, pb + [band], lin_ids=(4, 12)), 1e-9, ()),
        "imu_only_mixed": ({}, None, lambda s: W(cv, s, mixed, lin_ids=(0, 1)), 1e-8, ()),
        "queries": ({}, None, lambda s: _run_queries(cv, s, sw), None, ()),
        "marg_lds": ({}, None, lambda s: _run_marg(cv, s, [sm] * 3, [srole] * 3, single=1), None, ()),
        "marg_blocked": ({"CTVIO_MARG_BLOCKED": 1}, None, lambda s: _run_marg(cv, s, [sm] * 2, [srole] * 2), None, ()),
        "marg_c5_blocked": ({}, None, lambda s: _run_marg(cv, s, [c5m], [c5role], form=True), 1e-7, ()),
        "marg_host": ({"CTVIO_MARG_HOST": 1}, None, lambda s: _run_marg(cv, s, [sm], [srole], single=0), None, ()),
        "covariance": ({}, 1, lambda s: _run_cov(cv, s, cw, csel), None, ()),
    }


_REF = {}


def _run_case(cv, name, poison):
    env, det, run, _, _ = _case_table(cv)[name]
    with _env(CTVIO_POISON=poison, **env):
        s = _solver(cv, det)
    try:
        return run(s)
    finally:
        s.close()


CASES = ["ragged7", "ragged7_n200", "ragged7_chol0", "ragged7_chol1", "sizes26", "p301", "p301_tile2", "config5", "prior_merged_store",
         "prior_split_store", "prior_accumulate", "prior_accumulate_band", "imu_only_mixed", "queries", "marg_lds", "marg_blocked",
         "marg_c5_blocked", "marg_host", "covariance"]


@pytest.mark.parametrize("pattern", [1, 2])
@pytest.mark.parametrize("case", CASES)
def test_poison_changes_nothing(cv, case, pattern):
    _, _, _, tol, skip = _case_table(cv)[case]
    if case not in _REF:
        _REF[case] = _run_case(cv, case, None)
    got = _run_case(cv, case, pattern)
    assert_same(got, _REF[case], tol, skip, f"{case} poison {pattern}")
    if case == "marg_host":
        assert got["host"] is True


# ------------------------------------------------------------------------------------------------ (b) history does not matter

def test_history_does_not_matter(cv):
    """One handle, one sequence of batches that shrinks and grows both arenas and reallocates them; every step equals the same batch on a fresh
    handle, and the three runs of the seven-window batch are bitwise equal to each other.  The batch of 241 windows outgrows the pinned result
    areas reserved under the 200-window batch (the head of the per-call arena: one record per window, the poll words in a segment of their
    own, the batch state; an eighth of headroom): the records of all its windows come back intact, and the arenas grow under it, so the
    cached hipGraph of the LM pass must be captured again, not replayed with stale pointers.  Every per-call entry lays its scratch out in
    the same two arenas, so the covariance and the queries that follow the config-5 marginalisation run over its numbers in another layout."""
    r7 = _ragged7(cv)
    c2 = [cv.synth.make_window("config2", seed=1002 + i % 64) for i in range(241)]
    c5 = [cv.synth.make_window("config5", seed=1011)]
    tiny = [cv.synth.make_window("tiny", seed=7)]
    qw = _query_window(cv)
    c5m, c5role = _c5_marg()
    cw, csel = _cov_windows(cv)
    sw = _spline_windows(cv)
    tq = np.linspace(qw.t0_ns, qw.max_time_ns() - 1, 97).astype(np.int64)

    def query(s):
        s.set_windows([qw.copy()])
        return {"q": s.spline_eval(0, tq)}

    steps = [("c2x200", lambda s: _run_windows(cv, s, c2[:200], lin_ids=(0, 199), steps=False), 1e-7),
             ("tiny", lambda s: _run_windows(cv, s, tiny), None),
             ("config5", lambda s: _run_windows(cv, s, c5, iters=4), 1e-7),
             ("ragged7", lambda s: _run_windows(cv, s, r7, lin_ids=range(7)), None),
             ("query", query, None),
             ("marg_c5", lambda s: _run_marg(cv, s, [c5m], [c5role], form=True), 1e-7),
             ("covariance", lambda s: _run_cov(cv, s, cw, csel), None),
             ("queries", lambda s: _run_queries(cv, s, sw), None),
             ("ragged7", lambda s: _run_windows(cv, s, r7, lin_ids=range(7)), None),
             ("c2x241", lambda s: _run_windows(cv, s, c2, lin_ids=(0, 200, 240), steps=False), 1e-7),
             ("ragged7", lambda s: _run_windows(cv, s, r7, lin_ids=range(7)), None)]
    fresh = {}
    seven = []
    with cv.Solver() as s:
        for name, run, tol in steps:
            got = run(s)
            if name not in fresh:
                with cv.Solver() as f:
                    fresh[name] = run(f)
            assert_same(got, fresh[name], tol, (), f"step {name}")
            if name == "ragged7":
                seven.append(got)
            if name == "c2x241":
                assert s.n == 241
    assert len(seven) == 3
    assert_same(seven[1], seven[0], None, (), "ragged7 run 2")
    assert_same(seven[2], seven[0], None, (), "ragged7 run 3")


# ------------------------------------------------------------------------------------------------ (c) the adaptor under poison

def test_cpp_adaptor_under_poison(cv, tmp_path):
    """tests/slide_demo.cpp (the C++ adaptor: SolverCache keeps one handle per thread for every solve, Trajectory query, marginalisation and
    residual summary of the three slide windows) writes the same bytes with the switch off and with either pattern -- each run a fresh
    process under its own time limit."""
    import slide_helpers as sh
    import query_harness as qh
    exe = qh.build_demo("slide_demo", tmp_path)
    qh._dump(sh.make_world(), str(tmp_path / "world.txt"))
    outs = []
    for pattern in (None, 1, 2):
        env = {k: v for k, v in os.environ.items() if k != "CTVIO_POISON"}
        if pattern is not None:
            env["CTVIO_POISON"] = str(pattern)
        res = tmp_path / f"out_{pattern}.txt"
        p = subprocess.run(["timeout", "-k", "10", "300", exe, str(tmp_path / "world.txt"), str(res)], env=env, capture_output=True, text=True)
        assert p.returncode == 0, (pattern, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        outs.append(res.read_bytes())
    assert len(outs[0]) > 0
    assert outs[1] == outs[0], "pattern 1"
    assert outs[2] == outs[0], "pattern 2"
