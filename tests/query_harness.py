"""What the GPU tests of the query entries (tests/test_gpu_<entry>.py) and of the adaptor demos share: the device references, the solved
window behind the per-file `config1_solved` fixtures, the bit comparisons of a batch call against its other call forms, the "the call leaves
the solve alone" sequence, the tail of the refusal tests, and building / running / reading back an adaptor demo (tests/*_demo.cpp).

A plain module: the test files import it after their `sys.path.insert(0, HERE)`.  What differs between the entries is an argument here or
stays in the test file: the per-entry calls and their assertions come in as callables."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# The bit-for-bit comparisons need a linearisation that is itself repeatable: by default a batch with a window beyond the LDS-resident Hessian
# (the P = 301 and K = 27 windows of test_gpu_covariance.mixed_batch) assembles its normal equations with floating-point atomics, and two runs
# differ at 1e-13 before any kernel of the covariance starts.  deterministic = 2 fixes the order for every batch.
DET = dict(deterministic=2)
STATE_ARRAYS = ("quat", "pos", "bias", "rho")


def device_reference(s, wid, w):
    """cov_reference over all P unknowns of window wid on the device's own linearisation at its current state."""
    import cov_helpers as ch
    H, W, Hll, _, _ = s.linearize(wid)
    return ch.cov_reference(H, W, Hll, ~ch.constant_mask(w), range(w.P))


def device_joint_reference(s, wid, w):
    """lmpoint_helpers.joint_reference of window wid on the device's own linearisation at its current state."""
    import cov_helpers as ch
    import lmpoint_helpers as lh
    H, W, Hll, _, _ = s.linearize(wid)
    return lh.joint_reference(H, W, Hll, ~ch.constant_mask(w))


def solved_window(cv, cfg, seed, iters):
    """Generator behind the module fixtures: yields (solver, the window at the solved state) once, on an open handle, after an iters-iteration
    solve of synth window (cfg, seed); the handle closes when the fixture is torn down."""
    w = cv.synth.make_window(cfg, seed=seed)
    with cv.Solver() as s:
        b = [w.copy()]
        s.set_windows(b)
        s.solve(iters)
        yield s, b[0]


def same_bits(a, b, fields=None):
    """Bitwise equality (NaN == NaN) of two results: arrays, None, tuples / lists of results, or -- with fields -- the named attributes of two
    namespaces."""
    if fields is not None:
        return all(same_bits(getattr(a, f), getattr(b, f)) for f in fields)
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b, equal_nan=True)


def check_batch_bits(single, batch, win, columns, out, n_windows):
    """The bits of a query depend on its window and its own columns alone.  out = batch(win, *columns), a tuple of per-query arrays, computed on
    another handle; single(i, *columns of window i) and batch are the entry's two calls on the handle under test.  Compared with out: the
    single-window entry per window, a second call, the reversed order, and calls with 1 / 2 / the outer 2 of the 3 queries per window (the
    queries come window-interleaved, three per window: other tile partners)."""
    for i in range(n_windows):
        idx = np.nonzero(win == i)[0]
        assert same_bits(tuple(single(i, *(c[idx] for c in columns))), tuple(o[idx] for o in out)), i
    assert same_bits(tuple(batch(win, *columns)), tuple(out))
    rev = batch(win[::-1].copy(), *(c[::-1].copy() for c in columns))
    assert same_bits(tuple(o[::-1] for o in rev), tuple(out))
    n = n_windows
    for keep in (np.arange(n), np.arange(2 * n), np.r_[np.arange(n), np.arange(2 * n, 3 * n)]):
        assert same_bits(tuple(batch(win[keep].copy(), *(c[keep].copy() for c in columns))), tuple(o[keep] for o in out)), keep


def check_leaves_the_solve_alone(cv, ws, calls, sels=None, solver_kw=DET, compare_ld=True, then=None):
    """State bits, graph captures and a following solve are unchanged by the entry's calls.  On a handle that has solved ws for 6 iterations
    without write-back, calls(s, b) makes the entry's calls and asserts what is the entry's own (finite outputs, the timing slots, values-only
    bits); b are the handle's windows.  Around it: with sels, ctvio_covariance_batch gives identical bits before and after; the graph captures
    and the batch state are unchanged; then(s, b, what calls returned), if given, runs the entry's cross-checks that need a write-back; 6 more
    iterations give the summaries and the state (STATE_ARRAYS, and ld with compare_ld) of a fresh handle that made no call in between."""
    with cv.Solver(**solver_kw) as s:
        b = [w.copy() for w in ws]
        s.set_windows(b)
        s.solve(6, writeback=False)
        cap, state = s.graph_captures, s.get_batch_state()
        before = s.covariance_batch(sels, rho=True) if sels is not None else None
        got = calls(s, b)
        if sels is not None:
            assert same_bits(s.covariance_batch(sels, rho=True), before)
        assert s.graph_captures == cap
        assert all(np.array_equal(x, y) for x, y in zip(state, s.get_batch_state()))
        if then is not None:
            then(s, b, got)
        sm = s.solve(6)
        assert s.graph_captures == cap
    with cv.Solver(**solver_kw) as f:
        fb = [w.copy() for w in ws]
        f.set_windows(fb)
        f.solve(6, writeback=False)
        smf = f.solve(6)
    assert sm == smf
    for x, y in zip(b, fb):
        for a in STATE_ARRAYS:
            assert np.array_equal(getattr(x, a), getattr(y, a)), a
        if compare_ld:
            assert x.ld == y.ld


def check_usable_after(cv, w, s):
    """The tail of the refusal tests: after the refused calls, handle s solves w like a fresh handle."""
    b = [w.copy()]
    s.set_windows(b)
    sm = s.solve(15)[0]
    with cv.Solver() as f:
        fb = [w.copy()]
        f.set_windows(fb)
        assert f.solve(15)[0] == sm
    assert np.array_equal(b[0].pos, fb[0].pos) and np.array_equal(b[0].quat, fb[0].quat)


def _dump(w, path):
    """The text dump of a window that tests/demo_window.hpp reads."""
    with open(path, "w") as f:
        p = lambda *a: f.write(" ".join(repr(float(x)) if isinstance(x, (float, np.floating)) else str(int(x)) for x in a) + "\n")
        p(w.K, w.F, w.L, w.M, w.NB, w.V, w.pn, len(w.p_kind), w.t0_ns, w.dt_ns)
        for k in range(w.K):
            p(*w.quat[k].tolist(), *w.pos[k].tolist())
        for fr in range(w.F):
            p(*w.bias[fr].tolist())
        for l in range(w.L):
            p(float(w.rho[l]))
        p(float(w.ld), float(w.ld_lo), float(w.ld_hi), int(w.fix_ld))
        p(*w.q_CI.tolist()); p(*w.p_CI.tolist()); p(*w.gravity.tolist()); p(*w.imu_w.tolist()); p(float(w.img_w))
        if w.pn:
            p(*np.asfortranarray(w.pJ0).ravel(order="F").tolist())
            p(*w.pr0.tolist())
            for b in range(len(w.p_kind)):
                f.write(f"{int(w.p_kind[b])} {int(w.p_index[b])} {int(w.p_off[b])} " + " ".join(repr(float(x)) for x in w.p_x0[b]) + "\n")
        for m in range(w.M):
            f.write(f"{int(w.imu_t[m])} " + " ".join(repr(float(x)) for x in (*w.imu_gyro[m], *w.imu_acc[m])) + f" {int(w.imu_bias[m])}\n")
        for b in range(w.NB):
            f.write(f"{int(w.bc_i[b])} {int(w.bc_j[b])} " + " ".join(repr(float(x)) for x in w.bc_w[b]) + "\n")
        for v in range(w.V):
            f.write(f"{int(w.v_lm[v])} {int(w.v_ti[v])} {int(w.v_tj[v])} {int(w.v_rowi[v])} {int(w.v_rowj[v])} "
                    + " ".join(repr(float(x)) for x in (*w.v_pi[v], *w.v_pj[v])) + "\n")


def build_demo(name, tmp_path):
    """Compiles tests/<name>.cpp against include/ and the built libctvio.so; returns the path of the program."""
    exe = str(tmp_path / name)
    lib = os.path.join(ROOT, "ctrl-vio_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, name + ".cpp"),
                           "-L", lib, "-lctvio", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def read_state(w0, arr):
    """arr: the numbers DemoWindow::write_state wrote for a window shaped like w0, and what follows.  Returns (w0 at that state, what follows
    the line `iterations final_cost`)."""
    K, F, L = w0.K, w0.F, w0.L
    kn = arr[:7 * K].reshape(K, 7)
    wa = w0.copy()
    wa.quat, wa.pos = kn[:, :4].copy(), kn[:, 4:].copy()
    wa.bias = arr[7 * K:7 * K + 6 * F].reshape(F, 6).copy()
    wa.rho = arr[7 * K + 6 * F:7 * K + 6 * F + L].copy()
    wa.ld = float(arr[7 * K + 6 * F + L])
    return wa, arr[7 * K + 6 * F + L + 3:]


def run_demo(exe, w0, tmp_path, *args, state=True):
    """Dumps w0 to in.txt and runs `exe in.txt out.txt *args`.  Returns (the window at the demo's solved state, the rest of out.txt as an
    array); for a demo that writes no state (state=False): (None, all of out.txt)."""
    _dump(w0, str(tmp_path / "in.txt"))
    subprocess.run([exe, str(tmp_path / "in.txt"), str(tmp_path / "out.txt")] + [str(a) for a in args], check=True, timeout=120)
    arr = np.array(open(tmp_path / "out.txt").read().split(), float)
    return read_state(w0, arr) if state else (None, arr)
