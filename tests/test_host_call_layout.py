"""CPU: the layout helper of the per-call entries (csrc/host_pack.hpp: CallLayout), compiled with g++ for the test only
(tests/host_call_layout_check.cpp).  Every entry of ctvio.hip names the segments of its scratch once and gets aligned offsets, a total and,
after the one reservation of the call, typed pointers.  The cases are the entries' segment lists at the smallest interesting sizes and the
degenerate ones (no queries, no selection with var_rho, nothing marginalised, a batch with no blocked window, a batch of only blocked ones).
The shim also reads out the LDS layouts of the two tile Cholesky kernels (csrc/device_types.hpp: CholTilesLds, CholFlowLds).
Beside it the host-only parts the query entries share: the order of the queries by window and its cut into tiles (QueryOrder), the
device-only scratch (CovScratch) and the status merge and fill (merge_status, fill_not_ok, cov_block, gate_value).
The same file is also built as a stand-alone program under AddressSanitizer + UBSan, which fills every segment of every case through its
pointer over buffers of exactly the reserved sizes and runs the order and fill cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INC = "/opt/rocm/include"
SRC = os.path.join(HERE, "host_call_layout_check.cpp")
HDRS = [os.path.join(HERE, "..", "ctrl-vio_amd", "csrc", f) for f in ("host_pack.hpp", "device_types.hpp")] + [os.path.join(HERE, "..", "include", "ctvio.h")]
LINK = ["-pthread"]   # (nothing here calls a HIP function: the helper is host-only arithmetic)


def _build(out, flags):
    if not os.path.isdir(ROCM_INC):
        pytest.skip("HIP headers not found")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", ROCM_INC] + flags + ["-o", out, SRC] + LINK)
    return out


@pytest.fixture(scope="module")
def cl():
    lib = C.CDLL(_build(os.path.join(HERE, "_build", "libhostcalllayout.so"), ["-fPIC", "-shared"]))
    lib.cl_case_name.restype = C.c_char_p
    lib.cl_layout.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.cl_chol_lds.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
    return lib


def layout(cl, c, which):
    """-> ([(name, offset, bytes, dbl)], total, device total, segments of the head)"""
    cap = 64
    name = (C.c_char_p * cap)(); off = np.zeros(cap, np.uint64); nb = np.zeros(cap, np.uint64); dbl = np.zeros(cap, np.int32); tot = np.zeros(3, np.uint64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    n = cl.cl_layout(c, which, cap, C.cast(name, C.c_void_p), p(off), p(nb), p(dbl), p(tot))
    assert 0 <= n <= cap
    return [(name[i].decode(), int(off[i]), int(nb[i]), int(dbl[i])) for i in range(n)], int(tot[0]), int(tot[1]), int(tot[2])


NAMES = ["head_only", "head_241", "linearize_tiny", "linearize_cost_only", "lm_step", "residual_summary", "gauge_two_windows", "query_none",
         "query_97_pose", "query_batch_5", "cov_tiny_20", "cov_no_selection_var_rho", "cov_nothing", "marg_no_blocked", "marg_only_blocked",
         "marg_mixed", "mb_window_268_553", "mb_window_m0", "query_scr_0", "query_scr_0_cov", "query_scr_5", "query_scr_5_cov"]


def test_the_cases_are_the_listed_ones(cl):
    assert [cl.cl_case_name(c).decode() for c in range(cl.cl_ncases())] == NAMES


@pytest.mark.parametrize("which", [0, 1], ids=["io", "scr"])
@pytest.mark.parametrize("case", NAMES)
def test_layout_rules(cl, case, which):
    c = NAMES.index(case)
    segs, total, dev_total, nhead = layout(cl, c, which)
    up = lambda b: (b + 255) // 256 * 256
    end = 0
    for name, off, nb, _ in segs:
        assert off % 256 == 0, name
        assert off == end, name                      # declaration order, no gap beyond the alignment tail, no overlap
        end = off + up(nb)                           # (a segment without elements costs nothing: the next one starts at its offset)
    assert total == end                              # the total is the last segment's aligned end
    assert dev_total % 256 == 0 and dev_total <= total
    if which == 0:
        assert nhead == 3 and [s[0] for s in segs[:3]] == ["lm", "poll", "state"]
        assert segs[1][2] == 16 and segs[1][1] >= segs[0][1] + segs[0][2]       # the poll words: a segment of their own behind the records
        landing = [s for s in segs if s[1] >= dev_total and s[2]]
        assert all(not s[3] for s in landing)         # host-only landing areas are never poisoned: there is nothing on the device
        assert (dev_total < total) == bool(landing)
    else:
        assert dev_total == total
    # a pointer before the reservation, or growing after it, is refused; pointers after it are base + offset
    assert cl.cl_refusals(c, which) == 0
    assert cl.cl_fill_and_read(c, which) == 0


def test_degenerate_cases_cost_what_they_should(cl):
    by = lambda case, which: {i: s for i, s in enumerate(layout(cl, NAMES.index(case), which)[0])}
    q = by("query_none", 0)
    assert [q[i][2] for i in range(3, 10)] == [0, 0, 16, 0, 0, 0, 0] and q[5][1] == q[3][1]          # only the error word
    cv_ = by("cov_no_selection_var_rho", 0)
    assert [cv_[i][2] for i in range(3, 8)] == [0, 24, 0, 0, 96]
    assert layout(cl, NAMES.index("cov_no_selection_var_rho"), 1)[0][2][2] == 0                       # no Y
    m = layout(cl, NAMES.index("marg_no_blocked"), 1)[0]
    assert [s[2] for s in m[6:12]] == [115 * 115 * 8, 0, 0, 0, m[10][2], 40 * 8] and m[12][2] == 0 and m[13][2] == 0   # m = 0; no blocked scratch
    assert m[7][1] == m[8][1] == m[9][1] == m[10][1]
    b = layout(cl, NAMES.index("marg_only_blocked"), 1)
    assert [s[0] for s in b[0]] == ["mb", "rank"] and b[0][0][2] == layout(cl, NAMES.index("mb_window_268_553"), 1)[1]


def test_query_scratch_costs_nothing_without_covariances(cl):
    """host_pack.hpp: CovScratch, the one device-only layout of the query entries (mask | excl | records)."""
    for case in ("query_scr_0", "query_scr_5"):
        segs, total, _, _ = layout(cl, NAMES.index(case), 1)
        assert [s[0] for s in segs] == ["mask", "excl", "records"] and [s[2] for s in segs] == [0, 0, 0] and total == 0
    segs, total, _, _ = layout(cl, NAMES.index("query_scr_5_cov"), 1)
    assert [s[2] for s in segs] == [115, 115, 5 * 1184] and [s[3] for s in segs] == [0, 0, 0] and total == 256 + 256 + 6144
    assert [s[2] for s in layout(cl, NAMES.index("query_scr_0_cov"), 1)[0]] == [115, 115, 0]


ORDER_WIN = [2, 0, 2, 1, 2, 2, 2, 2, 2, 2, 2]
ORDER_CASES = [("none", -1, [], 2), ("one", -1, [1], 8), ("single_window", 1, None, 2)] + [("mixed_%d" % p, -1, ORDER_WIN, p) for p in (1, 2, 8)]


@pytest.mark.parametrize("name,only,win,per_tile", ORDER_CASES, ids=[c[0] for c in ORDER_CASES])
def test_query_order(cl, name, only, win, per_tile):
    """host_pack.hpp: QueryOrder -- the stable order by window of the query entries and its cut into tiles of at most per_tile queries of
    one window (1: nav_state / body_rates / imu_predict, 2: pose_covariance / relative_pose, 8: project_landmarks)."""
    n = 5 if win is None else len(win)
    w = None if win is None else np.asarray(win, np.int32)
    wins = np.full(n, only, np.int32) if win is None else w
    slot = np.full(max(n, 1), -7, np.int32); tile = np.zeros(3 * 16, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    nt = cl.cl_query_order(only, n, None if w is None or n == 0 else p(w), 3, per_tile, p(slot), 16, p(tile))
    assert 0 <= nt <= 16
    assert slot[:n].tolist() == np.argsort(wins, kind="stable").tolist()               # the stable order
    tiles = tile[:3 * nt].reshape(nt, 3)
    nxt = 0
    for tw, first, cnt in tiles.tolist():
        assert first == nxt and 1 <= cnt <= per_tile                                    # a partition of [0, n), in order
        assert set(wins[slot[first:first + cnt]].tolist()) == {tw}                      # one window per tile
        nxt = first + cnt
    assert nxt == n
    if name.startswith("mixed"):
        # window 0 and window 1: one query each; window 2: nine -- runs that end at the window boundary, more than 8 in one window
        assert tiles[:2].tolist() == [[0, 0, 1], [1, 1, 1]]
        assert tiles[2:, 2].tolist() == {1: [1] * 9, 2: [2, 2, 2, 2, 1], 8: [8, 1]}[per_tile] and set(tiles[2:, 0].tolist()) == {2}


def test_query_order_refuses_a_window_out_of_range(cl):
    w = np.asarray([0, 3, -1], np.int32); buf = np.zeros(48, np.int32)
    assert cl.cl_query_order(-1, 3, w.ctypes.data_as(C.c_void_p), 3, 2, buf.ctypes.data_as(C.c_void_p), 16, buf.ctypes.data_as(C.c_void_p)) == -1
    assert cl.cl_order_cases() == 0        # the same cases in C++ (the sanitizer program runs these), with the message of the refusal


@pytest.mark.parametrize("dim", [2, 3, 6, 15])
def test_status_fill(cl, dim):
    """host_pack.hpp: fill_not_ok -- the block of a query that is not OK: no information (2) +inf on the diagonal and 0 elsewhere, else NaN."""
    for st in (1, 2, 3):
        o = np.full(dim * dim + 1, -1.0)
        cl.cl_fill_not_ok(o.ctypes.data_as(C.c_void_p), dim, st)
        want = np.diag(np.full(dim, np.inf)) if st == 2 else np.full((dim, dim), np.nan)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(o[:-1].reshape(dim, dim), want, equal_nan=True) and o[-1] == -1.0
    assert cl.cl_fill_cases() == 0         # cov_block, merge_status and gate_value beside it (the sanitizer program runs these too)


@pytest.mark.parametrize("flow", [0, 1], ids=["barrier", "flow"])
@pytest.mark.parametrize("ntr", range(1, 15))
def test_tile_cholesky_lds_layout(cl, flow, ntr):
    """device_types.hpp: CholTilesLds / CholFlowLds, the LDS of k_cholesky_tiles / k_cholesky_flow for every tile-row count a window with
    P <= 223 can have.  The launch bytes are the values the launch plan computed before the layout was stated (they decide how many
    workgroups share a CU, so they must not move)."""
    name = (C.c_char_p * 8)(); off = np.zeros(8, np.uint64); nb = np.zeros(8, np.uint64); tot = np.zeros(1, np.uint64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    n = cl.cl_chol_lds(flow, ntr, C.cast(name, C.c_void_p), p(off), p(nb), p(tot))
    segs = [(name[i].decode(), int(off[i]), int(nb[i])) for i in range(n)]
    assert [s[0] for s in segs] == (["Id", "Li", "Ls", "Pn", "tv", "xs", "flags"] if flow else ["Id", "Li", "Pn", "tv", "xs", "flags", "park"])
    end = 0
    for nm, o, b in segs:
        assert o >= end and b > 0, nm                # in order, disjoint
        end = o + b
    assert end <= int(tot[0])
    assert all(o % 8 == 0 for nm, o, _ in segs if nm in ("flags", "park"))
    recorded = (272 + 5 * ntr * 272 + 32 * ntr + 48) * 8 if flow else (272 + 2 * ntr * 272 + 32 * ntr + 4 + 768) * 8
    assert int(tot[0]) == recorded
    if ntr == 14:
        assert int(tot[0]) <= 160 * 1024


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The helper over real std::vector-backed bases, as a program of its own with AddressSanitizer + UBSan linked in."""
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not installed")
    exe = _build(str(tmp_path / "call_layout_asan"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCALL_LAYOUT_MAIN"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1"))
    assert p.returncode == 0 and "CALL_LAYOUT_OK %d cases" % len(NAMES) in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
