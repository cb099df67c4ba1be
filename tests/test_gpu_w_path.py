"""GPU (-m gpu): the two kernels that produce and consume W -- the rows of W that k_vis_eval forms in LDS sweeps of NR landmarks (the row buffer
shares the 20 480-byte workgroup buffer with the staged block records), and the per-window Schur kernel's tiles, each multiplying only the
K-steps (4 sorted landmark rows) inside its row range -- against the oracle's dense normal equations and its dense solve of the un-eliminated system."""
import os
import re

import numpy as np
import pytest

from test_gpu_sparsity import _two_track_window

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ctrl-vio_amd", "csrc")


def _kernel_constants():
    """The constexpr ints the visual kernel lays its LDS out with, read from the sources it is compiled from."""
    ns = {}
    for name in ("device_types.hpp", "kernels_visual.hpp"):
        for k, expr in re.findall(r"constexpr int (\w+) = ([^;]+);", open(os.path.join(CSRC, name)).read()):
            try:
                ns[k] = int(eval(expr, {"__builtins__": {}}, dict(ns)))
            except Exception:
                pass
    return ns


def _wave_landmarks(w):
    """Landmarks per wave of 64 block slots (host_pack.hpp: a landmark's blocks are consecutive slots in landmark order and never straddle a
    group of 64: padding slots in front of it)."""
    cnt = np.bincount(w.v_lm, minlength=w.L)
    pos, per = 0, {}
    for c in cnt:
        if c == 0:
            continue
        if (pos & 63) + c > 64:
            pos = (pos + 63) & ~63
        per[pos >> 6] = per.get(pos >> 6, 0) + 1
        pos += int(c)
    return per


def _sweeps(cv, w):
    """W-row sweeps of the window's busiest wave, by the kernel's own arithmetic (kernels_visual.hpp: NR rows of RS = SPW + 3 doubles)."""
    c = _kernel_constants()
    klo, khi = cv.packer.landmark_spans(w)
    spw = 6 * int(max(1, (khi - klo + 1).max()))
    rows = (c["VIS_ROW_BYTES"] // 8 - 1) // (spw + 3)
    return max(-(-n // max(1, min(n, rows))) for n in _wave_landmarks(w).values()), c


def _assert_normal_equations(cv, oracle, w, tol=1e-10):
    H, g, cost = oracle.OracleWindow(w.copy()).build_normal()
    P = w.P
    sc = np.sqrt(np.maximum(np.diag(H), 1e-30))
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        Hg, Wg, Hllg, gg, costg = s.linearize(0)
    assert costg == pytest.approx(cost, rel=1e-12)
    assert np.abs((Hg - H[:P, :P]) / np.outer(sc[:P], sc[:P])).max() < tol
    assert np.abs((Wg - H[:P, P:]) / np.outer(sc[:P], sc[P:])).max() < tol
    assert np.abs(Hllg / np.diag(H)[P:] - 1).max() < tol
    assert np.abs((gg - g) / sc).max() < tol * np.abs(g / sc).max()


@pytest.mark.parametrize("split", ["0", "1"])
def test_w_rows_in_several_sweeps(cv, oracle, split, monkeypatch):
    """A window of two-block landmarks (32 to a wave) beside one landmark seen in every frame (its 24-knot span sets the LDS row width of the
    batch): the row buffer holds fewer rows than a wave has landmarks, so the W-row phase runs at least two sweeps -- counted from the
    kernel's own constants -- through the merged launch (k_linearize_f64) and through k_vis_eval itself (CTVIO_SPLIT_LINEARIZE=1).  H, g,
    W, Hll and the cost against the oracle's dense normal equations, 1e-10 relative as test_linearize_matches_oracle."""
    w = _two_track_window(cv, "config1", 1610, L=80, track=(3, 0, 1))
    n, c = _sweeps(cv, w)
    assert c["VIS_LDS_BYTES"] <= 20480 and c["VIS_ROW_BYTES"] + 64 * 16 == c["VIS_LDS_BYTES"]
    assert n >= 2, n
    monkeypatch.setenv("CTVIO_SPLIT_LINEARIZE", split)
    _assert_normal_equations(cv, oracle, w)


def _k4(cv):
    return cv.synth.make_window("config1", seed=1620, F=2, dt_ns=140_000_000, L=30, M=80)


def _k9(cv):
    return cv.synth.make_window("config1", seed=1621, F=4, dt_ns=60_000_000, L=30, M=160)


def _k24_fixed(cv):
    w = cv.synth.make_window("config1", seed=1622)
    w.fixed_upto = 1
    return w


def _two_track(cv):
    return _two_track_window(cv, "config1", 1623)


@pytest.mark.parametrize("make,K,tiles", [(_k4, 4, 6), (_k9, 9, 15), (_k24_fixed, 24, 55), (_two_track, 24, 55)],
                         ids=["K4_fewer_tiles_than_waves", "K9_two_tiles_per_wave", "K24_fixed_knot", "two_frame_and_every_frame_landmark"])
def test_schur_window_kstep_ranges(cv, oracle, make, K, tiles):
    """k_schur_window_f64 (200 copies: the per-window kernel runs from 192 windows on) deals the tiles with products to its eight waves and
    multiplies, per tile, only the K-steps (4 sorted landmark rows) whose rows reach both column tiles.  One LM step against the oracle's
    dense Cholesky of the un-eliminated system, tolerance as test_schur_step_equals_the_dense_solve: 6 tiles for 8 waves (K = 4: two waves
    without a tile), 15 tiles (K = 9: one or two per wave, the other slots empty), 55 tiles with the columns of a fixed knot inactive
    (K = 24), and a two-frame landmark beside an every-frame one (K-step ranges of one step and of every step)."""
    w = make(cv)
    assert w.K == K and w.P <= 223
    nk, ldt, nrow = (6 * K + 15) // 16, (w.P - 1) // 16, w.P // 16 + 1      # tiles with products: knot / line-delay columns, rows up to the rhs row
    cols = lambda r: min(r + 1, nk) + (1 if nk <= ldt <= r else 0)
    assert sum(cols(r) for r in range(nrow) if r < nk or r == ldt or r == w.P // 16) == tiles
    d_o, mc_o = oracle.OracleWindow(w.copy()).lm_step(1e4, use_schur=False)
    with cv.Solver() as s:
        s.set_windows([w.copy() for _ in range(200)])
        for wid in (0, 199):
            d_g, mc_g = s.lm_step(wid, 1e4)
            assert np.abs(d_g - d_o).max() <= 1e-8 * np.abs(d_o).max(), wid
            assert mc_g == pytest.approx(mc_o, rel=1e-9)
