#!/usr/bin/env python
"""Bit comparison of the covariance entries between two builds of the library, on one GPU.  `dump OUT.npz` runs every entry that goes through
k_cov_solve -- ctvio_covariance_batch (with var_rho), ctvio_pose_covariance_batch (body and camera pose), ctvio_landmark_points_batch,
ctvio_nav_state_batch, ctvio_relative_pose_batch, ctvio_project_landmarks_batch, ctvio_body_rates_batch, ctvio_imu_predict_batch,
ctvio_predict_landmarks_batch, ctvio_visual_gate_batch and ctvio_imu_gate_batch, each with every optional output (gates, row model; the two
leave-one-out gates with the default and a strict min_redundancy) and, where the entry has one, in its values-only form (covariance outputs
null) -- on the mixed batch of tests/test_gpu_covariance.py under deterministic = 2, at the initial state and after a 6-iteration solve,
and on a solved `config1` window (ctvio_covariance with 64 scattered selections + var_rho there), with the library CTVIO_LIB_PATH names
(default: the in-tree build), and saves every output and the solved state.  The two gates run once more on the solved mixed batch with a
handle created under CTVIO_GATE_SLICE=64, the slice budget their GPU tests use to force several slices.  The query sets are those of the entries' own GPU tests.  `compare A.npz B.npz` lists the
arrays whose bits differ (exit status 1 if any).  Not a test: the second build has to come from another checkout.
usage: python tools/covariance_bits.py dump new.npz; CTVIO_LIB_PATH=/other/libctvio.so python tools/covariance_bits.py dump old.npz;
       python tools/covariance_bits.py compare new.npz old.npz"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def put(out, tag, res):
    """the arrays of an entry's result: a tuple, or a namespace"""
    items = vars(res).items() if hasattr(res, "__dict__") else enumerate(res)
    for k, v in items:
        if isinstance(v, np.ndarray):
            out[f"{tag}_{k}"] = v


def query_entries(out, tag, s, ws):
    """relative_pose, project_landmarks, body_rates, imu_predict, predict_landmarks, visual_gate and imu_gate on the windows ws as uploaded
    to s, each also values only (cov=False)"""
    import test_gpu_imu_predict as ti
    import test_gpu_predict_landmarks as tl
    import test_gpu_project_landmarks as tp
    from test_gpu_nav_state import mixed_queries as nav_queries
    from test_gpu_relative_pose import mixed_queries as rel_queries
    put(out, f"{tag}_rel", s.relative_pose_batch(*rel_queries(ws)))
    put(out, f"{tag}_rel_camera", s.relative_pose_batch(*rel_queries(ws), ws[-1].q_CI, ws[-1].p_CI))
    put(out, f"{tag}_rel_values", s.relative_pose_batch(*rel_queries(ws), cov=False))
    win, Q = tp.mixed_queries(ws)
    obs = np.stack([0.01 * np.cos(np.arange(len(Q))), 0.01 * np.sin(np.arange(len(Q)))], 1)
    put(out, f"{tag}_proj", s.project_landmarks_batch(win, *tp.cols(Q), obs=obs))
    put(out, f"{tag}_proj_rows", s.project_landmarks_batch(win, *tp.cols(Q), obs=obs, row_model=(400.0, 240.0, 480, 3)))
    put(out, f"{tag}_proj_values", s.project_landmarks_batch(win, *tp.cols(Q), cov=False, row_model=(400.0, 240.0, 480, 3)))
    nwin, nt, nf = nav_queries(ws)
    put(out, f"{tag}_nav_values", s.nav_state_batch(nwin, nt, nf, cov=False))
    meas = np.tile(np.array([0.1, -0.2, 0.3, 0.5, -0.4, 9.6]), (len(nwin), 1))
    put(out, f"{tag}_rates", s.body_rates_batch(nwin, nt, nf, meas=meas))
    put(out, f"{tag}_rates_values", s.body_rates_batch(nwin, nt, nf, cov=False))
    pw, fr, ms, sam = ti.mixed_queries(ws)
    put(out, f"{tag}_imu", s.imu_predict_batch(pw, fr, ms, *ti.cat(sam, range(len(pw)))))
    put(out, f"{tag}_imu_last", s.imu_predict_batch(pw, fr, ms, *ti.cat(sam, range(len(pw))), last_only=True))
    put(out, f"{tag}_imu_values", s.imu_predict_batch(pw, fr, ms, *ti.cat(sam, range(len(pw))), cov=False))
    preds = [([0, w.F - 1, w.F // 2, w.F - 1][i % 4],) + tl.draw(w, [21, 5, 21, 1][i % 4], 600 + i) for i, w in enumerate(ws)]
    pts = [(i, l, (53 * l + 7) % 480) for i, w in enumerate(ws) for l in range(w.L)]
    pobs = np.stack([0.01 * np.sin(np.arange(len(pts))), 0.01 * np.cos(np.arange(len(pts)))], 1)
    put(out, f"{tag}_pred", tl.batch_call(s, list(range(len(ws))), preds, pts, obs=pobs))
    put(out, f"{tag}_pred_rows", tl.batch_call(s, list(range(len(ws))), preds, pts, obs=pobs, row_model=(400.0, 240.0, 480, 3)))
    put(out, f"{tag}_pred_values", tl.batch_call(s, list(range(len(ws))), preds, pts, cov=False, row_model=(400.0, 240.0, 480, 3)))
    put(out, f"{tag}_points_values", s.landmark_points_batch(cov=False))
    gates(out, tag, s)


def gates(out, tag, s):
    """visual_gate and imu_gate: default and strict min_redundancy with every optional output, and values only"""
    put(out, f"{tag}_gate", s.visual_gate_batch())
    put(out, f"{tag}_gate_strict", s.visual_gate_batch(min_redundancy=0.5))
    put(out, f"{tag}_gate_values", s.visual_gate_batch(cov=False))
    put(out, f"{tag}_imugate", s.imu_gate_batch())
    put(out, f"{tag}_imugate_strict", s.imu_gate_batch(min_redundancy=0.5))
    put(out, f"{tag}_imugate_values", s.imu_gate_batch(cov=False))


def dump(path):
    cv = importlib.import_module("ctrl-vio_amd")
    import cov_helpers as ch
    from test_gpu_covariance import DET, mixed_batch
    from test_gpu_nav_state import mixed_queries as nav_queries
    from test_gpu_pose_covariance import mixed_queries
    out = {}
    ws, sels = mixed_batch(cv)
    win, t = mixed_queries(ws)
    nwin, nt, nf = nav_queries(ws)
    with cv.Solver(**DET) as s:
        s.set_windows([w.copy() for w in ws])
        for tag in ("init", "solved"):
            covs, vars_, sing = s.covariance_batch(sels, rho=True)
            for i, (c, v) in enumerate(zip(covs, vars_)):
                out[f"{tag}_cov{i}"] = c; out[f"{tag}_var{i}"] = v
            out[f"{tag}_singular"] = sing
            out[f"{tag}_pose"], out[f"{tag}_pose_status"] = s.pose_covariance_batch(win, t)
            out[f"{tag}_pose_camera"], _ = s.pose_covariance_batch(win, t, ws[1].q_CI, ws[1].p_CI)
            out[f"{tag}_points"], out[f"{tag}_points_cov"], out[f"{tag}_points_status"] = s.landmark_points_batch()
            out[f"{tag}_nav"], out[f"{tag}_nav_cov"], out[f"{tag}_nav_status"] = s.nav_state_batch(nwin, nt, nf)
            query_entries(out, tag, s, ws)
            s.solve(6, writeback=False)
        state = s.get_batch_state()
        for i, a in enumerate(state):
            out[f"state{i}"] = a
    os.environ["CTVIO_GATE_SLICE"] = "64"   # (read once per handle, at its creation)
    try:
        with cv.Solver(**DET) as s:
            s.set_windows([w.copy() for w in ws])
            s.solve(6, writeback=False)
            gates(out, "sliced", s)
    finally:
        del os.environ["CTVIO_GATE_SLICE"]
    w = cv.synth.make_window("config1", seed=1000)
    with cv.Solver() as s:
        s.set_windows([w.copy()])
        s.solve(15, writeback=False)
        out["config1_cov"], out["config1_var"], _ = s.covariance(0, ch.scattered_selection(w, 64), rho=True)
        query_entries(out, "config1", s, [w])
    np.savez(path, **out)
    print(f"saved {len(out)} arrays to {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files)) + [k for k in a.files if k in b.files and not np.array_equal(a[k], b[k], equal_nan=True)]
    print(f"{len(a.files)} arrays, differing: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
