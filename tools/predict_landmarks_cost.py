#!/usr/bin/env python
"""Device times (ctvio_last_timing, the library's HIP events) of ctvio_predict_landmarks_batch beside ctvio_project_landmarks_batch on the same
handle, on one GPU: one prediction of 21 samples per window from its newest frame time and every landmark of the window under it at one row
(TILE_PRED tiles: 8 points each), against the projection of every landmark into the newest frame (TILE_PROJ tiles).  Three batches: the mixed
batch of the tests (4 windows, solved 6 iterations, order-fixed), `config1` seed 1000 solved 15 iterations, and --windows config-2 windows
(P 211, L 200) solved 15 iterations.  After a warm-up the calls alternate; the median of the repetitions is printed, one JSON line per batch.
Not a test.
usage: python tools/predict_landmarks_cost.py [--windows N] [--reps N]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
cv = importlib.import_module("ctrl-vio_amd")


def measure(name, ws, iters, reps, **opts):
    from test_gpu_imu_predict import draw
    sam = [draw(w, 21, 900 + i % 8) for i, w in enumerate(ws)]
    imu = tuple(np.concatenate([x[k] for x in sam]) for k in range(3))
    ms = [21] * len(ws)
    pred = np.concatenate([np.full(w.L, i, np.int32) for i, w in enumerate(ws)])
    lm = np.concatenate([np.arange(w.L, dtype=np.int32) for w in ws])
    t = np.concatenate([np.full(w.L, int(max(w.v_tj.max(), w.v_ti.max())) if w.L else 0, np.int64) for w in ws])
    row = ((53 * lm + 7) % 480).astype(np.int32)
    win = list(range(len(ws)))
    full, vals, proj = [], [], []
    with cv.Solver(**opts) as s:
        s.set_windows([w.copy() for w in ws])
        s.solve(iters, writeback=False)
        s.predict_landmarks_batch(win, None, ms, *imu, pred, lm, row); s.project_landmarks_batch(pred, lm, t, row)     # warm-up
        s.predict_landmarks_batch(win, None, ms, *imu, pred, lm, row, cov=False)
        for _ in range(reps):
            o = s.predict_landmarks_batch(win, None, ms, *imu, pred, lm, row)
            full.append(s.last_timing()[0].copy())
            s.project_landmarks_batch(pred, lm, t, row)
            proj.append(s.last_timing()[0].copy())
            s.predict_landmarks_batch(win, None, ms, *imu, pred, lm, row, cov=False)
            vals.append(s.last_timing()[0].copy())
    a, b, c = (np.median(np.array(x), axis=0) for x in (full, proj, vals))
    r4 = lambda x: round(float(x), 4)
    print(json.dumps({"batch": name, "windows": len(ws), "predictions": len(ws), "points": int(lm.shape[0]), "status_nonzero": int((o.status != 0).sum()),
                      "predict_ms8": {"k_cov_prepare": r4(a[0]), "k_cov_solve": r4(a[1]), "k_cov_pred_jac": r4(a[2]), "k_imu_transition": r4(a[3]), "call": r4(a[7])},
                      "project_ms8": {"k_cov_prepare": r4(b[0]), "k_cov_solve": r4(b[1]), "k_cov_proj_jac": r4(b[2]), "call": r4(b[7])},
                      "predict_values_only_ms8": {"k_cov_pred_jac": r4(c[2]), "k_imu_transition": r4(c[3]), "call": r4(c[7])},
                      "k_cov_solve_ratio": round(float(a[1] / b[1]), 2), "jac_ratio": round(float(a[2] / b[2]), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    from test_gpu_covariance import DET, mixed_batch
    measure("mixed", mixed_batch(cv)[0], 6, a.reps, **DET)
    measure("config1 seed 1000", [cv.synth.make_window("config1", seed=1000)], 15, a.reps)
    uniq = [cv.synth.make_window("config2", seed=1011 + i) for i in range(min(a.windows, 8))]
    measure("config2", [uniq[i % len(uniq)] for i in range(a.windows)], 15, a.reps)


if __name__ == "__main__":
    main()
