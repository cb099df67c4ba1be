#!/usr/bin/env python
"""Device times (ctvio_last_timing, the library's HIP events) of ctvio_project_landmarks_batch beside ctvio_landmark_points_batch on the same
handle, on one GPU: one covariance call that projects every landmark once into the newest frame of its window (TILE_PROJ tiles: 8 queries
each) against the landmark cloud with covariances (TILE_POINT tiles: 5 landmarks each).  Three batches: the mixed batch of the tests (4
windows, solved 6 iterations, order-fixed), `config1` seed 1000 solved 15 iterations, and --windows config-2 windows (P 211, L 200) solved 15
iterations.  After a warm-up the two calls alternate; the median of the repetitions is printed, one JSON line per batch.  Not a test.
usage: python tools/time_project_landmarks.py [--windows N] [--reps N]"""
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
    win = np.concatenate([np.full(w.L, i, np.int32) for i, w in enumerate(ws)])
    lm = np.concatenate([np.arange(w.L, dtype=np.int32) for w in ws])
    t = np.concatenate([np.full(w.L, int(max(w.v_tj.max(), w.v_ti.max())) if w.L else 0, np.int64) for w in ws])
    row = ((53 * lm + 7) % 480).astype(np.int32)
    proj, pts, vals = [], [], []
    with cv.Solver(**opts) as s:
        s.set_windows([w.copy() for w in ws])
        s.solve(iters, writeback=False)
        s.project_landmarks_batch(win, lm, t, row); s.landmark_points_batch(); s.project_landmarks_batch(win, lm, t, row, cov=False)   # warm-up
        for _ in range(reps):
            o = s.project_landmarks_batch(win, lm, t, row)
            proj.append(s.last_timing()[0].copy())
            _, _, st = s.landmark_points_batch()
            pts.append(s.last_timing()[0].copy())
            s.project_landmarks_batch(win, lm, t, row, cov=False)
            vals.append(s.last_timing()[0].copy())
    a, b, c = (np.median(np.array(x), axis=0) for x in (proj, pts, vals))
    r4 = lambda x: round(float(x), 4)
    print(json.dumps({"batch": name, "windows": len(ws), "queries": int(lm.shape[0]), "status_nonzero": int((o.status != 0).sum()),
                      "points_status_nonzero": int((st != 0).sum()),
                      "project_ms8": {"k_cov_prepare": r4(a[0]), "k_cov_solve": r4(a[1]), "k_cov_proj_jac": r4(a[2]), "call": r4(a[7])},
                      "landmark_points_ms8": {"k_cov_prepare": r4(b[0]), "k_cov_solve": r4(b[1]), "k_cov_point_jac": r4(b[2]), "call": r4(b[7])},
                      "project_values_only_ms8": {"k_cov_proj_jac": r4(c[2]), "call": r4(c[7])},
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
