#!/usr/bin/env python
"""Device times (ctvio_last_timing, the library's HIP events) of three calls on 256 config-2 windows (P 211, L 200) solved 15 iterations, one
handle, on one GPU: ctvio_landmark_points_batch with covariances (TILE_POINT tiles: ceil(L / 5) per window), the same points only (one
kernel, nothing linearised) and ctvio_covariance_batch with var_rho and no selection (TILE_RHO tiles: ceil(L / 16) per window).  After a
warm-up of every call the three are timed in turn; the median of the repetitions is printed as one JSON line.  Not a test.
usage: python tools/time_landmark_points.py [--windows N] [--reps N]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cv = importlib.import_module("ctrl-vio_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    uniq = [cv.synth.make_window("config2", seed=1011 + i) for i in range(min(a.windows, 8))]
    ws = [uniq[i % len(uniq)] for i in range(a.windows)]
    none = [[] for _ in ws]
    full, points, rho = [], [], []
    with cv.Solver() as s:
        s.set_windows([w.copy() for w in ws])
        s.solve(15, writeback=False)
        s.landmark_points_batch(); s.landmark_points_batch(cov=False); s.covariance_batch(none, rho=True)   # warm-up (scratch allocation)
        for _ in range(a.reps):
            _, _, st = s.landmark_points_batch()
            full.append(s.last_timing()[0].copy())
            s.landmark_points_batch(cov=False)
            points.append(s.last_timing()[0].copy())
            _, _, sing = s.covariance_batch(none, rho=True)
            rho.append(s.last_timing()[0].copy())
    f, p, r = (np.median(np.array(x), axis=0) for x in (full, points, rho))
    L = ws[0].L
    print(json.dumps({"windows": a.windows, "P": ws[0].P, "L": L, "status_nonzero": int((st != 0).sum()), "singular": int(sing.sum()),
                      "points_cov_call_ms": round(float(f[7]), 4), "points_cov_k_cov_prepare_ms": round(float(f[0]), 4),
                      "points_cov_k_cov_solve_ms": round(float(f[1]), 4), "points_cov_k_cov_point_jac_ms": round(float(f[2]), 4),
                      "points_only_call_ms": round(float(p[7]), 4), "points_only_kernel_ms": round(float(p[0]), 4),
                      "var_rho_call_ms": round(float(r[7]), 4), "var_rho_k_cov_solve_ms": round(float(r[1]), 4),
                      "call_ratio": round(float(f[7] / r[7]), 2), "k_cov_solve_ratio": round(float(f[1] / r[1]), 2),
                      "tile_ratio": round(-(-L // 5) / -(-L // 16), 2)}), flush=True)


if __name__ == "__main__":
    main()
