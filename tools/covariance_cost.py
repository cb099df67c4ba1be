#!/usr/bin/env python
"""Time of ctvio_covariance_batch (31 selected trajectory unknowns per window + var_rho) against ctvio_lm_step on the same handle, on one GPU:
1 x and 64 x config 2 (P 211, L 200) and one config5_spread window at 23 ms knots (P 1003, L 1000).  The handle is warmed up; the two calls
are timed alternately (wall clock around the blocking call) and the median of the repetitions is printed, one JSON line per case, with the
device times of k_cov_prepare / k_cov_solve / k_cov_gram and of the whole call from the library's HIP events (ctvio_last_timing).
usage: python tools/covariance_cost.py [--reps N]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cv = importlib.import_module("ctrl-vio_amd")

CASES = [("1 x config2", "config2", 1, {}), ("64 x config2", "config2", 64, {}),
         ("1 x config5_spread @ 23 ms (P 1003)", "config5_spread", 1, dict(dt_ns=23_000_000))]


def selection(w, n=31):
    """The newest knots that can carry information (the last knot is padding), the last bias state and the line delay."""
    P, K = w.P, w.K
    return list(range(6 * (K - 5), 6 * (K - 1))) + list(range(P - 7, P))[: n - 24]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    for name, cfg, n, kw in CASES:
        uniq = [cv.synth.make_window(cfg, seed=1011 + i, **kw) for i in range(min(n, 8))]
        ws = [uniq[i % len(uniq)] for i in range(n)]
        sels = [selection(w) for w in ws]
        t_cov, t_step, dev = [], [], []
        with cv.Solver() as s:
            s.set_windows([w.copy() for w in ws])
            s.lm_step(0)
            s.covariance_batch(sels, rho=True)        # warm-up (scratch allocation)
            for _ in range(a.reps):
                t0 = time.perf_counter()
                s.lm_step(0)
                t1 = time.perf_counter()
                _, _, sing = s.covariance_batch(sels, rho=True)
                t2 = time.perf_counter()
                t_step.append(1e3 * (t1 - t0)); t_cov.append(1e3 * (t2 - t1))
                dev.append(s.last_timing()[0].copy())
        d = np.median(np.array(dev), axis=0)
        ms, mc = statistics.median(t_step), statistics.median(t_cov)
        print(json.dumps({"case": name, "P": ws[0].P, "L": ws[0].L, "windows": n, "selected": len(sels[0]), "singular": int(sing.sum()),
                          "lm_step_ms": round(ms, 3), "covariance_ms": round(mc, 3), "ratio": round(mc / ms, 2),
                          "k_cov_prepare_ms": round(float(d[0]), 4), "k_cov_solve_ms": round(float(d[1]), 4), "k_cov_gram_ms": round(float(d[2]), 4),
                          "call_device_ms": round(float(d[7]), 4)}), flush=True)


if __name__ == "__main__":
    main()
