#!/usr/bin/env python
"""Solve time of deterministic = 2 (order-fixed accumulation, k_assemble_wide for the windows beyond the LDS-resident Hessian) against
deterministic = 0 (atomic assembly) on one GPU: 64 config-5 windows (P 571), 64 config5_spread windows (P 571) and one config5_spread
window at 25 ms knots (P 937).  15 LM iterations per solve; one handle per mode, warmed up (allocation, graph capture); the two modes are
timed alternately and the median of the repetitions is printed, one JSON line per case.
usage: python tools/deterministic_cost.py [--reps N]
       python tools/deterministic_cost.py --one CASE DET   (one warmed-up solve of case CASE (0, 1, 2) under DET: for a kernel trace)"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cv = importlib.import_module("ctrl-vio_amd")

CASES = [("64 x config5", "config5", 64, {}), ("64 x config5_spread", "config5_spread", 64, {}),
         ("1 x config5_spread @ 25 ms (P 937)", "config5_spread", 1, dict(dt_ns=25_000_000))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--one", type=int, nargs=2, metavar=("CASE", "DET"))
    a = ap.parse_args()
    if a.one:
        name, cfg, n, kw = CASES[a.one[0]]
        ws = [cv.synth.make_window(cfg, seed=1011 + i % 8, **kw) for i in range(n)]
        with cv.Solver(deterministic=a.one[1]) as s:
            for _ in range(2):
                s.set_windows([w.copy() for w in ws])
                s.solve(a.iters, writeback=False)
        return
    for name, cfg, n, kw in CASES:
        uniq = [cv.synth.make_window(cfg, seed=1011 + i, **kw) for i in range(min(n, 8))]
        ws = [uniq[i % len(uniq)] for i in range(n)]
        handles = {det: cv.Solver(deterministic=det) for det in (0, 2)}
        times = {0: [], 2: []}
        for s in handles.values():                      # warm-up
            s.set_windows([w.copy() for w in ws])
            s.solve(a.iters, writeback=False)
        for _ in range(a.reps):
            for det, s in handles.items():
                s.set_windows([w.copy() for w in ws])
                t0 = time.perf_counter()
                s.solve(a.iters, writeback=False)
                times[det].append(1e3 * (time.perf_counter() - t0))
        for s in handles.values():
            s.close()
        m0, m2 = statistics.median(times[0]), statistics.median(times[2])
        print(json.dumps({"case": name, "P": ws[0].P, "windows": n, "iters": a.iters, "det0_ms": round(m0, 3), "det2_ms": round(m2, 3),
                          "ratio": round(m2 / m0, 3), "det0_all": [round(t, 3) for t in times[0]], "det2_all": [round(t, 3) for t in times[2]]}),
              flush=True)


if __name__ == "__main__":
    main()
