#!/usr/bin/env python
"""Device time of ctvio_body_rates_batch beside ctvio_nav_state_batch on the same queries, from ctvio_last_timing (needs a GPU): one query
per window of a batch of `--windows` config-2 windows (8 distinct, replicated), at the newest frame time, after a 15-iteration solve.
usage: python tools/body_rates_time.py [--windows 2048] [--repeat 9]
The entries are called alternately after two warm-up rounds; prints the median and the spread of ms8 over the repeats."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=9)
    a = ap.parse_args()
    cv = importlib.import_module("ctrl-vio_amd")
    uniq = [cv.synth.make_window("config2", seed=1000 + i) for i in range(8)]
    ws = [uniq[i % 8].copy() for i in range(a.windows)]
    n = a.windows
    t = np.array([w.t0_ns + (w.F - 1) * 100_000_000 for w in ws], np.int64)
    win = np.arange(n, dtype=np.int32)
    meas = np.tile(np.concatenate([np.zeros(3), -np.asarray(ws[0].gravity, float)]), (n, 1))
    rows = {"body_rates": [], "body_rates_gate": [], "body_rates_values": [], "nav_state": []}
    with cv.Solver() as s:
        s.set_windows(ws)
        s.solve(15)
        calls = {"body_rates": lambda: s.body_rates_batch(win, t)[3], "body_rates_gate": lambda: s.body_rates_batch(win, t, meas=meas)[3],
                 "body_rates_values": lambda: s.body_rates_batch(win, t, cov=False)[3], "nav_state": lambda: s.nav_state_batch(win, t)[2]}
        for k in range(a.repeat + 2):
            for name, call in calls.items():
                st = call()
                ms, _ = s.last_timing()
                assert not st.any(), (name, np.bincount(st))
                if k >= 2:
                    rows[name].append([float(x) for x in ms])
    res = {"windows": n, "P": ws[0].P, "repeat": a.repeat}
    for name, r in rows.items():
        r = np.array(r)
        res[name] = {"ms8_median": [round(float(x), 4) for x in np.median(r, 0)], "ms8_min": [round(float(x), 4) for x in r.min(0)],
                     "ms8_max": [round(float(x), 4) for x in r.max(0)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
