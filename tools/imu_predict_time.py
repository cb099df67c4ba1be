#!/usr/bin/env python
"""Device time of ctvio_imu_predict_batch beside ctvio_nav_state_batch on the same queries, from ctvio_last_timing (needs a GPU): one query
of `--samples` IMU samples per window of a batch of `--windows` config-2 windows (8 distinct, replicated), from the newest frame time.
usage: python tools/imu_predict_time.py [--windows 2048] [--samples 21] [--repeat 9]
Prints the median and the spread over the repeats after two warm-up calls of each entry."""
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
    ap.add_argument("--samples", type=int, default=21)
    ap.add_argument("--repeat", type=int, default=9)
    a = ap.parse_args()
    cv = importlib.import_module("ctrl-vio_amd")
    uniq = [cv.synth.make_window("config2", seed=1000 + i) for i in range(8)]
    ws = [uniq[i % 8].copy() for i in range(a.windows)]
    rng = np.random.default_rng(1)
    n, m = a.windows, a.samples
    t0 = np.array([w.t0_ns + (w.F - 1) * 100_000_000 for w in ws], np.int64)
    t = (t0[:, None] + 5_000_000 * np.arange(m, dtype=np.int64)[None, :]).reshape(-1)
    gyro = rng.normal(0, 0.5, (n * m, 3))
    acc = np.tile(np.asarray(ws[0].gravity, float), (n * m, 1)) + rng.normal(0, 1.0, (n * m, 3))
    win = np.arange(n, dtype=np.int32)
    rows = {"imu_predict": [], "imu_predict_last_only": [], "imu_predict_values": [], "nav_state": []}
    with cv.Solver() as s:
        s.set_windows(ws)
        s.solve(15)
        calls = {"imu_predict": lambda: s.imu_predict_batch(win, None, [m] * n, t, gyro, acc),
                 "imu_predict_last_only": lambda: s.imu_predict_batch(win, None, [m] * n, t, gyro, acc, last_only=True),
                 "imu_predict_values": lambda: s.imu_predict_batch(win, None, [m] * n, t, gyro, acc, cov=False),
                 "nav_state": lambda: s.nav_state_batch(win, t0)}
        for name, call in calls.items():
            for k in range(a.repeat + 2):
                out = call()
                ms, _ = s.last_timing()
                if k >= 2:
                    rows[name].append([float(x) for x in ms])
            assert not out[2].any(), (name, np.bincount(out[2]))
    res = {"windows": n, "samples": m, "repeat": a.repeat}
    for name, r in rows.items():
        r = np.array(r)
        res[name] = {"ms8_median": [round(float(x), 4) for x in np.median(r, 0)], "ms8_min": [round(float(x), 4) for x in r.min(0)],
                     "ms8_max": [round(float(x), 4) for x in r.max(0)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
