"""python tools/wgclk_stats.py <csv> <grid> <first launch>: spread of the workgroup start / end ticks (10 ns) per launch"""
import csv
import sys
from collections import defaultdict

import numpy as np

path, grid, first = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
rows = defaultdict(list)
for r in csv.DictReader(open(path)):
    if int(r["grid"]) == grid and int(r["launch"]) >= first:
        rows[int(r["launch"])].append((int(r["t0"]), int(r["t1"]), int(r["n"]), int(r["wg"]) % 8))
print(f"{path}: launches {sorted(rows)}")
print("launch  start(min med max)        end(min med max)         items(min med max)  empty slot-time")
acc = []
for k in sorted(rows):
    a = np.array(rows[k], dtype=np.int64)
    z = a[:, 0].min()  # s_memrealtime: one 100 MHz clock for the chip
    s, e, n = (a[:, 0] - z) / 100.0, (a[:, 1] - z) / 100.0, a[:, 2]  # us
    empty = (e.max() - e).sum() / (len(e) * e.max())
    late = s.sum() / (len(e) * e.max())
    acc.append((np.median(s), s.max(), e.min(), np.median(e), e.max(), empty, late))
    print(f"{k:4d}   {s.min():8.0f} {np.median(s):8.0f} {s.max():8.0f}   {e.min():8.0f} {np.median(e):8.0f} {e.max():8.0f} us   "
          f"{n.min():5d} {int(np.median(n)):5d} {n.max():5d}   after the end {100 * empty:5.2f} %  before the start {100 * late:5.2f} %")
m = np.mean(np.array(acc), axis=0)
print(f"mean   start med {m[0]:.0f} max {m[1]:.0f}   end min {m[2]:.0f} med {m[3]:.0f} max {m[4]:.0f} us   empty after {100 * m[5]:.2f} % before {100 * m[6]:.2f} %")
