#!/usr/bin/env python3
"""Tuned handle (jsdr_bpsk_create_tuned: every stream its own tuning) against ordinary handles; prints one JSON line.

2048 streams x 2^20 samples a call at 96 kHz, wall time of a call plus a sync of the handle, median of --steps after --warmup:

  (a) an ordinary handle at 12000 Hz, its default path (k_fm)
  (b) the same under JSDR_KNOBS=1 JSDR_FM=0: the three-kernel path the tuned handle is built on (the same round trip of dm
      through memory).  The knobs are read once a process, so (b) runs in a child process of this tool.
  (c) a tuned handle with every stream at 12000 Hz
  (d) a tuned handle with 2048 distinct tunings, none of them periodic
  (e) from the profile slots of one more call: k_tuner_walk and k_front_pst alone, for (d) and for 64 streams

(a) and (b) run code this handle does not touch: they are the yardstick of the same run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import java_sdr_amd as J  # noqa: E402

RATE = 96000


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def fill(N, L):
    """N rows of L samples (rows repeat every 16)"""
    rng = np.random.default_rng(1)
    blk = rng.integers(-12000, 12000, 2 * L * 16, dtype=np.int16)
    buf = J.DeviceBuffer(4 * L * N)
    for r in range(0, N, 16):
        rows = min(16, N - r)
        J.lib().jsdr_memcpy_h2d(J.binding.C.c_void_p(buf.ptr + 4 * L * r), J.binding._addr(blk), J.binding.C.c_size_t(4 * L * rows))
    J.binding.stream_sync()
    return buf


def distinct(N):
    """N tunings between 9 and 15 kHz whose tuner index has no period within 256 samples"""
    return [9000.0 + 2.9296875 * s + 0.37 for s in range(N)]


def ordinary(buf, N, L, warmup, steps):
    e = J.Bpsk(rate=RATE, blen=8192, tuning=12000, nstreams=N, max_batch_samples=L)
    ms = timed(lambda: (e.batch_i16(buf.ptr, 2 * L, L), e.sync()), warmup, steps)
    return round(ms, 3), e.front_kernel_name()


def slots(d, buf, L):
    d.profile_enable(True)
    d.profile_read()
    d.batch_i16(buf.ptr, 2 * L, L)
    d.sync()
    p = d.profile_read()
    d.profile_enable(False)
    return round(p["k_tuner_walk"][0], 3), round(p["k_front"][0], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--part", default="", help="b: the child process of (b)")
    a = ap.parse_args()
    N, L = a.streams, a.samples
    if a.part == "b":
        ms, front = ordinary(fill(N, L), N, L, a.warmup, a.steps)
        print(json.dumps({"b_three_kernel_ms": ms, "b_front": front}))
        return
    out = {"streams": N, "samples_per_call": L, "rate": RATE}
    env = dict(os.environ, JSDR_KNOBS="1", JSDR_FM="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "b", "--streams", str(N), "--samples", str(L),
                        "--warmup", str(a.warmup), "--steps", str(a.steps)], env=env, capture_output=True, text=True, check=True)
    out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    buf = fill(N, L)
    out["a_ordinary_ms"], out["a_front"] = ordinary(buf, N, L, a.warmup, a.steps)
    d = J.BpskTuned(RATE, 8192, [12000.0] * N, max_batch_samples=L)
    out["c_tuned_equal_ms"] = round(timed(lambda: (d.batch_i16(buf.ptr, 2 * L, L), d.sync()), a.warmup, a.steps), 3)
    del d
    d = J.BpskTuned(RATE, 8192, distinct(N), max_batch_samples=L)
    out["d_tuned_distinct_ms"] = round(timed(lambda: (d.batch_i16(buf.ptr, 2 * L, L), d.sync()), a.warmup, a.steps), 3)
    out["d_front"] = d.front_kernel_name()
    out["e_walk_ms"], out["e_front_pst_ms"] = slots(d, buf, L)
    del d
    n64 = min(64, N)
    d = J.BpskTuned(RATE, 8192, distinct(n64), max_batch_samples=L)
    d.batch_i16(buf.ptr, 2 * L, L)
    d.sync()
    out["e_walk_64_ms"], out["e_front_pst_64_ms"] = slots(d, buf, L)
    out["c_over_b"] = round(out["c_tuned_equal_ms"] / out["b_three_kernel_ms"], 3)
    out["d_over_b"] = round(out["d_tuned_distinct_ms"] / out["b_three_kernel_ms"], 3)
    out["d_over_a"] = round(out["d_tuned_distinct_ms"] / out["a_ordinary_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
