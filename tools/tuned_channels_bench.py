#!/usr/bin/env python3
"""Tuned channel handle (jsdr_bpsk_create_tuned_channels) against a tuned handle on the duplicated input; prints one JSON line.

--inputs x --channels rows of --samples samples a call at 96 kHz, int16, distinct non-periodic tunings:

  (t) a tuned handle of inputs x channels streams reading a buffer in which every input is repeated `channels` times
  (c) a tuned channel handle reading the inputs themselves

For each: wall time of a call plus a sync of the handle (median of --steps after --warmup), and from the profile slots of one more
call k_tuner_walk and the front end (k_front_pst / k_chan_front_pst) alone; the input bytes resident follow from the layout.
--only c: (c) alone, for timing builds of other tile shapes (tools/build_define.sh, JSDR_LIB)."""
import argparse
import json
import os
import statistics
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


def fill(nin, rep, L):
    """nin inputs of L samples, each row written `rep` times in a row (inputs repeat every 16)"""
    rng = np.random.default_rng(1)
    blk = rng.integers(-12000, 12000, (16, 2 * L), dtype=np.int16)
    buf = J.DeviceBuffer(4 * L * nin * rep)
    for r in range(nin * rep):
        row = np.ascontiguousarray(blk[(r // rep) % 16])
        J.lib().jsdr_memcpy_h2d(J.binding.C.c_void_p(buf.ptr + 4 * L * r), J.binding._addr(row), J.binding.C.c_size_t(4 * L))
    J.binding.stream_sync()
    return buf


def distinct(N):
    """N tunings between 9 and 15 kHz whose tuner index has no period within 256 samples"""
    return [9000.0 + 2.9296875 * s + 0.37 for s in range(N)]


def measure(d, buf, L, warmup, steps):
    ms = timed(lambda: (d.batch_i16(buf.ptr, 2 * L, L), d.sync()), warmup, steps)
    d.profile_enable(True)
    d.profile_read()
    d.batch_i16(buf.ptr, 2 * L, L)
    d.sync()
    p = d.profile_read()
    d.profile_enable(False)
    return {"call_ms": round(ms, 3), "walk_ms": round(p["k_tuner_walk"][0], 3), "front_ms": round(p["k_front"][0], 3),
            "front": d.front_kernel_name(), "input_bytes": buf.nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=256)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--only", default="", help="c: the tuned channel handle alone")
    a = ap.parse_args()
    nin, nch, L = a.inputs, a.channels, a.samples
    out = {"inputs": nin, "channels": nch, "samples_per_call": L, "rate": RATE, "lib": os.path.basename(J.library_path())}
    tun = distinct(nin * nch)
    if a.only != "c":
        buf = fill(nin, nch, L)
        d = J.BpskTuned(RATE, 8192, tun, max_batch_samples=L)
        out["t"] = measure(d, buf, L, a.warmup, a.steps)
        del d, buf
    buf = fill(nin, 1, L)
    d = J.BpskTunedChannels(RATE, 8192, nin, nch, tun, max_batch_samples=L)
    out["c"] = measure(d, buf, L, a.warmup, a.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
