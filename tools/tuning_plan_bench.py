#!/usr/bin/env python3
"""What a tuning plan costs (jsdr_bpsk_plan_stream_tunings, jsdr_bpsk_plan_stream_ramps: retunes inside a batch call of a tuned
handle); prints one JSON line.

The shape of tools/stream_tuning_bench.py: 2048 streams x 2^20 samples a call at 96 kHz, distinct non-periodic tunings, wall time
of a call plus a sync of the handle, median of --steps after --warmup, all in one run:

  (d) the tuned call without a plan (the kernels a plan does not touch)
  (f) a planned call: every stream one entry every 38 400 samples (27 entries, +10 Hz each), staggered by stream so that no two
      streams of a wave retune at the same sample.  f_plan_ms: giving the plan (validation, copy to the device), not in f_call_ms
  (g) the same retunes the only way there is without a plan: the call cut into 28 pieces with set_stream_tunings between them
      (which lines the instants up; the plan does not need that)
  (h) a ramp plan (jsdr_bpsk_plan_stream_ramps): (f)'s 27 entries a stream at (f)'s samples, each with the slope that reaches the next
      one's tuning (+10 Hz in 38 400 samples): every sample behind a stream's first entry lies under a slope
  (i) the same curves as a step plan: one entry every 256 samples from each stream's first entry on (0.07 Hz a step)
  and, from the profile slots of one more call each, k_tuner_walk and k_front for (d), (f), (h) and (i); for (h) and (i) the time
  of giving the plan and the bytes it takes on the device.  (d) and (f) are measured in the same run: compare with them alone."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import java_sdr_amd as J  # noqa: E402
from stream_tuning_bench import RATE, distinct, fill, slots  # noqa: E402

EVERY = 38400
FINE = 256  # (i): samples between two step entries that follow (h)'s curves


def median_ms(fn, warmup, steps, before=None):
    ts = []
    for k in range(warmup + steps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    N, L = a.streams, a.samples
    tun = distinct(N)
    nent = (L - 1) // EVERY
    room = L - nent * EVERY  # the stagger stays inside the call
    stagger = [(5 * s) % max(room, 1) for s in range(N)]
    st = np.repeat(np.arange(N, dtype=np.int32), nent)
    at = np.array([k * EVERY + stagger[s] for s in range(N) for k in range(1, nent + 1)], np.int64)
    tu = np.array([tun[s] + 10.0 * k for s in range(N) for k in range(1, nent + 1)], np.float64)
    out = {"streams": N, "samples_per_call": L, "rate": RATE, "entries_per_stream": nent, "entries": int(st.size)}
    buf = fill(N, L)
    d = J.BpskTuned(RATE, 8192, tun, max_batch_samples=L)

    def call():
        d.batch_i16(buf.ptr, 2 * L, L)
        d.sync()

    def reset():
        d.set_stream_tunings(0, tun)

    out["d_unplanned_ms"] = round(median_ms(call, a.warmup, a.steps, reset), 3)
    out["d_front"] = d.front_kernel_name()
    reset()
    out["d_walk_ms"], out["d_front_ms"] = slots(d, buf, L)

    def give():
        reset()
        d.plan_tunings(st, at, tu)

    out["f_planned_ms"] = round(median_ms(call, a.warmup, a.steps, give), 3)
    out["f_front"] = d.front_kernel_name()
    reset()
    out["f_plan_ms"] = round(median_ms(lambda: d.plan_tunings(st, at, tu), 0, a.steps), 3)
    out["f_walk_ms"], out["f_front_ms"] = slots(d, buf, L)
    assert d.planned() == 0 and d.stream_tuning(N - 1) == tun[N - 1] + 10.0 * nent

    def pieces():
        for k in range(nent + 1):
            if k:
                d.set_stream_tunings(0, [t + 10.0 * k for t in tun])
            a0, a1 = k * EVERY, (L if k == nent else (k + 1) * EVERY)
            d.batch_i16(buf.ptr + 4 * a0, 2 * L, a1 - a0)
        d.sync()

    out["g_pieces_ms"] = round(median_ms(pieces, a.warmup, a.steps, reset), 3)
    out["g_pieces"] = nent + 1
    out["f_over_d"] = round(out["f_planned_ms"] / out["d_unplanned_ms"], 3)
    out["g_over_d"] = round(out["g_pieces_ms"] / out["d_unplanned_ms"], 3)

    # (h): (f)'s entries with slopes; (i): the curves of (h) sampled every FINE samples
    slope = np.full(st.size, 10.0 / EVERY)
    sg = np.asarray(stagger, np.int64)
    i_st, i_at, i_tu = [], [], []
    for s in range(N):
        ns = np.arange(EVERY + sg[s], L, FINE, dtype=np.int64)
        k = (ns - sg[s]) // EVERY  # the entry of (h) in effect: 1 .. nent
        i_st.append(np.full(ns.size, s, np.int32))
        i_at.append(ns)
        i_tu.append(tun[s] + 10.0 * k + (ns - (k * EVERY + sg[s])).astype(np.float64) * (10.0 / EVERY))
    i_st, i_at, i_tu = np.concatenate(i_st), np.concatenate(i_at), np.concatenate(i_tu)
    for key, give_plan, nentries, per in (("h", lambda: d.plan_ramps(st, at, tu, slope), int(st.size), 24),
                                          ("i", lambda: d.plan_tunings(i_st, i_at, i_tu), int(i_st.size), 16)):
        def give_it():
            reset()
            give_plan()

        out[key + "_ms"] = round(median_ms(call, a.warmup, a.steps, give_it), 3)
        out[key + "_front"] = d.front_kernel_name()
        reset()
        out[key + "_plan_ms"] = round(median_ms(give_plan, 0, a.steps), 3)
        out[key + "_walk_ms"], out[key + "_front_ms"] = slots(d, buf, L)
        out[key + "_entries"] = nentries
        out[key + "_plan_bytes"] = nentries * per + 8 * (N + 1)
        assert d.planned() == 0
    assert d.stream_tuning(N - 1) == i_tu[-1]  # ((i) ran last: its last entry)
    out["h_over_d"] = round(out["h_ms"] / out["d_unplanned_ms"], 3)
    out["h_over_f"] = round(out["h_ms"] / out["f_planned_ms"], 3)
    out["i_over_d"] = round(out["i_ms"] / out["d_unplanned_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
