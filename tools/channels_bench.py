#!/usr/bin/env python3
"""Channel handle (jsdr_bpsk_create_channels) against ordinary handles; prints one JSON line.

  * K in {1, 2, 8, 16} channels x S = 2048 / K inputs (S K = 2048 streams), 2^20 samples a call, periodic tunings
    (multiples of rate / 256: the tuner index has a period <= 256) and tunings without such a period; against an ordinary
    handle of S K streams over the same inputs tiled K times (its own tuning, 12 kHz: k_fm)
  * one-frame receive_i16 latency of a 2-channel handle against two 1-stream handles (2048-sample frames)

Wall time per call: the call plus a sync of the handle, median of --steps after --warmup.  The host's schedule work is
inside that time (non-periodic channels build theirs every call).  FETCH_SIZE is a separate rocprofv3 --pmc run."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--ks", default="1,2,8,16")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--only", default="", help="k=K,periodic=0|1: one channel-handle configuration (for a profiler run)")
    a = ap.parse_args()
    N, L = a.streams, a.samples
    rng = np.random.default_rng(1)
    # the input: N rows of L samples (rows repeat every 16: an ordinary handle's tiled input is the same memory)
    blk = rng.integers(-12000, 12000, 2 * L * 16, dtype=np.int16)
    buf = J.DeviceBuffer(4 * L * N)
    for r in range(0, N, 16):
        J.lib().jsdr_memcpy_h2d(J.binding.C.c_void_p(buf.ptr + 4 * L * r), J.binding._addr(blk), J.binding.C.c_size_t(blk.nbytes))
    J.binding.stream_sync()
    out = {"streams": N, "samples_per_call": L, "rate": RATE}
    if a.only:
        kv = dict(x.split("=") for x in a.only.split(","))
        K, per = int(kv["k"]), int(kv["periodic"])
        tun = [375.0 * (32 + 8 * c) for c in range(K)] if per else [12010.0 + 10 * c for c in range(K)]
        d = J.BpskChannels(RATE, 8192, tun, ninputs=N // K, max_batch_samples=L)
        out["only_ms"] = timed(lambda: (d.batch_i16(buf.ptr, 2 * L, L), d.sync()), a.warmup, a.steps)
        print(json.dumps(out))
        return
    e = J.Bpsk(rate=RATE, blen=8192, tuning=12000, nstreams=N, max_batch_samples=L)
    out["ordinary_ms"] = timed(lambda: (e.batch_i16(buf.ptr, 2 * L, L), e.sync()), a.warmup, a.steps)
    out["ordinary_front"] = e.front_kernel_name()
    del e
    for K in [int(k) for k in a.ks.split(",")]:
        for per in (1, 0):
            tun = [375.0 * (32 + 8 * c) for c in range(K)] if per else [12010.0 + 10 * c for c in range(K)]
            d = J.BpskChannels(RATE, 8192, tun, ninputs=N // K, max_batch_samples=L)
            ms = timed(lambda: (d.batch_i16(buf.ptr, 2 * L, L), d.sync()), a.warmup, a.steps)
            st = d.schedule_stats()["computed_inline"]
            out[f"k{K}_{'periodic' if per else 'nonperiodic'}_ms"] = round(ms, 3)
            out[f"k{K}_{'periodic' if per else 'nonperiodic'}_schedules"] = st
            del d
    # host cost of the schedules alone: 16 non-periodic channels, one input
    d = J.BpskChannels(RATE, 8192, [12010.0 + 10 * c for c in range(16)], ninputs=1, max_batch_samples=L)
    one = timed(lambda: (d.batch_i16(buf.ptr, 2 * L, L), d.sync()), a.warmup, a.steps)
    d2 = J.BpskChannels(RATE, 8192, [375.0 * (32 + 8 * c) for c in range(16)], ninputs=1, max_batch_samples=L)
    one_p = timed(lambda: (d2.batch_i16(buf.ptr, 2 * L, L), d2.sync()), a.warmup, a.steps)
    out["k16_1input_nonperiodic_ms"] = round(one, 3)
    out["k16_1input_periodic_ms"] = round(one_p, 3)
    del d, d2
    # drop-in latency
    frame = 2048
    x = rng.integers(-12000, 12000, 2 * frame * a.frames, dtype=np.int16)
    ch = J.BpskChannels(RATE, 4 * frame, [12000, 24000])
    ones = [J.Bpsk(rate=RATE, blen=4 * frame, tuning=t) for t in (12000, 24000)]
    it = {"k": 0}

    def rx_ch():
        f = it["k"] % a.frames
        ch.receive_raw(x[2 * f * frame:2 * (f + 1) * frame])
        it["k"] += 1

    def rx_two():
        f = it["k"] % a.frames
        for o in ones:
            o.receive_raw(x[2 * f * frame:2 * (f + 1) * frame])
        it["k"] += 1
    out["receive_2ch_us"] = round(1e3 * timed(rx_ch, 10, a.frames), 1)
    out["receive_two_1stream_us"] = round(1e3 * timed(rx_two, 10, a.frames), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
