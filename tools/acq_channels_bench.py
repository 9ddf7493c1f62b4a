#!/usr/bin/env python3
"""FFT-acquire channels of one channel handle (jsdr_bpsk_create_mode_channels) against ordinary FFT-acquire handles on the
same inputs; prints one JSON line.

  * (a) ONE channel handle of S / K inputs x K FFT-acquire channels, bands alternating (lower, upper, lower, ...)
  * (b) K ordinary FFT-acquire handles of S / K streams each over the same inputs, with those bands, called one after the other
  * K in {1, 2, 4}, frames of 2048 and 9600 samples, 96 kHz, 2^20 samples a call (whole frames of it), S = 1024: (b) at K = 1
    is a full grid
  * one-frame receive_i16 of a 2-channel handle (both bands) against two 1-stream FFT-acquire handles

Wall time: the call(s) plus a sync, median of --steps after --warmup.  Per-kernel times: one more call of each configuration
under jsdr_bpsk_profile_* (HIP events around every launch).  Counters are a separate rocprofv3 --pmc run."""
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


def kernels(handles, call):
    """{kernel: ms} of one call, summed over the handles"""
    for h in handles:
        h.profile_enable(True)
        h.profile_read()
    call()
    acc = {}
    for h in handles:
        for k, (ms, cnt) in h.profile_read().items():
            if cnt:
                acc[k] = round(acc.get(k, 0.0) + ms, 3)
        h.profile_enable(False)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--ks", default="1,2,4")
    ap.add_argument("--frames", default="2048,9600")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rx-frames", type=int, default=200)
    ap.add_argument("--only", default="", help="form=a|b,k=K,n=FRAME: one configuration (for a profiler run)")
    a = ap.parse_args()
    S = a.streams
    rng = np.random.default_rng(1)
    blk = rng.integers(-12000, 12000, 2 * a.samples * 16, dtype=np.int16)
    buf = J.DeviceBuffer(4 * a.samples * S)
    for r in range(0, S, 16):  # rows repeat every 16
        J.lib().jsdr_memcpy_h2d(J.binding.C.c_void_p(buf.ptr + 4 * a.samples * r), J.binding._addr(blk),
                                J.binding.C.c_size_t(blk.nbytes))
    J.binding.stream_sync()
    out = {"streams": S, "samples_per_call": a.samples, "rate": RATE, "cases": []}
    only = dict(x.split("=") for x in a.only.split(",")) if a.only else None
    for n in [int(v) for v in a.frames.split(",")]:
        L = (a.samples // n) * n
        for K in [int(v) for v in a.ks.split(",")]:
            if only and (int(only["k"]) != K or int(only["n"]) != n):
                continue
            nin = S // K
            case = {"frame": n, "K": K, "inputs": nin, "frames_per_call": L // n}
            if not only or only["form"] == "a":
                d = J.BpskChannels(RATE, 4 * n, [12000.0] * K, do_up=[c & 1 for c in range(K)], ninputs=nin, max_batch_samples=L,
                                   do_fft=[1] * K)
                call = lambda: (d.batch_i16(buf.ptr, 2 * a.samples, L), d.sync())  # noqa: E731
                case["a_ms"] = round(timed(call, a.warmup, a.steps), 3)
                case["a_fwd_inv_frames"] = d.acq_last_launch()
                case["a_front"] = d.front_kernel_name()
                case["a_kernels"] = kernels([d], call)
                del d
            if not only or only["form"] == "b":
                hs = [J.Bpsk(rate=RATE, blen=4 * n, tuning=12000, do_fft=1, do_up=c & 1, nstreams=nin, max_batch_samples=L)
                      for c in range(K)]
                call = lambda: ([h.batch_i16(buf.ptr, 2 * a.samples, L) for h in hs], [h.sync() for h in hs])  # noqa: E731
                case["b_ms"] = round(timed(call, a.warmup, a.steps), 3)
                case["b_front"] = hs[0].front_kernel_name()
                case["b_kernels"] = kernels(hs, call)
                del hs
            out["cases"].append(case)
    if not only:
        frame = 2048
        x = rng.integers(-12000, 12000, 2 * frame * a.rx_frames, dtype=np.int16)
        ch = J.BpskChannels(RATE, 4 * frame, [12000.0, 12000.0], do_up=[0, 1], do_fft=[1, 1])
        ones = [J.Bpsk(rate=RATE, blen=4 * frame, tuning=12000, do_fft=1, do_up=u) for u in (0, 1)]
        it = {"k": 0}

        def rx_ch():
            f = it["k"] % a.rx_frames
            ch.receive_raw(x[2 * f * frame:2 * (f + 1) * frame])
            it["k"] += 1

        def rx_two():
            f = it["k"] % a.rx_frames
            for o in ones:
                o.receive_raw(x[2 * f * frame:2 * (f + 1) * frame])
            it["k"] += 1
        out["receive_2ch_us"] = round(1e3 * timed(rx_ch, 10, a.rx_frames), 1)
        out["receive_two_1stream_us"] = round(1e3 * timed(rx_two, 10, a.rx_frames), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
