#!/usr/bin/env python3
"""Demod channel handle (jsdr_demod_create_channels) against ordinary handles; prints one JSON line.

  * (a) one channel handle of K channels over --inputs inputs against (b) K ordinary handles of --inputs streams fed the same
    input, K in {1, 2, 8, 16}; NFM and AM, filter, down-conversion and AGC on, each channel its own band (so its own carrier
    table), 2048-sample frames at 96 kHz, 2^20 samples a call
  * (c) one-frame receive_f32 of a 2-channel handle against two 1-stream handles

Wall time per call: the call(s) plus a device sync, median of --steps after --warmup.  The host's carrier recurrences are
inside that time.  --only k=K,mode=M,form=chan|ord runs one configuration (for a rocprofv3 --pmc FETCH_SIZE run) and adds
the handles' per-kernel HIP-event times of the timed calls (jsdr_demod_profile_*).  --frame: samples per frame."""
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
N = 2048


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def band(c):
    return 1000 + 1500 * c, 8000 + 1500 * c


def make(form, K, nin, L, mode):
    if form == "chan":
        d = J.DemodChannels(RATE, N, nin, K, L)
        for c in range(K):
            d.configure_channel(c, mode, 1, 1, 1)
            d.channel_weights(c, *band(c))
        return [d]
    hs = []
    for c in range(K):
        h = J.Demod(RATE, N, nin, L)
        h.configure(mode, 1, 1, 1)
        h.weights(*band(c))
        hs.append(h)
    return hs


def runner(hs, inp, out, nin, L):
    def run():
        if len(hs) == 1 and isinstance(hs[0], J.DemodChannels):
            hs[0].batch_i16(inp.ptr, 2 * L, L, out.ptr, 2 * L)
        else:
            for c, h in enumerate(hs):  # handle c writes the rows channel c would
                h.batch_i16(inp.ptr, 2 * L, L, out.ptr + c * nin * 4 * L, 2 * L)
        J.binding.stream_sync()
    return run


def main():
    global N
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=128)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--ks", default="1,2,8,16")
    ap.add_argument("--modes", default="3,2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--only", default="")
    ap.add_argument("--frame", type=int, default=N)
    a = ap.parse_args()
    N = a.frame
    nin, L = a.inputs, a.samples - a.samples % a.frame  # whole frames
    ks = [int(k) for k in a.ks.split(",")]
    rng = np.random.default_rng(1)
    inp = J.DeviceBuffer.from_host(rng.integers(-12000, 12000, (nin, 2 * L), dtype=np.int16))
    out = J.DeviceBuffer(max(ks) * nin * 4 * L)
    res = {"inputs": nin, "samples_per_call": L, "rate": RATE, "frame": N}
    if a.only:
        kv = dict(x.split("=") for x in a.only.split(","))
        K, mode = int(kv["k"]), int(kv["mode"])
        hs = make(kv["form"], K, nin, L, mode)
        run = runner(hs, inp, out, nin, L)
        for _ in range(a.warmup):
            run()
        for h in hs:
            h.profile_read()
            h.profile_enable(True)
        res["only_ms"] = round(timed(run, 0, a.steps), 3)
        kms = {}
        for h in hs:
            for k, (ms, cnt) in h.profile_read().items():
                if cnt:
                    kms[k] = kms.get(k, 0.0) + ms / a.steps
        res["kernel_ms_per_call"] = {k: round(v, 3) for k, v in kms.items()}
        print(json.dumps(res))
        return
    for mode in [int(m) for m in a.modes.split(",")]:
        name = {2: "am", 3: "nfm"}.get(mode, f"mode{mode}")
        for K in ks:
            for form in ("chan", "ord"):
                hs = make(form, K, nin, L, mode)
                res[f"{name}_k{K}_{form}_ms"] = round(timed(runner(hs, inp, out, nin, L), a.warmup, a.steps), 3)
                del hs
    # drop-in latency: a 2-channel receive against two 1-stream receives
    x = (rng.standard_normal((a.frames, 2 * N)) * 0.3).astype(np.float32)
    ch = J.DemodChannels(RATE, N, 1, 2)
    ones = [J.Demod(RATE, N, 1) for _ in range(2)]
    for c in range(2):
        ch.configure_channel(c, 3, 1, 1, 1)
        ch.channel_weights(c, *band(c))
        ones[c].configure(3, 1, 1, 1)
        ones[c].weights(*band(c))
    it = {"k": 0}

    def rx_ch():
        ch.receive(x[it["k"] % a.frames])
        it["k"] += 1

    def rx_two():
        for o in ones:
            o.receive(x[it["k"] % a.frames])
        it["k"] += 1

    res["receive_2ch_us"] = round(1e3 * timed(rx_ch, 10, a.frames), 1)
    res["receive_two_1stream_us"] = round(1e3 * timed(rx_two, 10, a.frames), 1)
    res["receive_one_1stream_us"] = round(1e3 * timed(lambda: ones[0].receive(x[0]), 10, a.frames), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
