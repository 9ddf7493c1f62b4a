#!/usr/bin/env python3
"""The demod scope (jsdr_demod_scope_i16) timed beside the batch call it contains; one JSON line a part.  Not part of bench.py.

  --streams x --samples int16 IQ (default 1024 x 2^20: 4 GiB in, 4 GiB of audio out), frames of --n samples (2048), NFM with
  filter, mixer and AGC on, a panel --width (1024) by --height (400):
    batch        jsdr_demod_batch_i16
    scope_all    jsdr_demod_scope_i16 with trace, spectrum and dbg rows
    scope_trace  trace rows alone
    scope_spec   spectrum rows alone
Timed with jsdr_timer_* (device events on the null stream), --warmup warm-ups, then the best of --reps (5) calls, all of them
listed.  The figures of DESIGN.md section 7 "The demod scope" are

    python tools/ab_demod_scope.py"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import java_sdr_amd as J  # noqa: E402
import oracle_lib as O  # noqa: E402  (the generator's cosine table)

RATE, MODE_NFM, BAND = 96000, 3, (3000, 11000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=0, help="jsdr_demod_scope_chunk (0: the default)")
    a = ap.parse_args()
    S, L, n, W, H = a.streams, a.samples, a.n, a.width, a.height
    assert L % n == 0
    rows = S * (L // n)
    ct, _ = O.synth_tables(6000)
    d_ct = J.DeviceBuffer.from_host(ct)
    d_in = J.DeviceBuffer(4 * S * L)
    J.synth_tones(d_in, 0, rows, n, d_ct, 250, O.mix64(7))
    d_audio = J.DeviceBuffer(4 * S * L)
    d_trace = J.DeviceBuffer(4 * rows * W)
    d_spec = J.DeviceBuffer(4 * rows * W)
    d_dbg = J.DeviceBuffer(8 * S * L)
    J.binding.stream_sync()
    h = J.Demod(RATE, n, S, L)
    h.configure(MODE_NFM, 1, 1, 1)
    h.weights(*BAND)
    h.scope_chunk(a.chunk)
    t = J.Timer()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        J.binding.stream_sync()
        ms = []
        for _ in range(a.reps):
            t.start()
            fn()
            t.stop()
            ms.append(round(t.elapsed_ms(), 3))
        return ms

    parts = (("batch", lambda: h.batch_i16(d_in, 2 * L, L, d_audio, 2 * L)),
             ("scope_all", lambda: h.scope_i16(d_in, 2 * L, L, d_audio, 2 * L, W, H, d_trace, d_spec, d_dbg)),
             ("scope_trace", lambda: h.scope_i16(d_in, 2 * L, L, d_audio, 2 * L, W, H, trace_dev=d_trace)),
             ("scope_spec", lambda: h.scope_i16(d_in, 2 * L, L, d_audio, 2 * L, W, H, spec_dev=d_spec)))
    base = None
    for name, fn in parts:
        ms = timed(fn)
        if base is None:
            base = min(ms)
        print(json.dumps({"part": name, "streams": S, "samples": L, "n": n, "frames": rows, "width": W, "height": H,
                          "best_ms": min(ms), "ms": ms, "over_batch": round(min(ms) / base, 3),
                          "kernel": h.scope_kernel() if name != "batch" else "", "live": list(J.live_resources())}), flush=True)


if __name__ == "__main__":
    main()
