#!/usr/bin/env python3
"""jsdr_bpsk_scope_i16 against jsdr_bpsk_batch_i16 on the same handle, in one process; prints one JSON line.

  batch           batch_i16 alone
  all             the scope call with all six outputs
  pts_bits_max    ... with pts, bits and max only
  tuned           ... with tuned only

--spectra: jsdr_bpsk_scope_spectra_i16 instead -- batch, tuned, tspec_tpeak, dspec_dpeak, all_four (the handle's own rows, in passes)
and tuned_tspec_tpeak (the caller's rows), and from the last against `tuned` the green-spectrum kernel's time, bytes/s and FP64 rate.

--streams x --samples at 96 kHz, frames of 2048 samples, tuning 12 000 (default 1024 x 2^20: 512 frames a stream, tuned is 16 GiB).
Per line: wall time of a call plus a sync of the handle and the device, median of --steps after --warmup; `over_batch` is the
line's time less the batch call's.  The input rows repeat every 16 streams."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATE, N = 96000, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--spectra", action="store_true", help="the lines of jsdr_bpsk_scope_spectra_i16 instead (see above)")
    ap.add_argument("--plot-width", type=int, default=749)
    a = ap.parse_args()
    import java_sdr_amd as J
    C = J.binding.C
    S, L = a.streams, a.samples // N * N
    rows = S * (L // N)
    ring = N * 9600 // RATE
    rng = np.random.default_rng(1)
    blk = rng.integers(-12000, 12000, 2 * L * 16, dtype=np.int16)
    buf = J.DeviceBuffer(4 * L * S)
    for r in range(0, S, 16):
        J.lib().jsdr_memcpy_h2d(C.c_void_p(buf.ptr + 4 * L * r), J.binding._addr(blk), C.c_size_t(4 * L * min(16, S - r)))
    J.binding.stream_sync()
    d = J.Bpsk(rate=RATE, blen=4 * N, tuning=12000, nstreams=S, max_batch_samples=L)
    size = dict(tuned=16 * rows * N, ds=16 * rows * ring, iq=16 * rows * ring, max=16 * rows, pts=16 * rows * ring, bits=rows * ring)
    out = {k: J.DeviceBuffer(v) for k, v in size.items()}
    lines = {"batch": None, "all": tuple(size), "pts_bits_max": ("pts", "bits", "max"), "tuned": ("tuned",)}
    if a.spectra:
        Wp = a.plot_width
        size.update(tspec=4 * rows * Wp, tpeak=16 * rows, dspec=4 * rows * Wp, dpeak=16 * rows)
        out.update({k: J.DeviceBuffer(size[k]) for k in ("tspec", "tpeak", "dspec", "dpeak")})
        lines = {"batch": None, "tuned": ("tuned",), "tspec_tpeak": ("tspec", "tpeak"), "dspec_dpeak": ("dspec", "dpeak"),
                 "all_four": ("tspec", "tpeak", "dspec", "dpeak"), "tuned_tspec_tpeak": ("tuned", "tspec", "tpeak")}
    res = {"streams": S, "samples_per_call": L, "rate": RATE, "frame": N, "rows": rows}
    for name, outs in lines.items():
        if outs is None:
            call = lambda: d.batch_i16(buf.ptr, 2 * L, L)  # noqa: E731
        elif a.spectra:
            kw = {k: out[k].ptr for k in outs}
            call = lambda kw=kw: d.scope_spectra_i16(buf.ptr, 2 * L, L, plot_width=a.plot_width, **kw)  # noqa: E731
        else:
            kw = {k: out[k].ptr for k in outs}
            call = lambda kw=kw: d.scope_i16(buf.ptr, 2 * L, L, **kw)  # noqa: E731
        ts = []
        for k in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            call()
            d.sync()
            J.binding.stream_sync()
            if k >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"ms": round(statistics.median(ts), 3), "kernels": d.scope_kernel() if outs else ""}
    for name in lines:
        if name != "batch":
            res[name]["over_batch_ms"] = round(res[name]["ms"] - res["batch"]["ms"], 3)
    if a.spectra:
        # the green-spectrum kernel over the caller's rows in HBM: what the call with tuned + tspec + tpeak takes over tuned alone.
        # A row of n = 2^k points: 16 n bytes read; log2 n stages of n / 2 butterflies of 10 FP64 operations, 3 n for the magnitudes
        ms = res["tuned_tspec_tpeak"]["ms"] - res["tuned"]["ms"]
        logn = N.bit_length() - 1
        res["green_kernel"] = {"ms": round(ms, 3), "read_GBps": round(16 * N * rows / ms / 1e6, 1),
                               "fp64_GFLOPs": round((5 * N * logn + 3 * N) * rows / ms / 1e6, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
