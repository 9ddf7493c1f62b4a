#!/usr/bin/env python3
"""Fused jsdr_fft_waterfall_i16 against jsdr_fft_batch_i16 + jsdr_waterfall_lines on the same buffers; one JSON line a shape.

--frames frames of 2048 int16 samples (synthetic tones, jsdr_synth_tones) at each of --widths: the pair, the fused call and the
pair's two kernels alone, alternating, --windows windows of --calls calls each between two HIP events (median, min, max in ms a
call); then every 4099th pixel row of the two forms compared.  The figures of DESIGN.md section 7 "k_fft_pix" are

    python tools/fft_waterfall_bench.py --frames 524288 --widths 1024 512 --calls 8
    python tools/fft_waterfall_bench.py --frames 4194304 --widths 1024 --calls 2"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import java_sdr_amd as J  # noqa: E402
import oracle_lib as O  # noqa: E402  (the generator's cosine table)

N, RATE = 2048, 96000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 19)
    ap.add_argument("--widths", type=int, nargs="+", default=[1024, 512])
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--calls", type=int, default=8)
    a = ap.parse_args()
    nf, wmax = a.frames, max(a.widths)
    ct, _ = O.synth_tables(6000)
    d_ct = J.DeviceBuffer.from_host(ct)
    d_iq = J.DeviceBuffer(nf * N * 4)
    J.synth_tones(d_iq, 0, nf, N, d_ct, 250, O.mix64(7))
    d_psd = J.DeviceBuffer(nf * (N + 2) * 4)
    d_pair, d_fused = J.DeviceBuffer(nf * wmax * 4), J.DeviceBuffer(nf * wmax * 4)
    J.binding.stream_sync()
    f = J.Fft(N, RATE)
    t = J.Timer()

    def timed(fn):
        t.start()
        for _ in range(a.calls):
            fn()
        t.stop()
        return t.elapsed_ms() / a.calls

    for width in a.widths:
        forms = {
            "fft": lambda: f.batch_i16(d_iq, nf, d_psd),
            "waterfall": lambda: J.waterfall_lines_dev(d_psd, nf, N, width, d_pair),
            "fused": lambda: f.waterfall_i16(d_iq, nf, width, d_fused),
        }
        forms["pair"] = lambda: (forms["fft"](), forms["waterfall"]())
        for _ in range(3):
            forms["pair"]()
            forms["fused"]()
        J.binding.stream_sync()
        ms = {k: [] for k in ("pair", "fused", "fft", "waterfall")}
        for _ in range(a.windows):
            for k in ms:
                ms[k].append(timed(forms[k]))
        same = all(np.array_equal(d_pair.to_host(np.uint32, width, offset_bytes=k * width * 4),
                                  d_fused.to_host(np.uint32, width, offset_bytes=k * width * 4)) for k in range(0, nf, 4099))
        row = {"n": N, "frames": nf, "width": width, "kernel": f.waterfall_kernel(), "same_pixels": bool(same)}
        for k, v in ms.items():
            row[k + "_ms"] = [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
