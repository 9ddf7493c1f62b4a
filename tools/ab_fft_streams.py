#!/usr/bin/env python3
"""The strided PSD / waterfall calls (jsdr_fft_batch_streams_i16, jsdr_fft_waterfall_streams_i16) timed against what they replace;
one JSON line a part.  Not part of bench.py.

  (a) --streams streams x --frames frames of 2048 int16 samples at --stride int16 values a stream: the strided call against one
      jsdr_fft_batch_i16 launch a stream on the same stream (what a caller with such rows did, and the group did, before);
  (b) the same frames packed: the contiguous call against itself (the session's run-to-run spread), then against the strided
      instantiation forced on the packed rows (JSDR_FFT_STREAMS_FORCE, toggled between windows): the price of the mapping;
  (c) (a) for the fused waterfall at --width.

Forms alternate window by window, --windows windows of --calls calls each between two HIP events; median, min and max in ms a
call.  Every 4099th output row of the two forms of a part is compared.  The figures of DESIGN.md section 7 "raw[stream][stride]" are

    JSDR_KNOBS=1 python tools/ab_fft_streams.py"""
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


def stats(v):
    return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=512, help="frames a stream")
    ap.add_argument("--stride", type=int, default=2 * (2 << 20), help="int16 values between two streams")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    if os.environ.get("JSDR_KNOBS") != "1":
        sys.exit("part (b) forces the strided kernel through JSDR_FFT_STREAMS_FORCE: run with JSDR_KNOBS=1")
    os.environ["JSDR_FFT_STREAMS_FORCE"] = "0"
    S, F, stride, width = a.streams, a.frames, a.stride, a.width
    assert stride % 2 == 0 and stride >= F * 2 * N
    nf, row = S * F, N + 2
    ct, _ = O.synth_tables(6000)
    d_ct = J.DeviceBuffer.from_host(ct)
    d_str = J.DeviceBuffer(2 * S * stride)
    d_pk = J.DeviceBuffer(4 * nf * N)
    for s in range(S):  # the same frames in both layouts
        J.synth_tones(d_str.ptr + 2 * s * stride, s * F, F, N, d_ct, 250, O.mix64(7))
    J.synth_tones(d_pk, 0, nf, N, d_ct, 250, O.mix64(7))
    d_a, d_b = J.DeviceBuffer(4 * nf * row), J.DeviceBuffer(4 * nf * row)
    J.binding.stream_sync()
    f = J.Fft(N, RATE)
    t = J.Timer()

    def timed(fn):
        t.start()
        for _ in range(a.calls):
            fn()
        t.stop()
        return t.elapsed_ms() / a.calls

    def forced(on):
        os.environ["JSDR_FFT_STREAMS_FORCE"] = "1" if on else "0"

    def ab(forms, outs, row_words):
        """alternate the forms; then compare sampled rows of the first and the last form's outputs"""
        for fn in forms.values():
            fn()
        J.binding.stream_sync()
        ms = {k: [] for k in forms}
        for _ in range(a.windows):
            for k, fn in forms.items():
                ms[k].append(timed(fn))
        same = all(np.array_equal(outs[0].to_host(np.uint32, row_words, offset_bytes=4 * k * row_words),
                                  outs[1].to_host(np.uint32, row_words, offset_bytes=4 * k * row_words)) for k in range(0, nf, 4099))
        return {k + "_ms": stats(v) for k, v in ms.items()}, bool(same)

    def per_stream_psd():
        for s in range(S):
            f.batch_i16(d_str.ptr + 2 * s * stride, F, d_a.ptr + 4 * s * F * row)

    def per_stream_pix():
        for s in range(S):
            f.waterfall_i16(d_str.ptr + 2 * s * stride, F, width, d_pa.ptr + 4 * s * F * width)

    base = {"n": N, "streams": S, "frames_per_stream": F, "stride_i16": stride}
    # (a)
    r, same = ab({"per_stream": per_stream_psd, "strided": lambda: f.batch_streams_i16(d_str, S, stride, F, d_b)}, (d_a, d_b), row)
    r["ratio_per_stream_over_strided"] = round(r["per_stream_ms"][0] / r["strided_ms"][0], 3)
    print(json.dumps({"part": "a", **base, **r, "launch": f.last_launch(), "same_rows": same}), flush=True)
    # (b)
    r, same = ab({"contiguous": lambda: (forced(False), f.batch_i16(d_pk, nf, d_a)),
                  "contiguous_again": lambda: (forced(False), f.batch_i16(d_pk, nf, d_a)),
                  "strided_forced": lambda: (forced(True), f.batch_streams_i16(d_pk, S, F * 2 * N, F, d_b))}, (d_a, d_b), row)
    forced(False)
    r["spread_contiguous"] = round(r["contiguous_again_ms"][0] / r["contiguous_ms"][0], 4)
    r["ratio_strided_over_contiguous"] = round(r["strided_forced_ms"][0] / r["contiguous_ms"][0], 4)
    print(json.dumps({"part": "b", **base, **r, "same_rows": same}), flush=True)
    # (c)
    d_a.free()
    d_b.free()
    d_pa, d_pb = J.DeviceBuffer(4 * nf * width), J.DeviceBuffer(4 * nf * width)
    r, same = ab({"per_stream": per_stream_pix, "strided": lambda: f.waterfall_streams_i16(d_str, S, stride, F, width, d_pb)},
                 (d_pa, d_pb), width)
    r["ratio_per_stream_over_strided"] = round(r["per_stream_ms"][0] / r["strided_ms"][0], 3)
    print(json.dumps({"part": "c", **base, "width": width, **r, "kernel": f.waterfall_kernel(), "same_rows": same}), flush=True)


if __name__ == "__main__":
    main()
