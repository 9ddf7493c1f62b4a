#!/usr/bin/env python3
"""The batched phase scope (jsdr_phase_scope_i16) timed against what the library offered for the same device-resident int16
frames before it; one JSON line a part.  Not part of bench.py.

  --frames frames of 2048 int16 samples (default 2^19: 4 GiB, well past the 256 MB cache), packed and as --streams streams at a
  stride of 2 x frames-per-stream x 2n, for bx in --bx (default 0, 512, 2048):
    scope      one jsdr_phase_scope_i16 launch: max, column means and plot points;
    baseline   jsdr_convert_i16 into a float copy + jsdr_phase_maxabs (the part every bx needs), and for bx > 0 the blocking
               jsdr_phase_columns timed over --columns-frames frames (host clock: the call synchronises) and SCALED to all frames
               -- an extrapolation, marked as such; scaling the means on the host is not counted at all;
    psd        jsdr_fft_batch_i16 over the same packed frames: the read rate the scope's bx = 0 is expected to come near.

Device events, --warmup warm-ups, the median of --reps calls; the algorithmic traffic is 4 B a sample in and 4 + 24 ncol B a frame
out.  The figures of DESIGN.md section 7 "The phase scope in one launch" are

    python tools/ab_phase_scope.py"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import java_sdr_amd as J  # noqa: E402
import oracle_lib as O  # noqa: E402  (the generator's cosine table)

N, RATE, HALF, QUARTER = 2048, 96000, 300, 137


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 19)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--bx", type=int, nargs="*", default=[0, 512, 2048])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--columns-frames", type=int, default=64)
    a = ap.parse_args()
    nf, S = a.frames, a.streams
    assert nf % S == 0
    F = nf // S
    stride = 2 * F * 2 * N
    ct, _ = O.synth_tables(6000)
    d_ct = J.DeviceBuffer.from_host(ct)
    d_pk = J.DeviceBuffer(2 * nf * 2 * N)
    d_str = J.DeviceBuffer(2 * S * stride)
    J.synth_tones(d_pk, 0, nf, N, d_ct, 250, O.mix64(7))
    for s in range(S):  # the same frames in both layouts
        J.synth_tones(d_str.ptr + 2 * s * stride, s * F, F, N, d_ct, 250, O.mix64(7))
    J.binding.stream_sync()
    t = J.Timer()
    P = J.Phase(N)
    lib = J.lib()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        J.binding.stream_sync()
        ms = []
        for _ in range(a.reps):
            t.start()
            fn()
            t.stop()
            ms.append(t.elapsed_ms())
        return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]

    d_max = J.DeviceBuffer(4 * nf)
    in_bytes = nf * 2 * N * 2
    for bx in a.bx:
        ncol = J.phase_layout(N, bx)[0].size
        d_avg = J.DeviceBuffer(8 * nf * ncol) if ncol else None
        d_pts = J.DeviceBuffer(16 * nf * ncol) if ncol else None
        out_bytes = nf * (4 + 24 * ncol)
        ref = None
        for name, src, ns, st, fps in (("packed", d_pk, 1, 0, nf), ("strided", d_str, S, stride, F)):
            ms = timed(lambda: P.scope_i16(src, ns, st, fps, 0, 0, bx, HALF, QUARTER, d_max, d_avg, d_pts))
            got = [d_max.to_host(np.uint32, 4096)] + [d.to_host(np.uint32, 4096 * k) for d, k in ((d_avg, 2), (d_pts, 4)) if d is not None]
            same = ref is None or all(np.array_equal(x, y) for x, y in zip(got, ref))
            ref = got
            print(json.dumps({"part": "scope", "layout": name, "n": N, "frames": nf, "bx": bx, "ncol": ncol, "ms": ms,
                              "kernel": P.scope_kernel(), "in_GB": round(in_bytes / 1e9, 3), "out_GB": round(out_bytes / 1e9, 3),
                              "TB_per_s": round((in_bytes + out_bytes) / ms[0] / 1e9, 3), "same_rows_as_packed": bool(same)}), flush=True)
        for d in (d_avg, d_pts):
            if d is not None:
                d.free()
    # the baseline: a float copy and the float max kernel (every bx), the blocking per-frame columns call (bx > 0)
    d_f = J.DeviceBuffer(4 * nf * 2 * N)

    def convert_max():
        J.binding._check(lib.jsdr_convert_i16(C.c_void_p(d_pk.ptr), C.c_int64(nf * N), 2, 0, 0, C.c_void_p(d_f.ptr), None), "convert")
        J.binding._check(lib.jsdr_phase_maxabs(C.c_void_p(d_f.ptr), C.c_int64(nf), N, C.c_void_p(d_max.ptr), None), "maxabs")

    base = timed(convert_max)
    print(json.dumps({"part": "baseline", "what": "convert_i16 + phase_maxabs", "frames": nf, "ms": base,
                      "bytes_GB": round((in_bytes + 2 * 2 * in_bytes + 4 * nf) / 1e9, 3)}), flush=True)
    cap = N + 1
    pix, ai, aq, ncol = np.empty(cap, np.int32), np.empty(cap, np.float32), np.empty(cap, np.float32), C.c_int()
    for bx in a.bx:
        if bx == 0:
            continue
        k = a.columns_frames

        def columns():
            for f in range(k):
                J.binding._check(lib.jsdr_phase_columns(C.c_void_p(d_f.ptr + 8 * N * f), N, bx, J.binding._addr(pix), J.binding._addr(ai),
                                                        J.binding._addr(aq), cap, C.byref(ncol)), "columns")

        columns()
        w = []
        for _ in range(5):
            t0 = time.perf_counter()
            columns()
            w.append((time.perf_counter() - t0) * 1e3)
        per_frame = statistics.median(w) / k
        print(json.dumps({"part": "baseline", "what": "phase_columns, a blocking call a frame", "bx": bx, "frames_timed": k,
                          "ms_per_frame": round(per_frame, 4), "EXTRAPOLATED_ms_all_frames": round(per_frame * nf, 1),
                          "EXTRAPOLATED_plus_convert_max_ms": round(per_frame * nf + base[0], 1)}), flush=True)
    d_f.free()
    # the PSD kernel over the same packed frames
    f = J.Fft(N, RATE)
    d_psd = J.DeviceBuffer(4 * nf * (N + 2))
    ms = timed(lambda: f.batch_i16(d_pk, nf, d_psd))
    print(json.dumps({"part": "psd", "kernel": f.kernel_name(), "frames": nf, "ms": ms, "in_GB": round(in_bytes / 1e9, 3),
                      "read_TB_per_s": round(in_bytes / ms[0] / 1e9, 3), "TB_per_s": round((in_bytes + 4 * nf * (N + 2)) / ms[0] / 1e9, 3)}),
          flush=True)


if __name__ == "__main__":
    main()
