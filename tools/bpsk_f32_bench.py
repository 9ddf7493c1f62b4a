#!/usr/bin/env python3
"""jsdr_bpsk_batch_f32 in the tune mode: the fused float kernel against the three-kernel float path and against the int16
form; prints one JSON line.

  (a) batch_f32, the fused float kernel (k_fm_f32)
  (b) batch_f32 under JSDR_KNOBS=1 JSDR_FM=0: k_front<F32IN> + k_matched + k_dm_history, dm through HBM and back
  (c) batch_i16 on the same streams (k_fm): the floor -- a float kernel reads twice the bytes

--streams x --samples at 96 kHz, tuning 12 000.  Per line: wall time of a call plus a sync of the handle, median of --steps
after --warmup, and the per-kernel HIP-event times (jsdr_bpsk_profile_*) of one more call.  Each line runs in a child
process of its own (the knob is read when the library loads); --line a|b|c runs one line in this process (for a profiler
run: rocprofv3 --pmc FETCH_SIZE -- python tools/bpsk_f32_bench.py --line a)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATE = 96000


def one_line(line, N, L, warmup, steps):
    import java_sdr_amd as J
    C = J.binding.C
    f32 = line != "c"
    rng = np.random.default_rng(1)
    raw = rng.integers(-12000, 12000, 2 * L * 16, dtype=np.int16)
    # the input: N rows of L samples (rows repeat every 16); floats off the int16 grid
    blk = (raw.astype(np.float32) / np.float32(32767.0) * np.float32(0.93)).astype(np.float32) if f32 else raw
    row = (8 if f32 else 4) * L
    buf = J.DeviceBuffer(row * N)
    for r in range(0, N, 16):
        rows = min(16, N - r)
        J.lib().jsdr_memcpy_h2d(C.c_void_p(buf.ptr + row * r), J.binding._addr(blk), C.c_size_t(row * rows))
    J.binding.stream_sync()
    d = J.Bpsk(rate=RATE, blen=8192, tuning=12000, nstreams=N, max_batch_samples=L)
    call = (lambda: (d.batch_f32(buf.ptr, 2 * L, L), d.sync())) if f32 else (lambda: (d.batch_i16(buf.ptr, 2 * L, L), d.sync()))
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    d.profile_enable(True)
    call()
    prof = {k: round(ms, 3) for k, (ms, n) in d.profile_read().items() if n}
    return {"ms": round(statistics.median(ts), 3), "front": d.front_kernel_name(), "kernels_ms": prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--line", default="", help="a, b or c: that line alone, in this process (b: set JSDR_KNOBS=1 JSDR_FM=0 yourself)")
    a = ap.parse_args()
    if a.line:
        print(json.dumps(one_line(a.line, a.streams, a.samples, a.warmup, a.steps)))
        return
    out = {"streams": a.streams, "samples_per_call": a.samples, "rate": RATE, "tuning": 12000}
    names = {"a": "f32_fused", "b": "f32_three_kernel", "c": "i16_fused"}
    for line in "abc":
        env = dict(os.environ)
        if line == "b":
            env.update(JSDR_KNOBS="1", JSDR_FM="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--line", line, "--streams", str(a.streams), "--samples", str(a.samples),
                            "--warmup", str(a.warmup), "--steps", str(a.steps)], env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"line ({line}) failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        out[names[line]] = json.loads(r.stdout.strip().split("\n")[-1])
    out["fused_over_three_kernel"] = round(out["f32_fused"]["ms"] / out["f32_three_kernel"]["ms"], 3)
    out["f32_over_i16"] = round(out["f32_fused"]["ms"] / out["i16_fused"]["ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
