#!/usr/bin/env python3
"""Writes tests/golden/bpsk_checkpoint_v1.bin: the blob that pins checkpoint format version 1.  Run on an MI355X; the file is
what the library saves there and is never edited by hand.

    python tools/make_checkpoint_golden.py [output path]

The blob: a 2-stream handle of jsdr_bpsk_create (96 kHz, 2-sample frames, tuning 12000 Hz, the tune mode), stream s fed the
first 40000 samples of make_dbpsk_stream(777, s, 65536) in one call, then save(0, 2).  tests/test_gpu_bpsk_checkpoint.py restores
it, feeds the other 25536 samples and compares with the oracle fed all 65536."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import java_sdr_amd as J  # noqa: E402
import oracle_lib as O  # noqa: E402

SEED, N, CUT = 777, 65536, 40000


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "bpsk_checkpoint_v1.bin")
    xs = [O.make_dbpsk_stream(SEED, s, N)[0] for s in range(2)]
    d_iq = J.DeviceBuffer.from_host(np.concatenate(xs))
    d = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=2, max_batch_samples=N)
    d.batch_i16(d_iq.ptr, 2 * N, CUT)
    blob = d.save(0, 2)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "wb") as f:
        f.write(blob)
    print(out, len(blob), J.blob_info(blob))


if __name__ == "__main__":
    main()
