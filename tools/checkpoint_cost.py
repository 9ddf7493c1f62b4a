#!/usr/bin/env python3
"""What a checkpoint costs: jsdr_bpsk_save and jsdr_bpsk_restore of every stream of a handle, timed with jsdr_timer_*
events around the call and with the host clock, beside a plain copy of the same number of bytes each way (pageable host memory,
as the calls use) and beside the parser alone (jsdr_bpsk_blob_info: the checksum over every byte).  k_state_pack and k_state_unpack are timed
by the library itself, with HIP events around the launch (jsdr_bpsk_state_kernel_ms).

    python tools/checkpoint_cost.py [--streams 8192] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import java_sdr_amd as J  # noqa: E402


def timed(fn, reps):
    """-> (best event ms, best host ms)"""
    ev, host = [], []
    t = J.Timer()
    for _ in range(reps):
        t.start()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
        t.stop()
        ev.append(t.elapsed_ms())
    return min(ev), min(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    S, L = a.streams, 8192
    rng = np.random.default_rng(1)
    row = rng.integers(-8000, 8000, 2 * L).astype(np.int16)
    d_iq = J.DeviceBuffer.from_host(np.tile(row, (S, 1)))
    d = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=S, max_batch_samples=L)
    d.batch_i16(d_iq.ptr, 2 * L, L)
    d.sync()
    nbytes = d.state_bytes(S)
    blob = d.save()
    f = J.Bpsk(rate=96000, blen=8, tuning=12000, nstreams=S, max_batch_samples=L)
    f.restore(blob)
    assert f.save() == blob
    # the C calls themselves, into and out of one host buffer (the binding's own copies are not the library's)
    import ctypes as C
    lib = J.lib()
    buf = np.empty(nbytes, np.uint8)
    got = C.c_size_t()
    ptr = C.c_void_p(buf.ctypes.data)

    def save():
        assert lib.jsdr_bpsk_save(d.h, 0, S, ptr, C.c_size_t(nbytes), C.byref(got)) == 0

    def restore():
        assert lib.jsdr_bpsk_restore(f.h, 0, ptr, C.c_size_t(nbytes)) == 0

    save_ev, save_host = timed(save, a.reps)
    assert buf.tobytes() == blob
    rest_ev, rest_host = timed(restore, a.reps)
    # the kernels by themselves: HIP events around the launch inside the library (the last call's)
    packs, unpacks = [], []
    for _ in range(a.reps):
        save()
        packs.append(d.state_kernel_ms()[0])
        restore()
        unpacks.append(f.state_kernel_ms()[1])
    pack_ms, unpack_ms = min(packs), min(unpacks)
    # the parser alone: the lengths and the checksum over every byte, no device
    info = J.binding.BpskBlobInfo()

    def parse():
        assert lib.jsdr_bpsk_blob_info(ptr, C.c_size_t(nbytes), C.byref(info)) == 0

    _, parse_host = timed(parse, a.reps)
    # the same bytes as plain copies
    dev = J.DeviceBuffer(nbytes)
    hostbuf = np.frombuffer(blob, np.uint8).copy()
    d2h_ev, d2h_host = timed(lambda: dev.to_host(np.uint8), a.reps)
    h2d = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        tmp = J.DeviceBuffer.from_host(hostbuf)
        h2d.append((time.perf_counter() - t0) * 1e3)
        tmp.free()
    print(json.dumps(dict(streams=S, record_bytes=J.blob_info(blob)["record_bytes"], blob_bytes=nbytes,
                          save_ms_events=round(save_ev, 3), save_ms_host=round(save_host, 3),
                          restore_ms_events=round(rest_ev, 3), restore_ms_host=round(rest_host, 3),
                          k_state_pack_ms=round(pack_ms, 3), k_state_unpack_ms=round(unpack_ms, 3),
                          checksum_ms_host=round(parse_host, 3), copy_d2h_ms=round(d2h_host, 3), copy_h2d_ms_with_alloc=round(min(h2d), 3))))


if __name__ == "__main__":
    main()
