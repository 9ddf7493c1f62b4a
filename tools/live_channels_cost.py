"""the cost of a live "FFT/Tune" switch of one channel of a live channel handle ("k_chan_seam_hist,
k_acq_edges_seam"): python tools/live_channels_cost.py [inputs=256] [log2 samples per call=17]

One jsdr_bpsk_create_live_channels handle of `inputs` x 4 channels at 96 kHz / 2048-sample frames, and as the yardstick, in the
same run, four ordinary handles of `inputs` streams each, created with the four channels' configurations and given
jsdr_bpsk_set_mode at the same points.  jsdr_bpsk_profile_* events around every call's kernels, the host clock around each
action and around each call (with a sync).  Run it as one process under its own timeout."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
import java_sdr_amd as J
import oracle_lib as O

NIN = int(sys.argv[1]) if len(sys.argv) > 1 else 256
L = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 17)
RATE, FRAME = 96000, 2048
CHANNELS = [(12000, 0, 0), (12000, 1, 0), (12000, 1, 1), (30000, 0, 0)]  # the switched channel is channel 0

iq = J.DeviceBuffer.from_host(np.tile(O.make_dbpsk_stream(7, 1, L, rate=RATE, carrier_hz=13200.0)[0], NIN))
d = J.BpskChannels(RATE, 4 * FRAME, [t for t, _, _ in CHANNELS], do_up=[u for _, _, u in CHANNELS], ninputs=NIN, max_batch_samples=L,
                   do_fft=[f for _, f, _ in CHANNELS], live=True)
refs = [J.Bpsk(rate=RATE, blen=4 * FRAME, tuning=t, do_fft=f, do_up=u, nstreams=NIN, max_batch_samples=L) for t, f, u in CHANNELS]
for h in [d] + refs:
    h.profile_enable(True)


def one(h):
    h.sync()
    t = time.perf_counter()
    h.batch_i16(iq.ptr, 2 * L, L)
    h.sync()
    wall = (time.perf_counter() - t) * 1e3
    prof = {k: v for k, v in h.profile_read().items() if v[1]}
    return sum(v[0] for v in prof.values()), wall, prof


def call(tag):
    k, w, prof = one(d)
    rk, rw = 0.0, 0.0
    for r in refs:
        a, b, _ = one(r)
        rk += a
        rw += b
    print(f"{tag:34s} channels: kernels {k:8.3f} ms wall {w:8.3f} ms front {d.front_kernel_name():14s} | four ordinary: kernels {rk:8.3f} ms "
          f"wall {rw:8.3f} ms", flush=True)
    print("    " + "  ".join(f"{n} {v[0]:.3f}/{v[1]}" for n, v in sorted(prof.items())), flush=True)


def action(tag, fn, ref_fn):
    d.sync()
    t = time.perf_counter()
    fn()
    host = (time.perf_counter() - t) * 1e3
    refs[0].sync()
    t = time.perf_counter()
    ref_fn()
    print(f"{tag:34s} channels: host {host:8.3f} ms | ordinary: host {(time.perf_counter() - t) * 1e3:8.3f} ms", flush=True)


print(f"{NIN} inputs x {len(CHANNELS)} channels x {L} samples a call, frames of {FRAME}")
for _ in range(3):
    call("steady (2 tune + 2 FFT channels)")
action("channel 0 -> FFT-acquire", lambda: d.set_channel_mode(0, 1, 0), lambda: refs[0].set_mode(1, 0))
call("first call after tune -> FFT")
call("second call after tune -> FFT")
call("steady (1 tune + 3 FFT channels)")
action("channel 0 -> tune", lambda: d.set_channel_mode(0, 0, 0), lambda: refs[0].set_mode(0, 0))
call("first call after FFT -> tune")
call("second call after FFT -> tune")
call("steady (2 tune + 2 FFT channels)")
