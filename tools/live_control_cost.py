"""the cost of a live-control action and of the call after it (k_front_split and the mode seams):
python tools/live_control_cost.py [streams=1024] [log2 samples per call=17]

One batch handle at 96 kHz / 2048-sample frames, jsdr_bpsk_profile_* events around every call: the GPU time of the call's
kernels, its wall time with a sync, and the front-end kernel it launched; the host time of each action."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np
import java_sdr_amd as J
import oracle_lib as O

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
L = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 17)
iq = J.DeviceBuffer.from_host(np.tile(O.make_dbpsk_stream(7, 1, L)[0], S))
d = J.Bpsk(nstreams=S, max_batch_samples=L)
d.profile_enable(True)


def call(tag):
    d.sync()
    t = time.perf_counter()
    d.batch_i16(iq.ptr, 2 * L, L)
    d.sync()
    wall = (time.perf_counter() - t) * 1e3
    prof = {k: v for k, v in d.profile_read().items() if v[1]}
    print(f"{tag:30s} kernels {sum(v[0] for v in prof.values()):7.3f} ms  wall {wall:7.3f} ms  front {d.front_kernel_name()}"
          f"  ({prof.get('k_front', (0.0,))[0]:.3f} ms in k_front's slot)", flush=True)


def action(tag, fn):
    t = time.perf_counter()
    fn()
    print(f"{tag:30s} host {(time.perf_counter() - t) * 1e3:7.3f} ms", flush=True)


print(f"{S} streams x {L} samples a call")
for _ in range(3):
    call("steady, 12000 Hz")
action("set_tuning(12010)", lambda: d.set_tuning(12010.0))
call("first after +10 Hz")
call("second after +10 Hz")
action("set_tuning(-300)", lambda: d.set_tuning(-300.0))
call("crossing 0 downward")
call("after it")
action("set_tuning(12000)", lambda: d.set_tuning(12000.0))
call("crossing 0 upward")
call("after it")
action("set_mode(1, 0), first time", lambda: d.set_mode(1, 0))
call("first FFT-acquire call (seam)")
call("second FFT-acquire call")
action("set_mode(0, 0)", lambda: d.set_mode(0, 0))
call("first tune call (seam)")
call("second tune call")
