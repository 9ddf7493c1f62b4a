"""GPU: every handle gives back what it holds.  jsdr_live_resources counts, process-wide, the device buffers (and their bytes),
pinned buffers and streams + events that the library's owning types (csrc/common.h) hold at the moment; here each kind of
handle is created, used for a call or two and destroyed, and all four counts must be back where they were -- after a destroy,
after a create that failed half way, after the calls that work in buffers of their own, and after twenty create / destroy cycles.
That the create RAISED the counts is asserted too: a counter that never moves would pass everything else.

Every shape is the smallest that allocates what the case is about; a case takes about a second."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):  # (the child process of the recovery case starts without conftest.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import java_sdr_amd as J  # noqa: E402
from fixture_cases import STREAMS, stream_input  # noqa: E402

pytestmark = pytest.mark.gpu
BUFS, BYTES, PINNED, OBJECTS = range(4)
L = 4096  # samples a call and a stream: two 2048-sample frames


def live():
    gc.collect()  # (a handle another test left in a reference cycle goes now, not inside a case)
    return J.live_resources()


def iq16(rows, n=L, seed=5):
    return np.random.default_rng(seed).integers(-3000, 3000, (rows, 2 * n), dtype=np.int16)


def run_batches(d, rows, calls=1, n=L):
    x = J.DeviceBuffer.from_host(iq16(rows, n))
    for _ in range(calls):
        d.batch_i16(x, 2 * n, n)
    d.sync()


# ------------------------------------------------------------------------------------------------ the families
def plain_bpsk():
    d = J.Bpsk(nstreams=2, max_batch_samples=L)
    run_batches(d, 2, calls=2)
    return d


def fft_acquire_bpsk():  # two frames a call: the three-phase front end's scratch comes with the first call
    d = J.Bpsk(do_fft=1, nstreams=2, max_batch_samples=L)
    run_batches(d, 2, calls=2)
    return d


def bpsk_switched_to_fft():  # a live tune -> FFT switch allocates the FFT-acquire buffers and the seam's scratch
    d = J.Bpsk(nstreams=2, max_batch_samples=L)
    run_batches(d, 2)
    before = J.live_resources()
    d.set_mode(1, 0)
    assert J.live_resources()[BUFS] > before[BUFS]
    run_batches(d, 2)
    return d


def channels():
    d = J.BpskChannels(96000, 8192, [12000.0, 9000.0], ninputs=1, max_batch_samples=L)
    run_batches(d, 1)
    return d


def mode_channels():
    d = J.BpskChannels(96000, 8192, [12000.0, 9000.0], do_up=[0, 1], do_fft=[1, 0], ninputs=1, max_batch_samples=L)
    run_batches(d, 1)
    return d


def live_channels():
    d = J.BpskChannels(96000, 8192, [12000.0, 9000.0], do_fft=[0, 1], ninputs=1, max_batch_samples=L, live=True)
    run_batches(d, 1)
    d.set_channel_mode(0, 1, 0)
    run_batches(d, 1)
    return d


def tuned_bpsk():
    d = J.BpskTuned(96000, 8192, [12000.0, 11000.0], max_batch_samples=L)
    run_batches(d, 2)
    return d


def saved_and_restored():  # the records' staging image and the two timing events come with the first save
    d = J.Bpsk(nstreams=2, max_batch_samples=L)
    run_batches(d, 2)
    before = J.live_resources()
    blob = d.save()
    assert J.live_resources()[BUFS] == before[BUFS] + 1 and J.live_resources()[OBJECTS] == before[OBJECTS] + 2
    d.restore(blob)
    run_batches(d, 2)
    return d


def profiled_bpsk():  # the event pool: read once (events back in the pool), then a call whose events are still out at destroy
    d = J.Bpsk(nstreams=2, max_batch_samples=L)
    before = J.live_resources()
    d.profile_enable(True)
    run_batches(d, 2)
    assert J.live_resources()[OBJECTS] > before[OBJECTS]
    assert sum(n for _, n in d.profile_read().values()) > 0
    pooled = J.live_resources()[OBJECTS]
    run_batches(d, 2)
    assert J.live_resources()[OBJECTS] == pooled  # (the second call took its events from the pool)
    return d


def receive_bpsk():  # a 1-stream handle: the pinned arena
    before = J.live_resources()
    d = J.Bpsk(nstreams=1)
    assert J.live_resources()[PINNED] == before[PINNED] + 1
    fr = iq16(1, 2048)[0]
    d.receive_raw(fr)
    d.receive_raw(fr)
    return d


def plain_demod():
    before = J.live_resources()
    d = J.Demod(nstreams=2, max_batch_samples=2048)
    assert J.live_resources()[PINNED] == before[PINNED] + 2  # the two carrier tables
    d.configure(3)
    d.batch_host_i16(iq16(2, 2048), 2048)
    return d


def demod_receive():
    d = J.Demod(nstreams=1)
    d.configure(2)
    d.receive(np.linspace(-1, 1, 4096, dtype=np.float32))  # pins its stage at the first frame
    return d


def demod_channels():
    d = J.DemodChannels(ninputs=1, nchannels=2, max_batch_samples=2048)
    d.configure_channel(0, 2)
    d.configure_channel(1, 3)
    d.batch_host_i16(iq16(1, 2048), 2048)
    return d


def fft_receive():
    f = J.Fft(2048, 96000)
    f.receive(np.linspace(-1, 1, 4096, dtype=np.float32))
    return f


def fir_complex_gen():
    f = J.Fir(48000.0)
    f.weights(300, 3000)
    f.complex_gen(1000, 500)  # the NCO table stays with the handle
    return f


def phase_handle():
    p = J.Phase(2048)
    p.receive(np.linspace(-1, 1, 4096, dtype=np.float32))
    p.columns(300)
    return p


def group_of_one():
    g = J.Group(1, 4, L)
    x = J.DeviceBuffer.from_host(iq16(4))
    g.batch_i16([x], 2 * L, L)
    g.sync()
    return g


FAMILIES = [plain_bpsk, fft_acquire_bpsk, bpsk_switched_to_fft, channels, mode_channels, live_channels, tuned_bpsk, saved_and_restored,
            profiled_bpsk, receive_bpsk, plain_demod, demod_receive, demod_channels, fft_receive, fir_complex_gen, phase_handle, group_of_one]
# what the family must have raised beside the device buffers and their bytes
ALSO = {receive_bpsk: [PINNED, OBJECTS], plain_demod: [PINNED, OBJECTS], demod_receive: [PINNED, OBJECTS], demod_channels: [PINNED, OBJECTS],
        fft_receive: [PINNED], fir_complex_gen: [], phase_handle: [], group_of_one: [OBJECTS]}


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
def test_counts_return_to_their_baseline(family):
    base = live()
    h = family()
    held = J.live_resources()
    print(family.__name__, "baseline", base, "held", held)
    del h
    after = live()
    for k in [BUFS, BYTES] + ALSO.get(family, [OBJECTS]):
        assert held[k] > base[k], (k, base, held)
    assert after == base, (base, held, after)


# the fast variant's shadow handle goes with its parent.  The knob that makes a stream uncertifiable is read from the
# environment, so the recipe (tests/test_gpu_fixtures.py) runs in a child process that has it set from the start.
def _recovered_child():
    p = STREAMS["clean"]
    n = 2048 * 20
    raw = stream_input("clean")[:2 * n]
    base = live()
    d = J.Bpsk(rate=p["rate"], blen=8192, tuning=p["tuning"], nstreams=3, max_batch_samples=n, variant="fast")
    x = J.DeviceBuffer.from_host(np.concatenate([raw, np.zeros(2 * n, np.int16), raw]))  # (silence: nothing to certify)
    d.batch_i16(x, 2 * n, n)
    out = {"flagged": d.uncertified_streams(), "base": base, "alone": J.live_resources()}
    out["recovered"] = d.recover_uncertified([x.ptr], [n], 2 * n)
    out["shadowed"] = J.live_resources()
    d.batch_i16(x, 2 * n, n)  # the shadow runs beside the fast kernels
    d.sync()
    out["again"] = d.recover_uncertified([x.ptr, x.ptr], [n, n], 2 * n)  # nothing new: the shadow stays
    out["same"] = J.live_resources()
    del d
    out["after"] = live()
    print("RESULT " + json.dumps(out))


def test_a_recovered_fast_handle_takes_its_shadow_along():
    env = dict(os.environ, JSDR_KNOBS="1", JSDR_FAST_ARGMAX_SCALE="1e14")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "recovered-child"], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    print(r)
    assert r["flagged"] == [0, 2] and r["recovered"] == 2 and r["again"] == 0
    base, alone, shadowed = r["base"], r["alone"], r["shadowed"]
    assert alone[BUFS] > base[BUFS]
    # the shadow: a whole handle more (its buffers, stream and events) and the two staging buffers
    assert shadowed[BUFS] > alone[BUFS] + 2 and shadowed[BYTES] > alone[BYTES] and shadowed[OBJECTS] > alone[OBJECTS]
    assert r["same"] == shadowed
    assert r["after"] == base


# ------------------------------------------------------------------------------------------------ failed creates
# Geometries whose largest single buffer is above 1 TB -- no card holds it, hipMalloc refuses it at once and takes nothing --
# while every buffer before it in the creator's chain stays below 64 MB:
#   jsdr_bpsk_create, 96 kHz, 65535 streams of 2^24 samples a call: ktu 16.8 MB, kvco 3.4 MB, hist_in 2 x 16.8 MB, then
#     dm = 65535 x (64 + 1677723 + 64) double2 = 1.76 TB.  (At 2^22 samples a call dm would be 0.44 TB.)
#   the channel creators and jsdr_bpsk_create_tuned start with jsdr_bpsk_create: the same chain at 65532 / 65535 streams.
#   jsdr_demod_create, 65535 streams of 2560 frames of 2048: hist 11 MB, lilq, nco 2 x 42 MB, car_dev 2 x 21 MB (and 2 x 21 MB
#     pinned), then d = 65535 x 5242880 floats = 1.37 TB.
#   jsdr_demod_create(48000, 64, 65535, 64 * 65535) does not get as far as a buffer: 65535 streams x 65535 frames is refused by
#     the argument check ("batch too large") -- kept as the check it is.
#   jsdr_demod_create_channels has no buffer that grows with streams x samples (its rows come with the first call): none here.
BIG = 1 << 24
FAILING = {
    "bpsk": lambda: J.Bpsk(nstreams=65535, max_batch_samples=BIG),
    "bpsk_channels": lambda: J.BpskChannels(96000, 8192, [12000.0] * 4, ninputs=16383, max_batch_samples=BIG),
    "bpsk_mode_channels": lambda: J.BpskChannels(96000, 8192, [12000.0] * 4, do_fft=[1, 0, 0, 0], ninputs=16383, max_batch_samples=BIG),
    "bpsk_live_channels": lambda: J.BpskChannels(96000, 8192, [12000.0] * 4, ninputs=16383, max_batch_samples=BIG, live=True),
    "bpsk_tuned": lambda: J.BpskTuned(96000, 8192, [12000.0] * 65535, max_batch_samples=BIG),
    "demod": lambda: J.Demod(48000, 2048, 65535, 2048 * 2560),
    "demod_refused_geometry": lambda: J.Demod(48000, 64, 65535, 64 * 65535),
}


@pytest.mark.parametrize("which", sorted(FAILING))
def test_a_failed_create_leaves_nothing(which):
    base = live()
    with pytest.raises(J.JsdrError) as e:
        FAILING[which]()
    msg = str(e.value)
    print(which, "->", msg)
    assert len(msg.split(": ", 1)[1]) > 10  # JSDR_ERR came with a message
    del e
    assert live() == base
    d = plain_bpsk()  # no sticky error is left behind: a small handle works
    assert d.counters(0)["cntRaw"] == 2 * L
    del d
    assert live() == base


# ------------------------------------------------------------------------------------------------ function-local buffers
def test_calls_that_work_in_buffers_of_their_own_give_them_back():
    f = J.Fir(48000.0)
    f.weights(300, 3000)
    base = live()
    f.filter_block(np.arange(1000, dtype=np.int32))
    assert live() == base
    a = np.arange(2000, dtype=np.int32).reshape(1000, 2)
    f.complex_mod(a, a)
    assert live() == base
    pix, ai, aq = J.phase_columns(np.linspace(-1, 1, 4096, dtype=np.float32), 300)
    assert len(pix) > 0 and live() == base
    J.fec_decode(J.fec_encode(np.arange(256, dtype=np.uint8)))  # (jsdr_fec_encode, jsdr_fec_decode: the helpers at the end of fec.hip)
    assert live() == base


# ------------------------------------------------------------------------------------------------ repeated cycles
def test_twenty_create_destroy_cycles_end_at_the_baseline():
    d = plain_bpsk()  # the warm-up cycle: whatever is set up once per process is there before the baseline is taken
    del d
    base = live()
    for _ in range(20):
        d = J.Bpsk(nstreams=2, max_batch_samples=L)
        run_batches(d, 2)
        del d
    assert live() == base


if __name__ == "__main__" and sys.argv[1:] == ["recovered-child"]:
    _recovered_child()
