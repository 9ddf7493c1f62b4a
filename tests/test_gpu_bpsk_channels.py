"""GPU: the channel handle (jsdr_bpsk_create_channels) -- ninputs x nchannels independently tuned demodulators fed the
same input, jsdr.java:479-483's nfcs FUNcubeBPSKDemod tabs.  Every stream against its own reference demodulator (or
against an ordinary handle already pinned to one) bit for bit: bits per call, FECDecode rc and bytes, the ten counters,
the 18 state doubles and the (fi,fq) trace."""
import os

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O

pytestmark = pytest.mark.gpu

RAGGED = [77, 1, 2048 * 8, 4099, 65536, 26, 40000]
STATE = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)  # (6, 7: FFT-acquire only)
CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK", "centreBin")


def same_counters(g, o):
    for k in CKEYS:
        assert g[k] == o[k], (k, g[k], o[k])


def same_state(g, o):
    for i in STATE:
        assert g[i] == o[i], (i, g[i], o[i])


def mixed_input(seed, n, carriers, rate=96000, noise=900.0):
    """int16-clipped sum of DBPSK streams at the given carriers (noise in each), and their payloads"""
    acc = np.zeros(2 * n, np.int64)
    pays = []
    for k, f in enumerate(carriers):
        iq, pay, _ = O.make_dbpsk_stream(seed, k, n, rate=rate, carrier_hz=f, noise_sigma=noise)
        acc += iq.astype(np.int64)
        pays.append(pay)
    return np.clip(acc, -32768, 32767).astype(np.int16), pays


def run_channels(inputs, tunings, chunks, rate=96000):
    """feed the inputs to one channel handle in the given calls; -> handle, per stream: bits, trace, fec of every call"""
    n = len(inputs[0]) // 2
    d = J.BpskChannels(rate, 8, tunings, ninputs=len(inputs), max_batch_samples=max(chunks), size=4)
    d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
    S = d.nstreams
    bits, trace, fec = ([[] for _ in range(S)] for _ in range(3))
    pos = 0
    for L in chunks:
        d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        for s in range(S):
            bits[s].append(J.Bpsk.bits(d, s).copy())
            trace[s].append(J.Bpsk.trace(d, s).copy())
            fec[s].extend(J.Bpsk.fec_results(d, s))
        pos += L
    assert pos == n
    return d, bits, trace, fec


def check_against_oracles(d, bits, trace, fec, inputs, tunings, rate=96000):
    K = len(tunings)
    n = len(inputs[0]) // 2
    for i, x in enumerate(inputs):
        for c, t in enumerate(tunings):
            s = i * K + c
            o = O.Bpsk(rate=rate, blen=4, tuning=int(t), trace=n // max(1, rate // 9600) + 8)
            o.receive_i16(x)
            assert np.array_equal(np.concatenate(bits[s]), o.bits()), f"input {i} channel {c}: bits differ"
            assert np.array_equal(np.concatenate(trace[s]), o.trace()), f"input {i} channel {c}: (fi,fq) differ"
            fo = o.fec_results()
            assert len(fec[s]) == len(fo), (i, c, len(fec[s]), len(fo))
            for (rc, _, data), (orc, _, odata) in zip(fec[s], fo):
                assert rc == orc and np.array_equal(data, odata)
            same_counters(d.counters(i, c), o.counters())
            same_state(d.state(i, c), o.state())
            assert np.array_equal(d.decoded(i, c), o.decoded())


def test_channel_handle_equals_one_reference_demodulator_per_channel():
    tunings = [12000, 24000, 12010, -5000]  # periodic, periodic, no period within 256 samples, pass-through
    chunks = RAGGED * 4
    n = sum(chunks)
    inputs, pays = [], []
    for i in range(3):
        x, p = mixed_input(100 + i, n, [13200.0, 25200.0])
        inputs.append(x)
        pays.append(p)
    d, bits, trace, fec = run_channels(inputs, tunings, chunks)
    assert d.front_kernel_name() == "k_chan_front"
    assert d.channel_info() == (3, 4)
    check_against_oracles(d, bits, trace, fec, inputs, tunings)
    # the channels that carry a signal decode it: the input means something
    for i in range(3):
        for c in (0, 1):
            got = [(rc, data) for rc, _, data in fec[i * 4 + c] if rc >= 0]
            assert got, (i, c)
            assert any(np.array_equal(data, pays[i][c][0]) for _, data in got), (i, c)


def test_one_channel_handle_equals_an_ordinary_handle():
    chunks = [77, 1, 16384, 4099, 26, 40000]
    n = sum(chunks)
    inputs = [O.make_dbpsk_stream(7, s, n, noise_sigma=900.0)[0] for s in range(2)]
    d, bits, trace, fec = run_channels(inputs, [12000], chunks)
    e = J.Bpsk(rate=96000, blen=8192, tuning=12000, nstreams=2, max_batch_samples=max(chunks))
    d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
    ebits, efec = [[], []], [[], []]
    pos = 0
    for L in chunks:
        e.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        for s in range(2):
            ebits[s].append(e.bits(s).copy())
            efec[s].extend(e.fec_results(s))
        pos += L
    assert e.front_kernel_name() != "k_chan_front"  # ordinary handles keep their kernels
    assert np.array_equal(d.trace(0, 0), e.trace(0)) and np.array_equal(d.trace(1, 0), e.trace(1))
    for s in range(2):
        assert np.array_equal(np.concatenate(bits[s]), np.concatenate(ebits[s]))
        same_counters(d.counters(s, 0), e.counters(s))
        same_state(d.state(s, 0), e.state(s))
        assert [(a, b) for a, b, _ in fec[s]] == [(a, b) for a, b, _ in efec[s]]
        assert all(np.array_equal(x[2], y[2]) for x, y in zip(fec[s], efec[s]))


@pytest.mark.parametrize("rate,tunings", [(48000, [9000, 9010]), (192000, [12000, -3000]), (44100, [8000, 11025])])
def test_channel_handle_at_other_rates(rate, tunings):
    n = 60000 * (rate // 9600) // 10
    x, _ = mixed_input(rate, n, [tunings[0] + 1200.0], rate=rate, noise=500.0)
    noise = np.random.default_rng(rate).integers(-20000, 20000, 2 * n).astype(np.int16)
    inputs = [x, noise]
    chunks = [n // 3, 5, n - n // 3 - 5]
    d, bits, trace, fec = run_channels(inputs, tunings, chunks, rate=rate)
    check_against_oracles(d, bits, trace, fec, inputs, tunings, rate=rate)


def test_live_per_channel_control_equals_ordinary_handles_given_the_same_actions():
    tunings = [12000, 24000, 12010]
    chunks = [4099, 16384, 77, 20000, 8192, 30000]
    n = sum(chunks)
    x, _ = mixed_input(5, n, [13200.0, 25200.0])
    # per call: (channel or None for every channel, new tuning)
    acts = {1: [(0, 12010.0)], 2: [(2, -100.0)], 4: [(None, 12000.0)]}
    d = J.BpskChannels(96000, 8192, tunings, max_batch_samples=max(chunks))
    refs = [J.Bpsk(rate=96000, blen=8192, tuning=t, nstreams=1, max_batch_samples=max(chunks)) for t in tunings]
    d_iq = J.DeviceBuffer.from_host(x)
    pos = 0
    for k, L in enumerate(chunks):
        for ch, t in acts.get(k, []):
            before = [d.channel_control(c) for c in range(3)]
            if ch is None:
                d.set_tuning(t)
                for r in refs:
                    r.set_tuning(t)
            else:
                d.set_channel_tuning(ch, t)
                refs[ch].set_tuning(t)
            for c in range(3):
                if ch is None or c == ch:
                    assert d.channel_control(c) == (t, 0, 0)
                else:
                    assert d.channel_control(c) == before[c]
            for c in range(3):  # dmMaxCorr zeroed exactly where the action says
                assert d.counters(0, c)["dmMaxCorr"] == refs[c].counters()["dmMaxCorr"]
        d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        for c, r in enumerate(refs):
            r.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
            assert np.array_equal(d.bits(0, c), r.bits()), (k, c)
            assert np.array_equal(d.trace(0, c), r.trace()), (k, c)
            same_counters(d.counters(0, c), r.counters())
            same_state(d.state(0, c), r.state())
            assert [(a, b) for a, b, _ in d.fec_results(0, c)] == [(a, b) for a, b, _ in r.fec_results()]
        pos += L


def test_drop_in_receive_with_two_channels_equals_batch_and_oracles(golden_dir):
    raw = np.fromfile(os.path.join(golden_dir, "sine4410.raw"), dtype="<i2")
    frame = 2048
    dbpsk, _ = mixed_input(9, frame * 24, [13200.0])
    for x in (raw[:4 * frame], dbpsk):
        nfr = len(x) // (2 * frame)
        x = x[:2 * frame * nfr]
        tunings = [12000, 13000]
        di = J.BpskChannels(96000, 8192, tunings)
        df = J.BpskChannels(96000, 8192, tunings)
        db, bits, trace, fec = run_channels([x], tunings, [frame] * nfr)
        buf = O.convert_i16(x)
        ibits = [[], []]
        fbits = [[], []]
        for f in range(nfr):
            di.receive_raw(x[2 * f * frame:2 * (f + 1) * frame])
            df.receive(buf[2 * f * frame:2 * (f + 1) * frame])  # JavaAudio-style floats
            for c in range(2):
                ibits[c].append(di.bits(0, c).copy())
                fbits[c].append(df.bits(0, c).copy())
        check_against_oracles(db, bits, trace, fec, [x], tunings)
        for c in range(2):
            assert np.array_equal(np.concatenate(ibits[c]), np.concatenate(bits[c]))
            assert np.array_equal(np.concatenate(fbits[c]), np.concatenate(bits[c]))
            for dd in (di, df):
                same_counters(dd.counters(0, c), db.counters(0, c))
                same_state(dd.state(0, c), db.state(0, c))
                assert np.array_equal(dd.trace(0, c), db.trace(0, c))
    # other floats are refused, the handle keeps going
    bad = np.full(2 * frame, 0.3, np.float32)
    with pytest.raises(J.JsdrError, match="32767"):
        df.receive(bad)


def test_schedule_is_built_once_for_equal_and_periodic_channels():
    d = J.BpskChannels(96000, 8192, [12000, 12000])
    x, _ = mixed_input(3, 2048 * 8, [13200.0])
    counts = []
    for f in range(8):
        d.receive_raw(x[2 * f * 2048:2 * (f + 1) * 2048])
        counts.append(d.schedule_stats()["computed_inline"])
    assert counts[0] == 1, counts  # two channels at the same tuning: one schedule
    assert counts[-1] == counts[2], counts  # periodic: nothing more after the first calls
    for c in range(2):
        assert np.array_equal(d.bits(0, 0), d.bits(0, 1))


def test_pack_slots_equal_the_slots_of_one_handle_per_channel():
    tunings = [12000, 24000, 12010]
    L = 50000
    x, _ = mixed_input(11, L, [13200.0, 25200.0])
    d = J.BpskChannels(96000, 8192, tunings, max_batch_samples=L)
    d_iq = J.DeviceBuffer.from_host(x)
    d.batch_i16(d_iq.ptr, 2 * L, L)
    info = d.slot_info()
    slots = J.DeviceBuffer(info["slot_bytes"] * 3)
    d.pack_slots(slots.ptr)
    J.binding.stream_sync()
    got = slots.to_host(np.uint8).reshape(3, -1)
    for c, t in enumerate(tunings):
        r = J.Bpsk(rate=96000, blen=8192, tuning=t, max_batch_samples=L)
        r.batch_i16(d_iq.ptr, 2 * L, L)
        assert r.slot_info() == info
        rs = J.DeviceBuffer(info["slot_bytes"])
        r.pack_slots(rs.ptr)
        J.binding.stream_sync()
        assert np.array_equal(got[c], rs.to_host(np.uint8)), c


def test_refused_calls_leave_the_controls_as_they_were():
    with pytest.raises(J.JsdrError, match="nchannels"):
        J.BpskChannels(96000, 8192, [])
    with pytest.raises(J.JsdrError, match="nchannels"):
        J.BpskChannels(96000, 8192, [12000] * 17)
    with pytest.raises(J.JsdrError, match="not finite"):
        J.BpskChannels(96000, 8192, [12000, float("nan")])
    d = J.BpskChannels(96000, 8192, [12000, 24000], ninputs=2, max_batch_samples=4096)
    d.set_channel_mode(1, 0, 1)
    before = [d.channel_control(c) for c in range(2)]
    assert before == [(12000.0, 0, 0), (24000.0, 0, 1)]
    x = J.DeviceBuffer.from_host(np.zeros(4 * 4096, np.int16))
    for bad in (lambda: d.set_channel_mode(0, 1, 0), lambda: d.set_mode(1, 0), lambda: d.reconfigure(12000.0, 1, 0),
                lambda: J.binding._check(J.lib().jsdr_bpsk_set_variant(d.h, 1), "jsdr_bpsk_set_variant"),
                lambda: d.set_channel_tuning(2, 100.0), lambda: d.set_channel_tuning(-1, 100.0),
                lambda: d.set_channel_mode(5, 0, 0), lambda: d.channel_control(2),
                lambda: d.set_channel_tuning(0, float("inf")), lambda: d.set_tuning(float("nan")),
                lambda: d.batch_i16(x.ptr, 2 * 4096 - 2, 4096)):
        with pytest.raises(J.JsdrError):
            bad()
        assert [d.channel_control(c) for c in range(2)] == before
    d.batch_i16(x.ptr, 2 * 4096, 4096)  # still works
    with pytest.raises(J.JsdrError, match="snapshot"):
        d.snapshot()
