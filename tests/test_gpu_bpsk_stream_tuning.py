"""GPU: the tuned handle (jsdr_bpsk_create_tuned) -- a batch of lock-step demodulators in the tune mode, every stream with its
own tuning and its own live retunes (FUNcubeBPSKDemod.java:173-190, :195-196).  Every stream against its own reference
demodulator -- the oracle for integer tunings, a one-stream ordinary handle given jsdr_bpsk_set_tuning for fractional ones and
for live actions -- bit for bit: bits per call, FECDecode rc / bit index / bytes, the ten counters, the 18 state doubles
(tuPhase, double 0, per stream) and the (fi, fq) trace.  There is no tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import live_control_cases as M  # noqa: E402  (scenarios and inputs only)

pytestmark = pytest.mark.gpu

# a tile of 256 outputs at a decimation of 10 is 2560 samples, and 26 is the history
RAGGED = [77, 1, 16384, 4099, 65536, 26, 40000]
EDGES = [25, 27, 2559, 2560, 2561, 2586]
STATE = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)  # (6, 7: FFT-acquire only)
CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK", "centreBin")
FREQ, PLUS10, SUB10 = 0, 1, 2  # live_control.COMMANDS (the tune-only ones)


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


def noise_input(seed, n):
    return np.random.default_rng(seed).integers(-20000, 20000, 2 * n).astype(np.int16)


def run_tuned(inputs, tunings, chunks, rate=96000):
    """stream s is fed inputs[s] in the given calls; -> handle, per stream: bits, trace, fec of every call"""
    n = len(inputs[0]) // 2
    S = len(tunings)
    assert len(inputs) == S
    d = J.BpskTuned(rate, 8, tunings, max_batch_samples=max(chunks), size=4)
    d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
    bits, trace, fec = ([[] for _ in range(S)] for _ in range(3))
    pos = 0
    for L in chunks:
        d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        for s in range(S):
            bits[s].append(d.bits(s).copy())
            trace[s].append(d.trace(s).copy())
            fec[s].extend(d.fec_results(s))
        pos += L
    assert pos == n
    return d, bits, trace, fec


def check_against_oracle(d, s, bits, trace, fec, x, t, rate=96000):
    n = len(x) // 2
    assert float(t) == int(t)
    o = O.Bpsk(rate=rate, blen=4, tuning=int(t), trace=n // max(1, rate // 9600) + 8)
    o.receive_i16(x)
    assert np.array_equal(np.concatenate(bits), o.bits()), f"stream {s} ({t} Hz): bits differ"
    assert np.array_equal(np.concatenate(trace), o.trace()), f"stream {s} ({t} Hz): (fi,fq) differ"
    fo = o.fec_results()
    assert len(fec) == len(fo), (s, t, len(fec), len(fo))
    for (rc, _, data), (orc, _, odata) in zip(fec, fo):
        assert rc == orc and np.array_equal(data, odata), (s, t)
    same_counters(d.counters(s), o.counters())
    same_state(d.state(s), o.state())
    assert np.array_equal(d.decoded(s), o.decoded())


def one_stream_ref(rate, t, max_batch, blen=8):
    """the reference demodulator of a stream: created with (int) of the tuning, given the tuning before its first sample"""
    r = J.Bpsk(rate=rate, blen=blen, tuning=int(t), nstreams=1, max_batch_samples=max_batch)
    r.set_tuning(float(t))
    return r


def same_as_handle(d, s, r, what, trace=True):
    """stream s of d against the one-stream handle r, after a call both were given"""
    assert np.array_equal(d.bits(s), r.bits()), what
    if trace:
        assert np.array_equal(d.trace(s), r.trace()), what
    same_counters(d.counters(s), r.counters())
    same_state(d.state(s), r.state())
    fg, fr = d.fec_results(s), r.fec_results()
    assert [(a, b) for a, b, _ in fg] == [(a, b) for a, b, _ in fr], what
    assert all(np.array_equal(x[2], y[2]) for x, y in zip(fg, fr)), what
    assert np.array_equal(d.decoded(s), r.decoded()), what


# ---- 1
def test_each_stream_equals_its_reference_demodulator():
    """67 streams: one wave of the walk and three lanes of the next.  The calls are RAGGED + EDGES, then RAGGED three times more:
    a FEC frame is 5200 bits, 416 000 samples, and the streams tuned 1200 Hz below a carrier must decode it (the oracle alone
    does, on these seeds and this length -- rc 6, 2 and 5 -- at 0.015 s a stream, so the 67 oracles cost about a second)."""
    S = 67
    chunks = RAGGED + EDGES + RAGGED * 3
    n = sum(chunks)
    src, pays = [], []
    for k, car in enumerate((13200.0, 25200.0, 10200.0)):
        iq, pay, _ = O.make_dbpsk_stream(300 + k, k, n, carrier_hz=car, noise_sigma=900.0)
        src.append(iq)
        pays.append(pay)
    src.append(noise_input(303, n))
    tunings = [12000, 24000, 9000, 12010, -5000, 0, 1, 47999, 95999] + [11000 + 37 * s for s in range(9, S)]
    inputs = [src[s % 4] for s in range(S)]
    d, bits, trace, fec = run_tuned(inputs, tunings, chunks)
    assert d.front_kernel_name() == "k_front_pst"
    assert [d.stream_tuning(s) for s in range(S)] == [float(t) for t in tunings]
    assert d.control() == (12000.0, 0, 0)
    for s in range(S):
        check_against_oracle(d, s, bits[s], trace[s], fec[s], inputs[s], tunings[s])
    for s in range(3):  # tuned 1200 Hz below the carrier on their input: its payload comes out
        got = [data for rc, _, data in fec[s] if rc >= 0]
        assert got and any(np.array_equal(data, pays[s][0]) for data in got), s


# ---- 2
def test_equal_tunings_are_the_ordinary_handle():
    S = 5
    chunks = RAGGED
    n = sum(chunks)
    inputs = [O.make_dbpsk_stream(7, s, n, noise_sigma=900.0)[0] for s in range(S)]
    d = J.BpskTuned(96000, 8192, [12000] * S, max_batch_samples=max(chunks))
    e = J.Bpsk(rate=96000, blen=8192, tuning=12000, nstreams=S, max_batch_samples=max(chunks))
    d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
    pos = 0
    for L in chunks:
        for h in (d, e):
            h.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        for s in range(S):
            assert np.array_equal(d.bits(s), e.bits(s)), (L, s)
            assert np.array_equal(d.trace(s), e.trace(s)), (L, s)
            same_counters(d.counters(s), e.counters(s))
            same_state(d.state(s), e.state(s))
            fg, fe = d.fec_results(s), e.fec_results(s)
            assert [(a, b) for a, b, _ in fg] == [(a, b) for a, b, _ in fe]
            assert all(np.array_equal(x[2], y[2]) for x, y in zip(fg, fe))
        pos += L
    assert d.front_kernel_name() == "k_front_pst"
    assert e.front_kernel_name() == "k_fm"  # ordinary handles keep their kernels
    assert d.slot_info() == e.slot_info()


# ---- 3
def test_fractional_tunings_and_live_per_stream_retunes():
    chunks = [4099, 16384, 77, 20000, 8192, 30000, 2560, 2586]
    n = sum(chunks)
    tunings = [12000.5, 11987.25, 12000.0, 12000.0, 300.75, -0.5]
    S = len(tunings)
    inputs = [O.make_dbpsk_stream(31, s, n, noise_sigma=900.0)[0] for s in range(S)]
    # before call k: (first stream, [new tunings]) -- one value: set_stream_tuning, more: the bulk form
    acts = {
        1: [(2, [12010.0])], 2: [(2, [12020.0]), (3, [0.0])],
        3: [(2, [12030.0]), (3, [-3000.0])],  # stream 3: frozen above 0, then down through 0 inside call 3 ...
        4: [(4, [310.25, 5.5])],
        5: [(3, [9000.0])],                    # ... and back up through 0 inside call 5 (from about -5500 rad)
        6: [(0, [12000.5])],                   # the current value: still an action
    }
    d = J.BpskTuned(96000, 8192, tunings, max_batch_samples=max(chunks))
    refs = [one_stream_ref(96000, t, max(chunks), blen=8192) for t in tunings]
    now = list(tunings)
    d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
    pos = 0
    for k, L in enumerate(chunks):
        for first, vals in acts.get(k, []):
            mc = [d.counters(s)["dmMaxCorr"] for s in range(S)]
            if k == 6:
                assert mc[0] > 0 and mc[1] > 0  # (there is something to zero, and something to keep)
            if len(vals) == 1:
                d.set_stream_tuning(first, vals[0])
            else:
                d.set_stream_tunings(first, vals)
            for i, v in enumerate(vals):
                refs[first + i].set_tuning(v)
                now[first + i] = v
            assert [d.stream_tuning(s) for s in range(S)] == now
            for s in range(S):  # dmMaxCorr zeroed exactly where the action says
                hit = first <= s < first + len(vals)
                assert d.counters(s)["dmMaxCorr"] == (0 if hit else mc[s]), (k, s)
                assert d.counters(s)["dmMaxCorr"] == refs[s].counters()["dmMaxCorr"], (k, s)
        d.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
        for s, r in enumerate(refs):
            r.batch_i16(d_iq.ptr + 4 * (s * n + pos), 2 * n, L)
            same_as_handle(d, s, r, (k, s))
        pos += L
    # stream 3 did pass through 0 in both directions: its phase is positive again, and was not after call 4
    assert d.state(3)[0] > 0.0
    assert d.control()[0] == 12000.5


# ---- 4
@pytest.mark.parametrize("name", ["retune", "zero"])
def test_fixture_scenario_as_one_stream_among_others(name):
    """stream 5 of 67 runs the scenario of tests/golden/live_control_fixtures.npz, its actions mapped to set_stream_tuning,
    while the other streams sit at other tunings and are retuned at other points"""
    FX = np.load(os.path.join(HERE, "golden", "live_control_fixtures.npz"))
    k_ = "l_" + name + "_"
    p = M.SCENARIOS[name]
    assert p["do_fft"] == 0 and p["rate"] == 96000
    raw = M.scenario_input(name)
    n, calls, N = p["frame"], p["calls"], sum(p["calls"])
    acts = {}
    for c, cmd, v in zip(FX[k_ + "act_call"], FX[k_ + "act_cmd"], FX[k_ + "act_val"]):
        assert int(cmd) in (FREQ, PLUS10, SUB10), cmd
        acts.setdefault(int(c), []).append((int(cmd), float(v)))
    S, ME = 67, 5
    tunings = [11000.0 + 37 * s for s in range(S)]
    tunings[ME] = float(p["tuning"])
    d = J.BpskTuned(96000, 4 * n, tunings, max_batch_samples=max(calls))
    d_iq = J.DeviceBuffer.from_host(np.tile(raw, S))
    bits, fec = [], []
    pos = 0
    for c, L in enumerate(calls):
        other = (7 * c + 1) % S  # the others: one of them retuned before every call
        if other != ME:
            d.set_stream_tuning(other, 11500.0 + 13.5 * c)
        if c % 5 == 4:
            d.set_stream_tunings(ME + 1, [9000.0 - c, -40.0 * c, 0.0])
        for cmd, v in acts.get(c, []):
            t = d.stream_tuning(ME)
            d.set_stream_tuning(ME, v if cmd == FREQ else t + 10.0 if cmd == PLUS10 else t - 10.0)
        d.batch_i16(d_iq.ptr + 4 * pos, 2 * N, L)
        pos += L
        bits.append(d.bits(ME).copy())
        fec.extend(d.fec_results(ME))
        cnt = list(d.counters(ME).values())
        assert cnt == [int(v) for v in FX[k_ + "counters"][c]], (name, c, cnt, list(FX[k_ + "counters"][c]))
        st = d.state(ME)
        assert st.tobytes() == FX[k_ + "state"][c].tobytes(), (name, c, st, FX[k_ + "state"][c])
        assert sum(len(x) for x in bits) == int(FX[k_ + "nbits"][c]), (name, c)
    assert np.array_equal(np.concatenate(bits), FX[k_ + "bits"]), name
    assert [r[0] for r in fec] == [int(v) for v in FX[k_ + "fec_rc"]], name
    for r, want in zip(fec, FX[k_ + "fec_data"]):
        assert np.array_equal(r[2], want), name


# ---- 5
@pytest.mark.parametrize("rate,tunings", [(48000, [9000, 9010.5]), (192000, [12000, -3000]), (44100, [8000, 11025]),
                                          (32000, [5000, 5000.25])])
def test_tuned_handle_at_other_decimations(rate, tunings):
    n = 60000 * (rate // 9600) // 10
    x, _ = mixed_input(rate, n, [tunings[0] + 1200.0], rate=rate, noise=500.0)
    src = [x, noise_input(rate, n)]
    chunks = [n // 3, 5, n - n // 3 - 5]
    tun = [tunings[0], tunings[1], tunings[0], tunings[1]]
    inputs = [src[0], src[0], src[1], src[1]]
    d, bits, trace, fec = run_tuned(inputs, tun, chunks, rate=rate)
    assert d.front_kernel_name() == "k_front_pst"
    d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
    for s, t in enumerate(tun):
        if float(t) == int(t):
            check_against_oracle(d, s, bits[s], trace[s], fec[s], inputs[s], t, rate=rate)
            continue
        r = one_stream_ref(rate, t, max(chunks))
        pos, rfec = 0, []
        for k, L in enumerate(chunks):
            r.batch_i16(d_iq.ptr + 4 * (s * n + pos), 2 * n, L)
            assert np.array_equal(bits[s][k], r.bits()), (s, k)
            assert np.array_equal(trace[s][k], r.trace()), (s, k)
            rfec.extend(r.fec_results())
            pos += L
        assert [(a, b) for a, b, _ in fec[s]] == [(a, b) for a, b, _ in rfec]
        assert all(np.array_equal(a[2], b[2]) for a, b in zip(fec[s], rfec))
        same_counters(d.counters(s), r.counters())
        same_state(d.state(s), r.state())


# ---- 6
def test_float_input_and_alternating_input_forms():
    """batch_f32 of arbitrary floats against one-stream handles fed receive_f32 frame by frame; int16 and float calls alternate as
    an ordinary handle allows; the int16 call after arbitrary floats is refused and changes nothing"""
    frame = 2048
    tunings = [12000.5, -700.25, 23999.0]
    S = len(tunings)
    # (form, frames): i16 / f32 of JavaAudio's (float)s/32767f values / f32 of any value
    plan = [("i16", 3), ("java", 2), ("i16", 1), ("any", 3), ("refused", 1), ("any", 1)]
    N = frame * sum(f for form, f in plan if form != "refused")
    xs = [O.make_dbpsk_stream(61, s, N, noise_sigma=900.0)[0] for s in range(S)]
    rng = np.random.default_rng(62)
    fls = []
    for s in range(S):
        fl = O.convert_i16(xs[s]).astype(np.float32)
        pos = 0
        for form, f in plan:
            if form == "any":  # not (float)s/32767f values
                seg = slice(2 * pos * frame, 2 * (pos + f) * frame)
                fl[seg] = (fl[seg] * np.float32(0.7) + rng.normal(0.0, 0.01, 2 * f * frame).astype(np.float32)) * np.float32(1.0001)
            if form != "refused":
                pos += f
        fls.append(fl)
    d = J.BpskTuned(96000, 4 * frame, tunings, max_batch_samples=3 * frame)
    refs = [one_stream_ref(96000, t, frame, blen=4 * frame) for t in tunings]
    d_i16 = J.DeviceBuffer.from_host(np.concatenate(xs))
    d_f32 = J.DeviceBuffer.from_host(np.concatenate(fls))
    pos = 0
    for form, f in plan:
        L = f * frame
        if form == "refused":
            before = [(list(d.counters(s).values()), d.state(s).tobytes()) for s in range(S)]
            with pytest.raises(J.JsdrError, match="32767"):
                d.batch_i16(d_i16.ptr + 4 * pos * frame, 2 * N, L)
            assert [(list(d.counters(s).values()), d.state(s).tobytes()) for s in range(S)] == before
            continue
        if form == "i16":
            d.batch_i16(d_i16.ptr + 4 * pos * frame, 2 * N, L)
        else:
            d.batch_f32(d_f32.ptr + 8 * pos * frame, 2 * N, L)
        assert d.front_kernel_name() == "k_front_pst"
        for s, r in enumerate(refs):
            rbits = []
            for k in range(pos, pos + f):
                if form == "i16":
                    r.receive_raw(xs[s][2 * k * frame:2 * (k + 1) * frame])
                else:
                    r.receive(fls[s][2 * k * frame:2 * (k + 1) * frame])
                rbits.append(r.bits().copy())
            assert np.array_equal(d.bits(s), np.concatenate(rbits)), (form, pos, s)
            assert np.array_equal(d.trace(s)[-len(r.trace()):], r.trace()), (form, pos, s)
            same_counters(d.counters(s), r.counters())
            same_state(d.state(s), r.state())
        pos += f


# ---- 7
def _outputs(d, S):
    return [(list(d.counters(s).values()), d.state(s).tobytes(), d.bits(s).tobytes(), d.trace(s).tobytes()) for s in range(S)]


def _rc(call):
    def f():
        J.binding._check(call(), "refused")
    return f


def test_refusals_leave_the_handle_untouched():
    with pytest.raises(J.JsdrError, match="null tuning"):
        J.BpskTuned(96000, 8192, [])
    with pytest.raises(J.JsdrError, match="below the rate"):
        J.BpskTuned(96000, 8192, [12000, float("nan")])
    with pytest.raises(J.JsdrError, match="below the rate"):
        J.BpskTuned(96000, 8192, [12000, 96000.0])
    L = 2600
    tunings = [12000.0, 12010.5, -5000.0]
    S = len(tunings)
    lib = J.lib()
    two = (C.c_double * 2)(100.0, float("nan"))
    ok2 = (C.c_double * 2)(100.0, 200.0)
    t_, f_, u_ = C.c_double(), C.c_int(), C.c_int()
    frame_i16 = np.zeros(2 * 2048, np.int16)
    frame_f32 = np.zeros(2 * 2048, np.float32)
    a = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    b = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    with pytest.raises(J.JsdrError, match="tuned handle has no fast variant"):  # (before the first sample: no other reason to refuse)
        J.binding._check(lib.jsdr_bpsk_set_variant(a.h, 1), "jsdr_bpsk_set_variant")
    refusals = [
        ("not a finite", lambda: a.set_stream_tuning(0, float("nan"))),
        ("not a finite", lambda: a.set_stream_tuning(1, float("inf"))),
        ("below the rate", lambda: a.set_stream_tuning(0, 96000.0)),
        ("out of range", lambda: a.set_stream_tuning(S, 100.0)),
        ("out of range", lambda: a.set_stream_tuning(-1, 100.0)),
        ("stream 2", _rc(lambda: lib.jsdr_bpsk_set_stream_tunings(a.h, 1, 2, two))),  # (the first value is good: not applied either)
        ("out of range", _rc(lambda: lib.jsdr_bpsk_set_stream_tunings(a.h, 2, 2, ok2))),
        ("out of range", _rc(lambda: lib.jsdr_bpsk_set_stream_tunings(a.h, 0, 0, ok2))),
        ("null", _rc(lambda: lib.jsdr_bpsk_set_stream_tunings(a.h, 0, 2, None))),
        ("out of range", lambda: a.stream_tuning(S)),
        ("null", _rc(lambda: lib.jsdr_bpsk_get_stream_tuning(a.h, 0, None))),
        ("below the rate", lambda: a.set_tuning(float("nan"))),
        ("below the rate", lambda: a.set_tuning(96000.0)),
        ("below the rate", lambda: a.reconfigure(1e6, 0, 1)),
        ("tune mode only", lambda: a.set_mode(1, 0)),
        ("tune mode only", lambda: a.reconfigure(12000.0, 1, 0)),
        ("fast variant", _rc(lambda: lib.jsdr_bpsk_set_variant(a.h, 1))),
        ("jsdr_bpsk_create", lambda: a.receive_raw(frame_i16)),
        ("jsdr_bpsk_create", lambda: a.receive(frame_f32)),
        ("streams, not channels", _rc(lambda: lib.jsdr_bpsk_set_channel_tuning(a.h, 0, C.c_double(100.0)))),
        ("streams, not channels", _rc(lambda: lib.jsdr_bpsk_set_channel_mode(a.h, 0, 0, 1))),
        ("streams, not channels", _rc(lambda: lib.jsdr_bpsk_get_channel_control(a.h, 0, C.byref(t_), C.byref(f_), C.byref(u_)))),
        ("stride", lambda: a.batch_i16(d_iq.ptr, 2 * L - 2, L)),
        ("outside", lambda: a.batch_i16(d_iq.ptr, 2 * L + 2, L + 1)),
    ]
    n = L * (len(refusals) + 1)
    inputs = [O.make_dbpsk_stream(71, s, n, noise_sigma=900.0)[0] for s in range(S)]
    d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
    for h in (a, b):
        h.batch_i16(d_iq.ptr, 2 * n, L)
    for k, (what, bad) in enumerate(refusals):
        with pytest.raises(J.JsdrError, match=what):
            bad()
        assert [a.stream_tuning(s) for s in range(S)] == tunings and a.control() == (12000.0, 0, 0), what
        for h in (a, b):
            h.batch_i16(d_iq.ptr + 4 * L * (k + 1), 2 * n, L)
        assert _outputs(a, S) == _outputs(b, S), (k, what)
    # the whole-handle controls a tuned handle does take
    a.set_mode(0, 1)
    assert a.control() == (12000.0, 0, 1) and a.counters(0)["dmMaxCorr"] == 0
    a.reconfigure(11000.0, 0, 0)
    assert [a.stream_tuning(s) for s in range(S)] == [11000.0] * S and a.control() == (11000.0, 0, 0)
    a.set_tuning(-12.5)
    assert [a.stream_tuning(s) for s in range(S)] == [-12.5] * S


@pytest.mark.parametrize("kind", ["ordinary", "channels", "live_channels"])
def test_per_stream_calls_are_refused_on_handles_of_other_creators(kind):
    L = 4096
    make = {"ordinary": lambda: J.Bpsk(nstreams=2, max_batch_samples=L),
            "channels": lambda: J.BpskChannels(96000, 8192, [12000, 12010], max_batch_samples=L),
            "live_channels": lambda: J.BpskChannels(96000, 8192, [12000, 12010], max_batch_samples=L, live=True)}[kind]
    a, b = make(), make()
    x = O.make_dbpsk_stream(81, 0, 2 * L, noise_sigma=900.0)[0]
    d_iq = J.DeviceBuffer.from_host(np.concatenate([x, x]))
    lib = J.lib()
    one = (C.c_double * 1)(12010.0)
    t_ = C.c_double()
    for h in (a, b):
        J.Bpsk.batch_i16(h, d_iq.ptr, 4 * L, L)
    control = a.control()
    for call in (lambda: lib.jsdr_bpsk_set_stream_tuning(a.h, 0, C.c_double(12010.0)),
                 lambda: lib.jsdr_bpsk_set_stream_tunings(a.h, 0, 1, one),
                 lambda: lib.jsdr_bpsk_get_stream_tuning(a.h, 0, C.byref(t_))):
        assert call() != 0
        assert "jsdr_bpsk_create_tuned" in lib.jsdr_last_error().decode()
        assert a.control() == control
    for h in (a, b):
        J.Bpsk.batch_i16(h, d_iq.ptr + 4 * L, 4 * L, L)
    for s in range(2):
        for get in (J.Bpsk.counters, J.Bpsk.bits, J.Bpsk.trace, J.Bpsk.state):
            ga, gb = get(a, s), get(b, s)
            assert ga == gb if isinstance(ga, dict) else np.array_equal(ga, gb), (kind, s)


# ---- 8
def test_pack_slots_equal_the_slots_of_one_handle_per_stream():
    tunings = [12000.0, 12010.5, -5000.0, 24000.0]
    S = len(tunings)
    L = 50000
    inputs = [mixed_input(11 + s, L, [13200.0, 25200.0])[0] for s in range(S)]
    d = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
    d.batch_i16(d_iq.ptr, 2 * L, L)
    info = d.slot_info()
    slots = J.DeviceBuffer(info["slot_bytes"] * S)
    d.pack_slots(slots.ptr)
    J.binding.stream_sync()
    got = slots.to_host(np.uint8).reshape(S, -1)
    for s, t in enumerate(tunings):
        r = one_stream_ref(96000, t, L, blen=8192)
        r.batch_i16(d_iq.ptr + 4 * s * L, 2 * L, L)
        assert r.slot_info() == info
        rs = J.DeviceBuffer(info["slot_bytes"])
        r.pack_slots(rs.ptr)
        J.binding.stream_sync()
        assert np.array_equal(got[s], rs.to_host(np.uint8)), s
