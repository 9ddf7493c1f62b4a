"""GPU: tuning plans (jsdr_bpsk_plan_stream_tunings) -- retunes INSIDE a batch call of a tuned handle, each stream at samples of
its own.  The reference for stream s is a one-stream ordinary handle fed the same samples in pieces cut at stream s's own entry
positions, with reconfigure(f, 0, 0) between the pieces (setup, FUNcubeBPSKDemod.java:192-209: dmMaxCorr carries on).  Compared
bit for bit: the bits of the call, FECDecode rc / bit index / bytes, the ten counters (dmMaxCorr included), the state doubles,
decoded[] and the (fi, fq) trace.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O
from test_gpu_bpsk_stream_tuning import (_outputs, _rc, check_against_oracle, mixed_input, one_stream_ref, same_counters,
                                         same_state)

pytestmark = pytest.mark.gpu


class Ref:
    """stream s's reference demodulator, reading row s of the device buffer the tuned handle reads"""

    def __init__(self, rate, tuning, max_batch, buf, row, nrow):
        self.r = one_stream_ref(rate, tuning, max_batch)
        self.buf, self.row, self.nrow = buf, row, nrow

    def call(self, pos, L, entries=(), f32=False):
        """samples pos .. pos + L - 1 in pieces cut at the entries [(at_sample, tuning)] -> bits, trace, fec of all pieces"""
        at = {int(a): float(f) for a, f in entries}
        assert all(0 <= a < L for a in at)
        cuts = sorted({0, L} | set(at))
        bits, trace, fec = [], [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a in at:
                self.r.reconfigure(at[a], 0, 0)
            first = self.row * self.nrow + pos + a
            if f32:
                self.r.batch_f32(self.buf.ptr + 8 * first, 2 * self.nrow, b - a)
            else:
                self.r.batch_i16(self.buf.ptr + 4 * first, 2 * self.nrow, b - a)
            fec.extend((rc, sum(len(x) for x in bits) + bi, data) for rc, bi, data in self.r.fec_results())  # (index among the call's bits)
            bits.append(self.r.bits().copy())
            trace.append(self.r.trace().copy())
        return np.concatenate(bits), np.concatenate(trace), fec


def same_call(d, s, ref, got, what):
    """stream s of d after a call against what its reference gave for the same samples"""
    bits, trace, fec = got
    assert np.array_equal(d.bits(s), bits), what
    assert np.array_equal(d.trace(s), trace), what
    fg = d.fec_results(s)
    assert [(a, b) for a, b, _ in fg] == [(a, b) for a, b, _ in fec], what
    assert all(np.array_equal(x[2], y[2]) for x, y in zip(fg, fec)), what
    same_counters(d.counters(s), ref.r.counters())
    same_state(d.state(s), ref.r.state())
    assert np.array_equal(d.decoded(s), ref.r.decoded()), what


def plan_of(entries):
    """{stream: [(at_sample, tuning)]} -> the three lists of plan_tunings"""
    st, at, tu = [], [], []
    for s in sorted(entries):
        for a, f in entries[s]:
            st.append(s)
            at.append(a)
            tu.append(f)
    return st, at, tu


def planned_call(d, refs, buf, nrow, pos, L, entries, f32=False, what="", give=True):
    """one call of L samples with the plan `entries` (give=False: it is pending already) on d and, in pieces, on every
    reference -> what each reference gave"""
    S = len(refs)
    if entries and give:
        d.plan_tunings(*plan_of(entries))
    assert d.planned() == sum(len(v) for v in entries.values())
    if f32:
        d.batch_f32(buf.ptr + 8 * pos, 2 * nrow, L)
    else:
        d.batch_i16(buf.ptr + 4 * pos, 2 * nrow, L)
    assert d.planned() == 0
    if L >= 1000:  # (a call with outputs names its front end)
        assert d.front_kernel_name() == ("k_front_pst_plan" if entries else "k_front_pst"), what
    out = []
    for s in range(S):
        out.append(refs[s].call(pos, L, entries.get(s, ()), f32))
        same_call(d, s, refs[s], out[-1], (what, pos, L, s))
        if entries.get(s):
            assert d.stream_tuning(s) == float(entries[s][-1][1]), (what, s)
    return out


def setup(rate, tunings, chunks_max, n, seed, carriers=None):
    S = len(tunings)
    inputs = [mixed_input(seed + s, n, [(carriers[s] if carriers else 13200.0)], rate=rate)[0] for s in range(S)]
    buf = J.DeviceBuffer.from_host(np.concatenate(inputs))
    d = J.BpskTuned(rate, 8192, tunings, max_batch_samples=chunks_max)
    refs = [Ref(rate, t, chunks_max, buf, s, n) for s, t in enumerate(tunings)]
    return d, refs, buf, inputs


# ---- 1
def test_entries_at_the_history_checkpoint_and_tile_positions():
    first, L, after = 4099, 20000, 5000
    n = first + L + after
    P = [0, 1, 25, 26, 27, 63, 64, 65, 2559, 2560, 2561, 2586, L - 27, L - 26, L - 1]
    tunings = [12000.0, 12010.5, 11987.25, 12000.0, 300.75, 12000.5]
    d, refs, buf, _ = setup(96000, tunings, L, n, 40)
    entries = {
        0: [(a, 12000.0 + 7.25 * (i + 1) * (-1) ** i) for i, a in enumerate(P)],  # every position
        # (1: none)
        2: [(0, 11990.0)],
        3: [(2560, 12010.0), (2561, 12020.5)],                                   # a sample apart
        4: [(25, 310.25), (26, 5.5), (27, 320.0)],                               # three in one checkpoint block
        5: [(64, 12000.5), (2559, 0.0), (2586, -500.0), (L - 27, 11990.0)],      # down through 0 and, in the next call, back up
    }
    planned_call(d, refs, buf, n, 0, first, {}, what="before")
    assert d.front_kernel_name() == "k_front_pst"
    planned_call(d, refs, buf, n, first, L, entries, what="planned")
    assert d.front_kernel_name() == "k_front_pst_plan"
    assert d.stream_tuning(1) == 12010.5 and d.control()[0] == entries[0][-1][1]
    assert d.state(5)[0] <= 0.0  # stream 5 is below 0: its last 26 samples passed through unmixed
    # the plan was one-shot and the kept indices were the factors of the last 26 samples: the next call continues
    planned_call(d, refs, buf, n, first + L, after, {}, what="after")
    assert d.front_kernel_name() == "k_front_pst"
    assert d.state(5)[0] > 0.0


# ---- 2
@pytest.mark.parametrize("L", [1, 25, 26, 77])
def test_planned_calls_shorter_than_the_history(L):
    first, after = 4099, 3000
    n = first + L + after
    d, refs, buf, _ = setup(96000, [12000.0, 12010.5, 11000.0], 4099, n, 50 + L)
    entries = {0: [(0, 12020.0)], 1: [(L - 1, 11990.5)], 2: [(0, 11010.0)] + ([(L - 1, 11020.25)] if L > 1 else [])}
    planned_call(d, refs, buf, n, 0, first, {}, what="before")
    planned_call(d, refs, buf, n, first, L, entries, what="short")
    planned_call(d, refs, buf, n, first + L, after, {}, what="after")
    assert [d.stream_tuning(s) for s in range(3)] == [12020.0, 11990.5, 11020.25 if L > 1 else 11010.0]


# ---- 3
@pytest.mark.parametrize("rate,edge", [(192000, 3380), (48000, 1280)])
def test_entries_at_the_tile_edge_of_other_decimations(rate, edge):
    L = 16384
    n = 3 * L
    base = 12000.0 if rate == 192000 else 9000.0
    d, refs, buf, _ = setup(rate, [base, base + 10.5, base - 20.0], L, n, rate // 1000, carriers=[base + 1200.0] * 3)
    a = {0: [(edge - 1, base + 5.0), (edge, base + 10.25), (edge + 1, base + 15.0)], 1: [(edge, base)]}
    b = {1: [(edge - 1, base + 20.5), (edge + 1, -40.0)], 2: [(edge, base - 10.0), (2 * edge, base)]}
    planned_call(d, refs, buf, n, 0, L, a, what="a")
    assert d.front_kernel_name() == "k_front_pst_plan"
    planned_call(d, refs, buf, n, L, L, b, what="b")
    planned_call(d, refs, buf, n, 2 * L, L, {}, what="c")
    assert d.front_kernel_name() == "k_front_pst"


# ---- 4
def test_planned_float_calls_alternating_with_int16_calls():
    L = 6000
    forms = [False, True, False, True, True, False]  # f32?
    n = L * len(forms)
    tunings = [12000.5, -700.25, 23999.0]
    S = len(tunings)
    xs = [O.make_dbpsk_stream(61, s, n, noise_sigma=900.0)[0] for s in range(S)]
    b16 = J.DeviceBuffer.from_host(np.concatenate(xs))
    b32 = J.DeviceBuffer.from_host(np.concatenate([O.convert_i16(x).astype(np.float32) for x in xs]))  # JavaAudio's floats
    d = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    refs = [Ref(96000, t, L, None, s, n) for s, t in enumerate(tunings)]
    for k, f32 in enumerate(forms):
        for r in refs:
            r.buf = b32 if f32 else b16
        entries = {0: [(0, 12000.5 + k), (2560 + k, 11990.25)], 2: [(25 + k, 23000.0 + k), (26 + k, 23010.5), (L - 1, 23999.0 - k)]}
        if k == 3:
            entries = {}
        planned_call(d, refs, b32 if f32 else b16, n, k * L, L, entries, f32=f32, what=("form", k))
        assert d.front_kernel_name() == ("k_front_pst_plan" if entries else "k_front_pst")


# ---- 5
def test_plans_that_restate_the_tunings_equal_the_oracle():
    """integer tunings, every entry the stream's current tuning: the planned kernels run and every stream is O.Bpsk of its
    tuning, through a FEC frame (5200 bits, 416 000 samples)"""
    chunks = [150000, 160000, 150016]
    n = sum(chunks)
    tunings = [12000, 24000, 9000]
    S = len(tunings)
    inputs = [O.make_dbpsk_stream(300 + s, s, n, carrier_hz=t + 1200.0, noise_sigma=900.0)[0] for s, t in enumerate(tunings)]
    d = J.BpskTuned(96000, 8, tunings, max_batch_samples=max(chunks), size=4)
    buf = J.DeviceBuffer.from_host(np.concatenate(inputs))
    bits, trace, fec = ([[] for _ in range(S)] for _ in range(3))
    pos = 0
    for k, L in enumerate(chunks):
        at = sorted({0, 1, 63, 64, 2560, L - 1} | set(range(997 + k, L, 1009)))
        d.plan_tunings(*plan_of({s: [(a, float(t)) for a in at[s:]] for s, t in enumerate(tunings)}))
        d.batch_i16(buf.ptr + 4 * pos, 2 * n, L)
        assert d.front_kernel_name() == "k_front_pst_plan" and d.planned() == 0
        for s in range(S):
            bits[s].append(d.bits(s).copy())
            trace[s].append(d.trace(s).copy())
            fec[s].extend(d.fec_results(s))
        pos += L
    for s in range(S):
        check_against_oracle(d, s, bits[s], trace[s], fec[s], inputs[s], tunings[s])
        assert any(rc >= 0 for rc, _, _ in fec[s]), s


# ---- 6
def drifting_stream(seed, stream, n, f0, step_hz, every, rate=96000, noise_sigma=900.0):
    """make_dbpsk_stream with a carrier that steps by step_hz every `every` samples, phase-continuous"""
    sps = rate // 1200
    nframes = -(-n // (5200 * sps)) + 1
    pay = np.stack([O.synth_payload(seed, stream, f) for f in range(nframes)])
    dsign = O.synth_diffsign(np.concatenate([O.fec_encode(p) for p in pay]), 1)
    ct, st = O.synth_tables(3000)
    gain = int(round(noise_sigma / 37837.0 * 32768.0))
    key = O.mix64((seed * 0x9E3779B1 + stream) ^ 0xA5A5A5A5)
    out, ph0, inc_prev = [], 0, None
    for k, g0 in enumerate(range(0, n, every)):
        inc = O.phase_inc_u32(f0 + k * step_hz, rate)
        if inc_prev is not None:
            ph0 = (ph0 + g0 * inc_prev - g0 * inc) & 0xFFFFFFFF  # the phase at g0 is the one the piece before ends on
        out.append(O.synth_dbpsk(g0, min(every, n - g0), dsign, sps, ph0, inc, ct, st, gain, key))
        inc_prev = inc
    return np.concatenate(out)


def test_plans_follow_stepping_carriers_through_a_decode():
    chunks = [115000] * 4
    n = sum(chunks)
    drift = [(13200.0, 40.0, 38400), (25200.0, -35.5, 30000), (10200.0, 25.25, 47001)]  # (carrier, step, every)
    S = len(drift)
    inputs = [drifting_stream(700, s, n, f0, st, ev) for s, (f0, st, ev) in enumerate(drift)]
    tunings = [f0 - 1200.0 for f0, _, _ in drift]
    buf = J.DeviceBuffer.from_host(np.concatenate(inputs))
    d = J.BpskTuned(96000, 8192, tunings, max_batch_samples=max(chunks))
    refs = [Ref(96000, t, max(chunks), buf, s, n) for s, t in enumerate(tunings)]
    rcs = [[] for _ in range(S)]
    pos = 0
    for L in chunks:
        entries = {}
        for s, (f0, st, ev) in enumerate(drift):
            e = [(g - pos, f0 - 1200.0 + (g // ev) * st) for g in range(ev, n, ev) if pos <= g < pos + L]
            if e:
                entries[s] = e
        assert entries
        got = planned_call(d, refs, buf, n, pos, L, entries, what="drift")  # (every FEC result compared, rc, bit index and bytes)
        for s in range(S):
            rcs[s].extend(rc for rc, _, _ in got[s][2])
        pos += L
    for s in range(S):
        assert any(rc >= 0 for rc in rcs[s]), (s, rcs[s])  # the references decode


# ---- 7
def test_plan_set_tuning_after_it_replaced_cleared_and_counted():
    L = 8000
    n = 5 * L
    tunings = [12000.0, 12010.5, 11987.25]
    S = len(tunings)
    inputs = [mixed_input(95 + s, n, [13200.0])[0] for s in range(S)]
    buf = J.DeviceBuffer.from_host(np.concatenate(inputs))
    d = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    refs = [Ref(96000, t, L, buf, s, n) for s, t in enumerate(tunings)]
    planned_call(d, refs, buf, n, 0, L, {}, what=0)
    # set_stream_tuning after the plan and before the call acts before sample 0; the entries come after it in sample order
    d.plan_tunings([0, 1], [100, 3000], [12020.0, 11000.0])
    d.set_stream_tuning(1, 12030.0)
    d.set_stream_tuning(2, 11900.0)
    for s, f in ((1, 12030.0), (2, 11900.0)):
        refs[s].r.set_tuning(f)
    assert d.planned() == 2 and [d.stream_tuning(s) for s in range(S)] == [12000.0, 12030.0, 11900.0]
    d.batch_i16(buf.ptr + 4 * L, 2 * n, L)
    assert d.planned() == 0 and d.front_kernel_name() == "k_front_pst_plan"
    for s, e in enumerate([[(100, 12020.0)], [(3000, 11000.0)], []]):
        same_call(d, s, refs[s], refs[s].call(L, L, e), ("set after plan", s))
    assert [d.stream_tuning(s) for s in range(S)] == [12020.0, 11000.0, 11900.0] and d.control()[0] == 12020.0
    # plan twice: the second replaces the first; n = 0 clears
    d.plan_tunings([0, 0, 2], [5, 6, 7], [1.0, 2.0, 3.0])
    assert d.planned() == 3
    d.plan_tunings([1], [63], [12000.25])
    assert d.planned() == 1
    planned_call(d, refs, buf, n, 2 * L, L, {1: [(63, 12000.25)]}, what="replaced", give=False)  # the second plan alone ran
    d.plan_tunings([0], [5], [1.0])
    d.plan_tunings([], [], [])
    assert d.planned() == 0
    planned_call(d, refs, buf, n, 3 * L, L, {}, what="cleared")
    assert d.front_kernel_name() == "k_front_pst"
    assert [d.stream_tuning(s) for s in range(S)] == [12020.0, 12000.25, 11900.0]


def test_save_after_a_planned_call_restores_into_a_fresh_handle():
    L = 8000
    n = 3 * L
    tunings = [12000.0, 12010.5, 300.75]
    d, refs, buf, _ = setup(96000, tunings, L, n, 99)
    planned_call(d, refs, buf, n, 0, L, {}, what=0)
    planned_call(d, refs, buf, n, L, L, {0: [(100, 12020.0), (L - 1, 11990.5)], 2: [(L - 20, -500.0)]}, what="planned")
    blob = d.save()
    f = J.BpskTuned(96000, 8192, [1.0, 2.0, 3.0], max_batch_samples=L)
    f.restore(blob)
    assert f.planned() == 0  # a plan is not state
    assert [f.stream_tuning(s) for s in range(3)] == [11990.5, 12010.5, -500.0] == [d.stream_tuning(s) for s in range(3)]
    for h in (d, f):
        h.batch_i16(buf.ptr + 4 * 2 * L, 2 * n, L)
    for s in range(3):
        got = refs[s].call(2 * L, L, [])
        same_call(d, s, refs[s], got, ("after save", s))
        same_call(f, s, refs[s], got, ("restored", s))


# ---- 8
def test_refused_plans_and_calls_leave_the_handle_and_a_pending_plan_untouched():
    L = 2600
    tunings = [12000.0, 12010.5, -5000.0]
    S = len(tunings)
    lib = J.lib()
    a = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    b = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    def arr(ctype, v):
        return None if v is None else (ctype * len(v))(*v)

    def plan(st, at, tu, n=None):
        return _rc(lambda: lib.jsdr_bpsk_plan_stream_tunings(a.h, arr(C.c_int32, st), arr(C.c_int64, at), arr(C.c_double, tu),
                                                             C.c_int64(len(st) if n is None else n)))

    refusals = [
        ("null array", plan(None, [1], [100.0], 1)),
        ("null array", plan([0], None, [100.0], 1)),
        ("null array", plan([0], [1], None, 1)),
        ("-1 entries", plan([0], [1], [100.0], -1)),
        ("out of range", plan([0, S], [1, 1], [100.0, 100.0])),
        ("out of range", plan([-1], [1], [100.0])),
        ("out of order", plan([1, 0], [1, 1], [100.0, 100.0])),           # streams descend
        ("out of order", plan([0, 0], [5, 4], [100.0, 100.0])),           # samples descend
        ("out of order", plan([0, 1, 1], [5, 7, 7], [1.0, 2.0, 3.0])),    # duplicated
        ("negative", plan([0, 1], [5, -1], [100.0, 100.0])),
        ("not a finite", plan([0, 1], [5, 6], [100.0, float("nan")])),
        ("not a finite", plan([0], [5], [float("inf")])),
        ("below the rate", plan([0, 2], [5, 6], [100.0, 96000.0])),
        ("stays pending", lambda: a.batch_i16(d_iq.ptr, 2 * n, 1500)),     # the pending plan has an entry at 1500
        ("stays pending", lambda: a.batch_f32(d_f.ptr, 2 * n, 1200)),
    ]
    n = L * (len(refusals) + 2)
    inputs = [O.make_dbpsk_stream(71, s, n, noise_sigma=900.0)[0] for s in range(S)]
    d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
    d_f = J.DeviceBuffer.from_host(np.concatenate([O.convert_i16(x).astype(np.float32) for x in inputs]))
    pending = ([0, 2, 2], [7, 64, 1500], [12005.0, -4000.0, 100.5])
    for h in (a, b):
        h.batch_i16(d_iq.ptr, 2 * n, L)
    for k, (what, bad) in enumerate(refusals):
        for h in (a, b):
            h.plan_tunings(*pending)
        with pytest.raises(J.JsdrError, match=what):
            bad()
        assert a.planned() == 3 and [a.stream_tuning(s) for s in range(S)] == [b.stream_tuning(s) for s in range(S)], what
        for h in (a, b):  # the refused call left the pending plan in force: both run it in this, longer call
            h.batch_i16(d_iq.ptr + 4 * L * (k + 1), 2 * n, L)
            assert h.front_kernel_name() == "k_front_pst_plan" and h.planned() == 0
        assert _outputs(a, S) == _outputs(b, S), (k, what)
        assert [a.stream_tuning(s) for s in range(S)] == [12005.0, 12010.5, 100.5], what
        for h in (a, b):
            h.set_stream_tunings(0, tunings)


@pytest.mark.parametrize("kind", ["ordinary", "channels", "fast"])
def test_plans_are_refused_on_handles_of_other_creators(kind):
    L = 4096
    make = {"ordinary": lambda: J.Bpsk(nstreams=2, max_batch_samples=L),
            "channels": lambda: J.BpskChannels(96000, 8192, [12000, 12010], max_batch_samples=L),
            "fast": lambda: J.Bpsk(nstreams=2, max_batch_samples=L)}[kind]
    a, b = make(), make()
    lib = J.lib()
    if kind == "fast":
        for h in (a, b):
            J.binding._check(lib.jsdr_bpsk_set_variant(h.h, 1), "jsdr_bpsk_set_variant")
    x = O.make_dbpsk_stream(81, 0, 2 * L, noise_sigma=900.0)[0]
    d_iq = J.DeviceBuffer.from_host(np.concatenate([x, x]))
    for h in (a, b):
        J.Bpsk.batch_i16(h, d_iq.ptr, 4 * L, L)
    control = a.control()
    cnt = C.c_int64(-1)
    for call in (lambda: lib.jsdr_bpsk_plan_stream_tunings(a.h, (C.c_int32 * 1)(0), (C.c_int64 * 1)(5), (C.c_double * 1)(12010.0), C.c_int64(1)),
                 lambda: lib.jsdr_bpsk_plan_stream_tunings(a.h, None, None, None, C.c_int64(0)),
                 lambda: lib.jsdr_bpsk_planned_tunings(a.h, C.byref(cnt))):
        assert call() != 0
        assert "jsdr_bpsk_create_tuned" in lib.jsdr_last_error().decode()
        assert a.control() == control and cnt.value == -1
    for h in (a, b):
        J.Bpsk.batch_i16(h, d_iq.ptr + 4 * L, 4 * L, L)
    for s in range(2):
        for get in (J.Bpsk.counters, J.Bpsk.bits, J.Bpsk.trace, J.Bpsk.state):
            ga, gb = get(a, s), get(b, s)
            assert ga == gb if isinstance(ga, dict) else np.array_equal(ga, gb), (kind, s)


# ---- 9
def test_a_plan_and_a_refused_plan_own_nothing_after_destroy():
    L = 4096
    x = O.make_dbpsk_stream(83, 0, 2 * L, noise_sigma=900.0)[0]
    d_iq = J.DeviceBuffer.from_host(np.concatenate([x, x]))
    J.binding.stream_sync()
    before = J.live_resources()
    d = J.BpskTuned(96000, 8192, [12000.0, 12010.5], max_batch_samples=L)
    made = J.live_resources()
    d.plan_tunings([0, 1, 1], [5, 64, 65], [12001.0, 12002.0, 12003.0])
    with_plan = J.live_resources()
    assert with_plan[0] > made[0] and with_plan[1] > made[1]  # the device copy is the library's own, and counted
    with pytest.raises(J.JsdrError, match="out of order"):  # refused mid-validation: the entries before it were good
        d.plan_tunings([0, 1, 1, 0], [5, 64, 65, 66], [1.0, 2.0, 3.0, 4.0])
    assert J.live_resources() == with_plan and d.planned() == 3
    d.batch_i16(d_iq.ptr, 2 * L, L)
    d.plan_tunings([1], [9], [12004.0])  # takes the place of the consumed plan's arrays
    assert J.live_resources()[0] == with_plan[0]
    d.plan_tunings([], [], [])          # cleared: the plan's three arrays go
    cleared = J.live_resources()
    assert cleared[0] == with_plan[0] - 3 and cleared[1] < with_plan[1]
    d.plan_tunings([0], [1], [12005.0])
    d.batch_i16(d_iq.ptr + 4 * L, 2 * L, L)
    d.sync()
    del d
    assert J.live_resources() == before
    # a handle whose only plan was refused
    d = J.BpskTuned(96000, 8192, [12000.0, 12010.5], max_batch_samples=L)
    with pytest.raises(J.JsdrError, match="not a finite"):
        d.plan_tunings([0, 1], [5, 6], [12001.0, float("nan")])
    assert J.live_resources() == made
    del d
    assert J.live_resources() == before
