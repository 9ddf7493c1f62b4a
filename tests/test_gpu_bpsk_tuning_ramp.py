"""GPU: ramp plans (jsdr_bpsk_plan_stream_ramps) -- tuning-plan entries whose tuning moves by a slope a sample.  A ramp is by
definition one step entry per sample, with the sample's tuning computed by one product and one sum in doubles, so there are two
references and no tolerance anywhere:
  (A) a twin BpskTuned on the same device buffer given plan_tunings with every ramp expanded to one step a sample (Python floats
      are IEEE doubles and Python never contracts a product and a sum) -- every stream, after every call: bits, trace, FEC rc /
      bit index / bytes, the counters, the state doubles, decoded[] and stream_tuning;
  (B) one-stream ordinary handles (Ref) cut at every sample of the ramp with reconfigure(tuning_n, 0, 0) in front of each, for
      short ramps -- so that the tests do not rest on the step path alone."""
import ctypes as C

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O
from test_gpu_bpsk_stream_tuning import _rc, mixed_input, same_counters, same_state
from test_gpu_bpsk_tuning_plan import Ref, plan_of, same_call, setup

pytestmark = pytest.mark.gpu


def expand(ramps, L):
    """{stream: [(at_sample, tuning, slope)]} -> {stream: [(at_sample, tuning)]}: a slope of zero is the step it is, a ramp one
    step per sample until the stream's next entry or the call's last sample"""
    out = {}
    for s, es in ramps.items():
        steps = []
        for i, (at, t, slope) in enumerate(es):
            end = es[i + 1][0] if i + 1 < len(es) else L
            if slope == 0.0:
                steps.append((at, t))
            else:
                steps.extend((n, t + float(n - at) * slope) for n in range(at, end))
        out[s] = steps
    return out


def ramps_of(ramps):
    """-> the four lists of plan_ramps"""
    st, at, tu, sl = [], [], [], []
    for s in sorted(ramps):
        for a, t, k in ramps[s]:
            st.append(s)
            at.append(a)
            tu.append(t)
            sl.append(k)
    return st, at, tu, sl


def same_as_twin(d, twin, S, what):
    for s in range(S):
        w = (what, s)
        assert np.array_equal(d.bits(s), twin.bits(s)), w
        assert np.array_equal(d.trace(s), twin.trace(s)), w
        fg, ft = d.fec_results(s), twin.fec_results(s)
        assert [(a, b) for a, b, _ in fg] == [(a, b) for a, b, _ in ft], w
        assert all(np.array_equal(x[2], y[2]) for x, y in zip(fg, ft)), w
        same_counters(d.counters(s), twin.counters(s))
        same_state(d.state(s), twin.state(s))
        assert np.array_equal(d.decoded(s), twin.decoded(s)), w
        assert d.stream_tuning(s) == twin.stream_tuning(s), w


def ramp_call(d, twin, S, buf, nrow, pos, L, ramps, f32=False, what="", refs=None):
    """one call of L samples: d with the ramp plan, the twin with the ramps expanded to steps, then every stream against the
    twin's.  refs {stream: Ref}: these streams also against one-stream handles cut at every entry of the expansion"""
    steps = expand(ramps, L)
    if ramps:
        d.plan_ramps(*ramps_of(ramps))
        twin.plan_tunings(*plan_of(steps))
    assert d.planned() == sum(len(v) for v in ramps.values())
    for h in (d, twin):
        if f32:
            h.batch_f32(buf.ptr + 8 * pos, 2 * nrow, L)
        else:
            h.batch_i16(buf.ptr + 4 * pos, 2 * nrow, L)
    assert d.planned() == 0
    if L >= 1000:  # (a call with outputs names its front end)
        sloped = any(k != 0.0 for es in ramps.values() for _, _, k in es)
        assert d.front_kernel_name() == ("k_front_pst_ramp" if sloped else "k_front_pst_plan" if ramps else "k_front_pst"), what
    same_as_twin(d, twin, S, what)
    for s, es in ramps.items():  # a ramp that runs to the call's end leaves the tuning of the call's last sample
        at, t, k = es[-1]
        assert d.stream_tuning(s) == (t if k == 0.0 else t + float(L - 1 - at) * k), (what, s)
    for s, ref in (refs or {}).items():
        same_call(d, s, ref, ref.call(pos, L, steps.get(s, ()), f32), (what, "one-stream reference", s))


def pair(rate, tunings, max_batch, n, seed):
    """a tuned handle, its twin and the one device buffer both read; stream s reads one of four inputs"""
    src = [mixed_input(seed + k, n, [13200.0], rate=rate)[0] for k in range(min(4, len(tunings)))]
    buf = J.DeviceBuffer.from_host(np.concatenate([src[s % len(src)] for s in range(len(tunings))]))
    return (J.BpskTuned(rate, 8192, tunings, max_batch_samples=max_batch), J.BpskTuned(rate, 8192, tunings, max_batch_samples=max_batch),
            buf)


# ---- 1
def test_ramps_at_the_history_checkpoint_and_tile_positions():
    first, L, after = 4099, 20000, 5000
    n = first + L + after
    P = [0, 1, 25, 26, 27, 63, 64, 65, 2559, 2560, 2561, 2586, L - 27, L - 26, L - 1]
    tunings = [12000.0, 12010.5, 11987.25, 12000.0, 300.75, 12000.5, 11999.0, 12000.0, 12001.5]
    S = len(tunings)
    d, refs, buf, _ = setup(96000, tunings, L, n, 140)  # (a Ref per stream is made; two are used)
    twin = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    held = {7: refs[7], 8: refs[8]}
    ramps = {
        0: [(a, 12000.0 + 7.25 * (i + 1) * (-1) ** i, 0.01 * (i + 1) * (-1) ** (i // 2)) for i, a in enumerate(P)],  # every position
        # (1: none)
        2: [(100, 11990.0, 0.003)],                             # from the middle of a block to the call's end: k is large at a block's start
        3: [(130, 12010.0, 0.02), (150, 12020.5, -0.03)],       # two ramps in one checkpoint block
        4: [(2560, 310.25, 0.5), (2561, 5.5, 0.25)],            # replaced a sample later
        5: [(64, 12000.5, 0.01), (2586, 12030.0, 0.0)],         # a ramp, then a hold
        6: [(25, 12010.0, 0.0), (L - 26, 11990.0, 0.0)],        # steps only
        7: [(63, 12005.0, 0.04), (63 + 140, 12010.75, 0.0)],    # short ramps that end in a hold: also against one-stream handles
        8: [(2559, 11995.0, -0.05), (2559 + 100, 11990.25, 0.0)],
    }
    ramp_call(d, twin, S, buf, n, 0, first, {}, what="before", refs=held)
    assert d.front_kernel_name() == "k_front_pst"
    ramp_call(d, twin, S, buf, n, first, L, ramps, what="ramps", refs=held)
    assert d.front_kernel_name() == "k_front_pst_ramp"
    assert d.stream_tuning(1) == 12010.5 and d.control()[0] == d.stream_tuning(0) == ramps[0][-1][1]  # (L - 1: k = 0)
    assert d.stream_tuning(2) == 11990.0 + float(L - 101) * 0.003
    # the plan was one-shot: the next call runs at the tunings the ramps ended on
    ramp_call(d, twin, S, buf, n, first + L, after, {}, what="after", refs=held)
    assert d.front_kernel_name() == "k_front_pst"


# ---- 2
def test_a_ramp_running_to_the_calls_end_and_continued_in_the_next_call():
    L = 12000
    n = 4 * L
    tunings = [12000.0, 11000.0, 12010.5]
    d, twin, buf = pair(96000, tunings, L, n, 150)
    ramp_call(d, twin, 3, buf, n, 0, L, {}, what="before")
    ramps = {0: [(500, 12000.0, 0.002)], 1: [(0, 11000.0, -0.001)]}
    ramp_call(d, twin, 3, buf, n, L, L, ramps, what="to the end")
    assert d.stream_tuning(0) == 12000.0 + float(L - 1 - 500) * 0.002 and d.stream_tuning(1) == 11000.0 + float(L - 1) * -0.001
    assert d.stream_tuning(2) == 12010.5 and d.control()[0] == d.stream_tuning(0)
    ramp_call(d, twin, 3, buf, n, 2 * L, L, {}, what="after, unplanned")  # the streams stand where their ramps ended
    assert d.front_kernel_name() == "k_front_pst"
    # continued: an entry at sample 0 of the next call with the tuning the line has there, and the same slope
    cont = {0: [(0, 12000.0 + float(L - 500) * 0.002, 0.002)], 1: [(0, 11000.0 + float(L) * -0.001, -0.001)]}
    ramp_call(d, twin, 3, buf, n, 3 * L, L, cont, what="continued")
    assert d.front_kernel_name() == "k_front_pst_ramp"


# ---- 3
def test_a_ramp_down_through_zero_and_back_up():
    L = 10000
    n = 3 * L
    d, twin, buf = pair(96000, [30.0, 12000.0, 12000.5], L, n, 160)
    ramp_call(d, twin, 3, buf, n, 0, L, {}, what="before")
    # 0 Hz at k = 600; from there tuPhase comes down, and stays at or below 0 from about sample 2700 on (index 256: passed through)
    ramp_call(d, twin, 3, buf, n, L, L, {0: [(100, 30.0, -0.05)], 2: [(70, 12000.5, 0.001)]}, what="down")
    assert d.state(0)[0] <= 0.0 and d.stream_tuning(0) < -400.0
    ramp_call(d, twin, 3, buf, n, 2 * L, L, {0: [(200, -464.0, 0.5)]}, what="up")
    assert d.state(0)[0] > 0.0 and d.stream_tuning(0) > 4000.0


# ---- 4
@pytest.mark.parametrize("L", [1, 25, 26, 77])
def test_ramp_calls_shorter_than_the_history(L):
    first, after = 4099, 3000
    n = first + L + after
    d, twin, buf = pair(96000, [12000.0, 12010.5, 11000.0], 4099, n, 170 + L)
    ramps = {0: [(0, 12020.0, 0.5)], 1: [(L - 1, 11990.5, -0.25)], 2: [(0, 11010.0, 1.0)] + ([(L - 1, 11020.25, 0.125)] if L > 1 else [])}
    ramp_call(d, twin, 3, buf, n, 0, first, {}, what="before")
    ramp_call(d, twin, 3, buf, n, first, L, ramps, what="short")
    ramp_call(d, twin, 3, buf, n, first + L, after, {}, what="after")
    assert [d.stream_tuning(s) for s in range(3)] == [12020.0 + float(L - 1) * 0.5, 11990.5, 11020.25 if L > 1 else 11010.0]


# ---- 5
def test_a_wave_of_ramping_stepping_and_idle_lanes():
    S, L = 70, 8192  # two workgroups of the walk: a full wave and six lanes
    n = 2 * L
    tunings = [11000.0 + 37.0 * s for s in range(S)]
    d, twin, buf = pair(96000, tunings, L, n, 180)
    ramps = {}
    for s in range(S):
        if s % 3 == 0:    # a ramp, no two from one sample; every fourth of them is held again before the call ends
            ramps[s] = [(19 + 53 * s, tunings[s] + 0.5, 0.0004 * (s + 1) * (-1) ** s)]
            if s % 4 == 0:
                ramps[s].append((5000 + 11 * s, tunings[s] - 2.25, 0.0))
        elif s % 3 == 1:  # steps
            ramps[s] = [(64 * s, tunings[s] + 3.0, 0.0), (64 * s + 1 + s, tunings[s] - 1.5, 0.0)]
    assert len({es[0][0] for es in ramps.values()}) == len(ramps)
    ramp_call(d, twin, S, buf, n, 0, L, ramps, what="mixed wave")
    ramp_call(d, twin, S, buf, n, L, L, {}, what="after")


# ---- 6
def test_float_ramp_calls_alternating_with_int16_calls():
    L = 6000
    forms = [True, False, True, True, False]  # f32?
    n = L * len(forms)
    tunings = [12000.5, -700.25, 23999.0]
    S = len(tunings)
    xs = [O.make_dbpsk_stream(61, s, n, noise_sigma=900.0)[0] for s in range(S)]
    b16 = J.DeviceBuffer.from_host(np.concatenate(xs))
    b32 = J.DeviceBuffer.from_host(np.concatenate([O.convert_i16(x).astype(np.float32) for x in xs]))  # JavaAudio's floats
    d = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    twin = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    for k, f32 in enumerate(forms):
        ramps = {0: [(k, 12000.5 + k, 0.01), (2560 + k, 11990.25, -0.002)], 2: [(25 + k, 23000.0 + k, 0.0), (26 + k, 23010.5, 0.05)]}
        if k == 3:
            ramps = {}
        ramp_call(d, twin, S, b32 if f32 else b16, n, k * L, L, ramps, f32=f32, what=("form", k))


# ---- 7
def test_zero_slopes_take_the_step_kernels_and_any_slope_the_ramp_kernels():
    L = 4096
    n = 4 * L
    tunings = [12000.0, 12010.5, 300.75]
    d, twin, buf = pair(96000, tunings, L, n, 190)
    steps = {0: [(5, 12001.0), (64, 12002.5)], 2: [(100, 310.0)]}
    d.plan_ramps(*ramps_of({s: [(a, t, 0.0) for a, t in es] for s, es in steps.items()}))
    twin.plan_tunings(*plan_of(steps))
    assert d.planned() == twin.planned() == 3
    for h in (d, twin):
        h.batch_i16(buf.ptr, 2 * n, L)
        assert h.front_kernel_name() == "k_front_pst_plan" and h.planned() == 0
    same_as_twin(d, twin, 3, "all slopes zero")
    d.plan_ramps([0, 0, 2], [5, 64, 100], [12001.0, 12002.5, 310.0], [0.0, -0.0, 1e-9])  # one slope that is not zero
    assert d.planned() == 3
    d.batch_i16(buf.ptr + 4 * L, 2 * n, L)
    assert d.front_kernel_name() == "k_front_pst_ramp" and d.planned() == 0
    d.batch_i16(buf.ptr + 4 * 2 * L, 2 * n, L)
    assert d.front_kernel_name() == "k_front_pst" and d.planned() == 0
    # a plan of either kind replaces a pending one of the other; no entries clears
    d.plan_ramps([1], [7], [12000.0], [0.25])
    d.plan_tunings([0, 1], [3, 4], [12000.0, 12001.0])
    assert d.planned() == 2
    d.plan_ramps([1], [7], [12000.0], [0.25])
    assert d.planned() == 1
    d.plan_ramps([], [], [], [])
    assert d.planned() == 0
    d.batch_i16(buf.ptr + 4 * 3 * L, 2 * n, L)
    assert d.front_kernel_name() == "k_front_pst"


# ---- 8
def test_save_after_a_ramp_call_restores_into_a_fresh_handle():
    L = 8000
    n = 3 * L
    tunings = [12000.0, 12010.5, 300.75]
    d, twin, buf = pair(96000, tunings, L, n, 200)
    ramp_call(d, twin, 3, buf, n, 0, L, {}, what="before")
    ramps = {0: [(100, 12020.0, 0.0031)], 2: [(L - 20, -500.0, 1.0 / 3.0)]}
    ramp_call(d, twin, 3, buf, n, L, L, ramps, what="ramps")
    blob = d.save()
    f = J.BpskTuned(96000, 8192, [1.0, 2.0, 3.0], max_batch_samples=L)
    f.restore(blob)  # (refuses a record whose tuPhaseInc is not 2 pi tuning / rate of its tuning: host and device agree on the end)
    assert f.planned() == 0
    assert [f.stream_tuning(s) for s in range(3)] == [d.stream_tuning(s) for s in range(3)]
    assert f.stream_tuning(0) == 12020.0 + float(L - 101) * 0.0031 and f.stream_tuning(2) == -500.0 + float(19) * (1.0 / 3.0)
    for h in (d, f, twin):
        h.batch_i16(buf.ptr + 4 * 2 * L, 2 * n, L)
    same_as_twin(d, twin, 3, "after save")
    same_as_twin(f, twin, 3, "restored")


# ---- 9
def test_refused_ramp_plans_and_calls_leave_the_handle_and_a_pending_plan_untouched():
    L = 2600
    tunings = [12000.0, 12010.5, -5000.0]
    S = len(tunings)
    lib = J.lib()
    a = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)
    b = J.BpskTuned(96000, 8192, tunings, max_batch_samples=L)

    def arr(ctype, v):
        return None if v is None else (ctype * len(v))(*v)

    def plan(st, at, tu, sl, n=None):
        return _rc(lambda: lib.jsdr_bpsk_plan_stream_ramps(a.h, arr(C.c_int32, st), arr(C.c_int64, at), arr(C.c_double, tu),
                                                           arr(C.c_double, sl), C.c_int64(len(st) if n is None else n)))

    refusals = [
        ("entry 1: slope .* is not finite", plan([0, 1], [5, 6], [100.0, 200.0], [0.5, float("nan")])),
        ("entry 0: slope .* is not finite", plan([0], [5], [100.0], [float("inf")])),
        ("null array", plan([0], [5], [100.0], None, 1)),
        # 95000 Hz + 1 Hz a sample reaches the rate at k = 1000: in front of the next entry (k = 1094) it is there
        ("entry 0: the ramp of stream 1 reaches .* in front of its next entry", plan([1, 1], [5, 1100], [95000.0, 12000.0], [1.0, 0.0])),
        ("entry 1: the ramp of stream 2 reaches .*inf", plan([0, 2, 2], [1, 5, 9], [1.0, -1e308, 0.0], [0.0, -1e308, 0.0])),
        ("out of order", plan([1, 0], [1, 1], [100.0, 100.0], [0.1, 0.1])),
        ("out of order", plan([0, 0], [5, 5], [100.0, 100.0], [0.1, 0.1])),
        ("below the rate", plan([0], [5], [96000.0], [-1.0])),
        ("stays pending", lambda: a.batch_i16(d_iq.ptr, 2 * n, 1500)),  # the pending plan has an entry at 1500
    ]
    n = L * (len(refusals) + 4)
    inputs = [O.make_dbpsk_stream(71, s, n, noise_sigma=900.0)[0] for s in range(S)]
    d_iq = J.DeviceBuffer.from_host(np.concatenate(inputs))
    pending = ([0, 2, 2], [7, 64, 1500], [12005.0, -4000.0, 100.5], [0.002, -0.01, 0.25])
    ends = [12005.0 + float(L - 1 - 7) * 0.002, 12010.5, 100.5 + float(L - 1 - 1500) * 0.25]
    for h in (a, b):
        h.batch_i16(d_iq.ptr, 2 * n, L)
    pos = L
    for what, bad in refusals:
        for h in (a, b):
            h.plan_ramps(*pending)
        with pytest.raises(J.JsdrError, match=what):
            bad()
        assert a.planned() == 3 and [a.stream_tuning(s) for s in range(S)] == tunings, what
        for h in (a, b):  # the refusal left the pending plan in force: both run it in this, longer call
            h.batch_i16(d_iq.ptr + 4 * pos, 2 * n, L)
            assert h.front_kernel_name() == "k_front_pst_ramp" and h.planned() == 0
        same_as_twin(a, b, S, what)
        assert [a.stream_tuning(s) for s in range(S)] == ends, what
        for h in (a, b):
            h.set_stream_tunings(0, tunings)
        pos += L
    # a ramp that reaches the rate at the call's last sample: 95000 Hz + 1 Hz a sample from sample 100 is at the rate at sample 1100
    for h in (a, b):
        h.plan_ramps([0, 1], [50, 100], [12001.0, 95000.0], [0.0, 1.0])
    for bad_L in (L, 1101):
        with pytest.raises(J.JsdrError, match="entry 1 of the pending ramp plan .*stream 1.* stays pending"):
            a.batch_i16(d_iq.ptr + 4 * pos, 2 * n, bad_L)
        assert a.planned() == 2 and [a.stream_tuning(s) for s in range(S)] == tunings
    for h in (a, b):  # a shorter call takes it: its last sample, 1099, has 95999 Hz
        h.batch_i16(d_iq.ptr + 4 * pos, 2 * n, 1100)
        assert h.front_kernel_name() == "k_front_pst_ramp" and h.planned() == 0
    same_as_twin(a, b, S, "the shorter call")
    assert [a.stream_tuning(s) for s in range(S)] == [12001.0, 95999.0, -5000.0]
    for h in (a, b):
        h.batch_i16(d_iq.ptr + 4 * (pos + 1100), 2 * n, L)
    same_as_twin(a, b, S, "after the shorter call")


@pytest.mark.parametrize("kind", ["ordinary", "channels"])
def test_ramp_plans_are_refused_on_handles_of_other_creators(kind):
    L = 4096
    make = {"ordinary": lambda: J.Bpsk(nstreams=2, max_batch_samples=L),
            "channels": lambda: J.BpskChannels(96000, 8192, [12000, 12010], max_batch_samples=L)}[kind]
    a, b = make(), make()
    lib = J.lib()
    x = O.make_dbpsk_stream(81, 0, 2 * L, noise_sigma=900.0)[0]
    d_iq = J.DeviceBuffer.from_host(np.concatenate([x, x]))
    for h in (a, b):
        J.Bpsk.batch_i16(h, d_iq.ptr, 4 * L, L)
    control = a.control()
    for call in (lambda: lib.jsdr_bpsk_plan_stream_ramps(a.h, (C.c_int32 * 1)(0), (C.c_int64 * 1)(5), (C.c_double * 1)(12010.0),
                                                         (C.c_double * 1)(0.01), C.c_int64(1)),
                 lambda: lib.jsdr_bpsk_plan_stream_ramps(a.h, None, None, None, None, C.c_int64(0))):
        assert call() != 0
        msg = lib.jsdr_last_error().decode()
        assert "jsdr_bpsk_plan_stream_ramps" in msg and "jsdr_bpsk_create_tuned" in msg
        assert a.control() == control
    for h in (a, b):
        J.Bpsk.batch_i16(h, d_iq.ptr + 4 * L, 4 * L, L)
    for s in range(2):
        for get in (J.Bpsk.counters, J.Bpsk.bits, J.Bpsk.trace, J.Bpsk.state):
            ga, gb = get(a, s), get(b, s)
            assert ga == gb if isinstance(ga, dict) else np.array_equal(ga, gb), (kind, s)


# ---- 10
def test_a_ramp_plan_owns_nothing_after_destroy():
    L = 4096
    x = O.make_dbpsk_stream(83, 0, 3 * L, noise_sigma=900.0)[0]
    d_iq = J.DeviceBuffer.from_host(np.concatenate([x, x]))
    J.binding.stream_sync()
    before = J.live_resources()
    d = J.BpskTuned(96000, 8192, [12000.0, 12010.5], max_batch_samples=L)
    made = J.live_resources()
    d.plan_ramps([0, 1, 1], [5, 64, 65], [12001.0, 12002.0, 12003.0], [0.01, 0.0, -0.02])
    with_plan = J.live_resources()
    assert with_plan[0] > made[0] and with_plan[1] > made[1]  # the device copy is the library's own, and counted
    with pytest.raises(J.JsdrError, match="not finite"):       # refused mid-validation: the entries before it were good
        d.plan_ramps([0, 1], [5, 64], [1.0, 2.0], [0.5, float("nan")])
    assert J.live_resources() == with_plan and d.planned() == 3
    d.batch_i16(d_iq.ptr, 2 * 3 * L, L)
    d.plan_tunings([1], [9], [12004.0])  # a step plan takes the place of the consumed ramp plan: one array fewer
    assert J.live_resources()[0] == with_plan[0] - 1
    d.plan_ramps([1], [9], [12004.0], [0.5])
    assert J.live_resources()[0] == with_plan[0]
    d.batch_i16(d_iq.ptr + 4 * L, 2 * 3 * L, L)
    d.plan_ramps([0], [1], [12005.0], [-0.5])
    d.plan_ramps([], [], [], [])         # cleared: the plan's four arrays go
    assert J.live_resources()[0] == with_plan[0] - 4
    d.plan_ramps([0], [1], [12005.0], [-0.5])
    d.batch_i16(d_iq.ptr + 4 * 2 * L, 2 * 3 * L, L)
    d.sync()
    del d
    assert J.live_resources() == before
