"""Ramp plans (jsdr_bpsk_plan_stream_ramps: tuning-plan entries that move by a slope a sample): the two calls are declared with
their prototypes, exported and bound, and the one-stream host form of the ramp walk is checked against its definition -- a ramp IS
one step entry per sample, so jsdr_bpsk_tuner_walk_plan_host given those entries, with the increments computed in Python floats
-- and against a Python restatement of FUNcubeBPSKDemod.java:384-390.  Index for index, the end phase and the end increment as
bit patterns."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

import java_sdr_amd as J

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jsdr_hip.h")
PROTOTYPES = {
    "jsdr_bpsk_plan_stream_ramps": "int jsdr_bpsk_plan_stream_ramps(jsdr_bpsk *h, const int32_t *stream, const int64_t *at_sample, "
                                   "const double *tuning_hz, const double *slope_hz_per_sample, int64_t n);",
    "jsdr_bpsk_tuner_walk_ramp_host": "int jsdr_bpsk_tuner_walk_ramp_host(double tu0, double tu_inc, int64_t n, int rate, "
                                      "const int64_t *at_sample, const double *tuning_at, const double *slope_at, int64_t nev, "
                                      "uint16_t *k9_out, double *tu_end, double *inc_end);",
}


def _code(text):
    """the header without its comments, white space folded"""
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))


def test_ramp_symbols_are_declared_exported_and_bound():
    code = _code(open(HDR).read())
    lib = J.lib()
    for name, proto in PROTOTYPES.items():
        assert name in J.EXPORTED_SYMBOLS, name
        assert _code(proto).strip() in code, proto
        assert hasattr(lib, name), name
    assert callable(getattr(J.BpskTuned, "plan_ramps", None))
    assert callable(J.tuner_walk_ramp_host)


def test_header_states_what_a_ramp_is_and_what_is_not_built():
    text = open(HDR).read()
    start = text.index("Ramp plans:")
    assert start > text.index("Tuning plans:")
    comment = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", text[start:text.index("*/", start)]))  # (the lines' " * " dropped)
    for what in ("NEXT batch call", "(double)k * slope", "each rounded by itself", "Zero slope", "LAST sample", "entry at sample 0",
                 "stays pending", "24 bytes an entry", "k_front_pst_ramp"):
        assert what in comment, what
    tail = comment[comment.index("Not built"):]
    for what in ("ordinary or channel handles", "JNI", "jsdr_group_*", "FAST", "FFT-acquire", "outlive a call"):
        assert what in tail, what


def test_plan_stream_ramps_refuses_a_null_handle():
    lib = J.lib()
    one_s, one_a, one_t, one_r = (C.c_int32 * 1)(0), (C.c_int64 * 1)(0), (C.c_double * 1)(12000.0), (C.c_double * 1)(0.001)
    for n, arrays in ((1, (one_s, one_a, one_t, one_r)), (0, (None, None, None, None))):
        assert lib.jsdr_bpsk_plan_stream_ramps(None, *arrays, C.c_int64(n)) != 0
        msg = lib.jsdr_last_error().decode()
        assert "jsdr_bpsk_plan_stream_ramps" in msg and "null" in msg, msg


# ---- the definition, restated: Python floats are IEEE doubles, and Python never contracts a product and a sum
def _tunings(n, ramps):
    """[(at_sample, tuning, slope)] -> the tuning of every sample 0 .. n - 1 (None before the first entry): the entry's own where
    the slope is zero, else one product and one sum"""
    out = [None] * n
    for e, (at, t, slope) in enumerate(ramps):
        end = ramps[e + 1][0] if e + 1 < len(ramps) else n
        for i in range(at, min(end, n)):
            out[i] = t if slope == 0.0 else t + float(i - at) * slope
    return out


def _walk(tu, inc, n, rate, ramps):
    """FUNcubeBPSKDemod.java:384-390 with tuPhaseInc = 2 pi tuning / rate (:196) of every sample's own tuning"""
    two_pi = 2.0 * math.pi
    k9 = np.empty(n, np.uint16)
    for i, t in enumerate(_tunings(n, ramps)):
        if t is not None:
            inc = 2.0 * math.pi * t / float(rate)
        tu += inc
        if tu > two_pi:
            tu -= two_pi
        k9[i] = int(tu * 256.0 / two_pi) % 256 if tu > 0.0 else 256
    return k9, tu, inc


def _as_steps(tu, inc, n, rate, ramps):
    """jsdr_bpsk_tuner_walk_plan_host given one entry per sample under an entry"""
    ts = _tunings(n, ramps)
    at = [i for i, t in enumerate(ts) if t is not None]
    incs = [2.0 * math.pi * ts[i] / rate for i in at]
    k, end = J.tuner_walk_plan_host(tu, inc, n, at, incs)
    return k, end, (incs[-1] if incs else inc)


def _bits(x):
    return struct.pack("<d", x)


N = 5003
# name -> [(at_sample, tuning in Hz, slope in Hz per sample)]
RAMPS = {
    "from_0": [(0, 12000.0, 0.0123)],
    "from_63": [(63, 11990.5, -0.0071)],
    "from_64": [(64, 12010.25, 0.25)],
    "from_65": [(65, 12000.0, 1.0 / 3.0)],
    "a_sample_apart": [(700, 12010.0, 0.01), (701, 11000.0, -0.02)],
    "ramp_then_hold": [(100, 12000.0, 0.05), (2100, 12100.0, 0.0)],
    # down through 0 Hz (reached at k = 400) and on below: once tuPhase has come down to 0 the samples pass through (index 256)
    "through_zero": [(300, 40.0, -0.1)],
    "not_reached": [(10, 12000.0, 0.01), (N, 5.0, 1.0), (N + 70, 6.0, 2.0)],
    "none": [],
}


@pytest.mark.parametrize("rate", [96000, 192000])
@pytest.mark.parametrize("tu0", [0.0, 1.25])
@pytest.mark.parametrize("name", list(RAMPS))
def test_tuner_walk_ramp_host_equals_one_step_a_sample_and_the_restated_recurrence(name, tu0, rate):
    ramps = RAMPS[name]
    inc0 = 2.0 * math.pi * 12000.0 / float(rate)
    k, end, inc_end = J.tuner_walk_ramp_host(tu0, inc0, N, rate, *([list(c) for c in zip(*ramps)] or [[], [], []]))
    assert k.dtype == np.uint16 and len(k) == N
    for ref in (_as_steps, _walk):
        k_ref, end_ref, inc_ref = ref(tu0, inc0, N, rate, ramps)
        assert np.array_equal(k, k_ref), (ref.__name__, np.flatnonzero(k != k_ref)[:8])
        assert _bits(end) == _bits(end_ref), ref.__name__
        assert _bits(inc_end) == _bits(inc_ref), ref.__name__
    k_h, end_h = J.tuner_walk_host(tu0, inc0, N)
    if name == "none":
        assert np.array_equal(k, k_h) and _bits(end) == _bits(end_h) and _bits(inc_end) == _bits(inc0)
        return
    assert not np.array_equal(k, k_h)  # the entries did something
    at, t, slope = [e for e in ramps if e[0] < N][-1]
    if slope != 0.0:  # the increment the stream leaves the walk with is the last sample's
        assert _bits(inc_end) == _bits(2.0 * math.pi * (t + float(N - 1 - at) * slope) / float(rate))
    if name == "through_zero":  # index 256 from the sample at which tuPhase has come down to 0, to the end, and only there
        hit = np.flatnonzero(k == 256)
        assert hit.size and 700 < hit[0] and hit[-1] == N - 1 and np.array_equal(hit, np.arange(hit[0], N))
        assert end <= 0.0 and inc_end < 0.0
    if name == "not_reached":
        k1, end1, inc1 = J.tuner_walk_ramp_host(tu0, inc0, N, rate, [10], [12000.0], [0.01])
        assert np.array_equal(k, k1) and _bits(end) == _bits(end1) and _bits(inc_end) == _bits(inc1)


def test_tuner_walk_ramp_host_argument_checks():
    lib = J.lib()
    k9 = np.empty(8, np.uint16)
    out = k9.ctypes.data_as(C.c_void_p)
    end, inc_end = C.c_double(), C.c_double()
    args = (C.c_double(0.5), C.c_double(0.1), C.c_int64(8), C.c_int(96000))
    # no entries and null arrays: the plain walk
    assert lib.jsdr_bpsk_tuner_walk_ramp_host(*args, None, None, None, C.c_int64(0), out, C.byref(end), C.byref(inc_end)) == 0
    k_h, end_h = J.tuner_walk_host(0.5, 0.1, 8)
    assert np.array_equal(k9, k_h) and end.value == end_h and inc_end.value == 0.1
    k0, end0, inc0 = J.tuner_walk_ramp_host(1.25, 0.5, 0, 96000)
    assert len(k0) == 0 and end0 == 1.25 and inc0 == 0.5
    at, ta, sa = (C.c_int64 * 2)(3, 5), (C.c_double * 2)(100.0, 200.0), (C.c_double * 2)(0.5, 0.0)
    bad = [
        (args + (at, ta, sa, C.c_int64(2), None, None, None), "null"),    # null output with n > 0
        (args + (None, ta, sa, C.c_int64(2), out, None, None), "null"),  # a null array with nev > 0
        (args + (at, None, sa, C.c_int64(2), out, None, None), "null"),
        (args + (at, ta, None, C.c_int64(2), out, None, None), "null"),
        (args + (at, ta, sa, C.c_int64(-1), out, None, None), "entries"),
        (args + ((C.c_int64 * 2)(5, 5), ta, sa, C.c_int64(2), out, None, None), "out of order"),
        (args + ((C.c_int64 * 2)(-1, 5), ta, sa, C.c_int64(2), out, None, None), "negative"),
        (args[:3] + (C.c_int(0), at, ta, sa, C.c_int64(2), out, None, None), "rate"),
        ((C.c_double(0.5), C.c_double(0.1), C.c_int64(-1), C.c_int(96000), None, None, None, C.c_int64(0), None, None, None), "samples"),
    ]
    for a, what in bad:
        assert lib.jsdr_bpsk_tuner_walk_ramp_host(*a) != 0, what
        msg = lib.jsdr_last_error().decode()
        assert "jsdr_bpsk_tuner_walk_ramp_host" in msg and what in msg, msg
    # the end outputs may be null
    assert lib.jsdr_bpsk_tuner_walk_ramp_host(*args, at, ta, sa, C.c_int64(2), out, None, None) == 0
    with pytest.raises(ValueError):
        J.tuner_walk_ramp_host(0.0, 0.1, 8, 96000, [1, 2], [1.0], [0.0, 0.0])
