"""Tuning plans (jsdr_bpsk_plan_stream_tunings: retunes inside the next batch call of a tuned handle, each stream at samples of
its own): the three calls are declared with their prototypes, exported and bound, and the one-stream host form of the planned
walk is checked against a Python restatement of FUNcubeBPSKDemod.java:384-390 with the increment switched at the entries, and
against jsdr_bpsk_tuner_walk_host run piecewise over the same cuts -- index for index, the end phase as a bit pattern."""
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
    "jsdr_bpsk_plan_stream_tunings": "int jsdr_bpsk_plan_stream_tunings(jsdr_bpsk *h, const int32_t *stream, const int64_t *at_sample, "
                                     "const double *tuning_hz, int64_t n);",
    "jsdr_bpsk_planned_tunings": "int jsdr_bpsk_planned_tunings(jsdr_bpsk *h, int64_t *n);",
    "jsdr_bpsk_tuner_walk_plan_host": "int jsdr_bpsk_tuner_walk_plan_host(double tu0, double tu_inc, int64_t n, const int64_t *at_sample, "
                                      "const double *inc_at, int64_t nev, uint16_t *k9_out, double *tu_end);",
}


def _code(text):
    """the header without its comments, white space folded"""
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))


def test_plan_symbols_are_declared_exported_and_bound():
    code = _code(open(HDR).read())
    lib = J.lib()
    for name, proto in PROTOTYPES.items():
        assert name in J.EXPORTED_SYMBOLS, name
        assert _code(proto).strip() in code, proto
        assert hasattr(lib, name), name
    for m in ("plan_tunings", "planned"):
        assert callable(getattr(J.BpskTuned, m, None)), m
    assert callable(J.tuner_walk_plan_host)


def test_header_states_what_a_plan_is_and_what_is_not_built():
    text = open(HDR).read()
    start = text.index("Tuning plans:")
    comment = re.sub(r"\s+", " ", text[start:text.index("*/", start)])
    for what in ("NEXT batch call", "dmMaxCorr is NOT zeroed", "one-shot", "jsdr_bpsk_save does not carry it", "stays pending"):
        assert what in comment, what
    tail = comment[comment.index("Not built"):]
    for what in ("JNI", "jsdr_group_*", "FAST", "FFT-acquire"):
        assert what in tail, what


def test_plan_calls_refuse_a_null_handle():
    lib = J.lib()
    one_s, one_a, one_t = (C.c_int32 * 1)(0), (C.c_int64 * 1)(0), (C.c_double * 1)(12000.0)
    assert lib.jsdr_bpsk_plan_stream_tunings(None, one_s, one_a, one_t, C.c_int64(1)) != 0
    msg = lib.jsdr_last_error().decode()
    assert "jsdr_bpsk_plan_stream_tunings" in msg and "null" in msg, msg
    assert lib.jsdr_bpsk_planned_tunings(None, C.byref(C.c_int64())) != 0
    msg = lib.jsdr_last_error().decode()
    assert "jsdr_bpsk_planned_tunings" in msg and "null" in msg, msg


# ---- the recurrence with a plan, restated: Python floats are IEEE doubles, and Python never contracts a product and a sum
def _walk_plan(tu, inc, n, at, incs):
    two_pi = 2.0 * math.pi
    k9 = np.empty(n, np.uint16)
    e = 0
    for i in range(n):
        if e < len(at) and at[e] == i:
            inc = incs[e]
            e += 1
        tu += inc
        if tu > two_pi:
            tu -= two_pi
        k9[i] = int(tu * 256.0 / two_pi) % 256 if tu > 0.0 else 256
    return k9, tu


def _piecewise(tu, inc, n, at, incs):
    """jsdr_bpsk_tuner_walk_host over the pieces the entries cut the n samples into"""
    cuts = [0] + [a for a in at if 0 < a < n] + [n]
    now = {a: v for a, v in zip(at, incs)}
    ks = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        inc = now.get(a, inc)
        k, tu = J.tuner_walk_host(tu, inc, b - a)
        ks.append(k)
    return np.concatenate(ks), tu


def _bits(x):
    return struct.pack("<d", x)


N = 4096
# name -> [(at_sample, tuning in Hz)]
PLANS = {
    "block_edges": [(0, 12010.0), (1, 11990.5), (63, 12020.0), (64, 12030.25), (65, 11000.0), (N - 1, 12000.0)],
    "consecutive": [(700, 12010.0), (701, 12020.0)],
    "three_in_one_block": [(130, 12010.0), (150, 11990.0), (191, 12005.5)],
    # down through 0 (index 256 appears), frozen, further down, and back up through 0 (index 256 goes away)
    "through_zero": [(100, 12000.5), (300, 0.0), (500, -500.0), (2500, 11990.0)],
    "none": [],
}


@pytest.mark.parametrize("rate", [96000, 192000])
@pytest.mark.parametrize("tu0", [0.0, 1.25])
@pytest.mark.parametrize("name", list(PLANS))
def test_tuner_walk_plan_host_equals_the_restated_recurrence_and_the_piecewise_walk(name, tu0, rate):
    at = [a for a, _ in PLANS[name]]
    incs = [2.0 * math.pi * f / float(rate) for _, f in PLANS[name]]
    inc0 = 2.0 * math.pi * 12000.0 / float(rate)
    k_ref, end_ref = _walk_plan(tu0, inc0, N, at, incs)
    k, end = J.tuner_walk_plan_host(tu0, inc0, N, at, incs)
    assert k.dtype == np.uint16 and len(k) == N
    assert np.array_equal(k, k_ref), np.flatnonzero(k != k_ref)[:8]
    assert _bits(end) == _bits(end_ref)
    k_p, end_p = _piecewise(tu0, inc0, N, at, incs)
    assert np.array_equal(k, k_p) and _bits(end) == _bits(end_p)
    if name == "none":
        k_h, end_h = J.tuner_walk_host(tu0, inc0, N)
        assert np.array_equal(k, k_h) and _bits(end) == _bits(end_h)
    elif name == "through_zero":  # index 256 is there, and only where Python says
        hit = np.flatnonzero(k == 256)
        assert hit.size and np.array_equal(hit, np.flatnonzero(k_ref == 256))
        assert 500 < hit[0] < 2500 <= hit[-1] < N - 1 and k[499] < 256 and k[-1] < 256
    else:  # the entries did something
        assert not np.array_equal(k, J.tuner_walk_host(tu0, inc0, N)[0])


def test_tuner_walk_plan_host_argument_checks():
    lib = J.lib()
    k9 = np.empty(8, np.uint16)
    end = C.c_double()
    args = (C.c_double(0.5), C.c_double(0.1), C.c_int64(8))
    # no entries and null arrays: the plain walk
    assert lib.jsdr_bpsk_tuner_walk_plan_host(*args, None, None, C.c_int64(0), k9.ctypes.data_as(C.c_void_p), C.byref(end)) == 0
    k_h, end_h = J.tuner_walk_host(0.5, 0.1, 8)
    assert np.array_equal(k9, k_h) and end.value == end_h
    k0, end0 = J.tuner_walk_plan_host(1.25, 0.5, 0)
    assert len(k0) == 0 and end0 == 1.25
    at, ia = (C.c_int64 * 2)(3, 5), (C.c_double * 2)(0.2, 0.3)
    bad = [
        (args + (at, ia, C.c_int64(2), None, None), "null"),                                         # null output with n > 0
        (args + (None, ia, C.c_int64(2), k9.ctypes.data_as(C.c_void_p), None), "null"),              # null positions with nev > 0
        (args + (at, None, C.c_int64(2), k9.ctypes.data_as(C.c_void_p), None), "null"),
        (args + (at, ia, C.c_int64(-1), k9.ctypes.data_as(C.c_void_p), None), "entries"),
        (args + ((C.c_int64 * 2)(5, 5), ia, C.c_int64(2), k9.ctypes.data_as(C.c_void_p), None), "out of order"),
        (args + ((C.c_int64 * 2)(-1, 5), ia, C.c_int64(2), k9.ctypes.data_as(C.c_void_p), None), "negative"),
        ((C.c_double(0.5), C.c_double(0.1), C.c_int64(-1), None, None, C.c_int64(0), None, None), "samples"),
    ]
    for a, what in bad:
        assert lib.jsdr_bpsk_tuner_walk_plan_host(*a) != 0, what
        msg = lib.jsdr_last_error().decode()
        assert "jsdr_bpsk_tuner_walk_plan_host" in msg and what in msg, msg
    # entries at or behind n are not reached
    k, e = J.tuner_walk_plan_host(0.5, 0.1, 8, [8, 100], [0.7, 0.9])
    assert np.array_equal(k, k_h) and e == end_h
