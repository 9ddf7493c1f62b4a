"""The tuned handle's C ABI (jsdr_bpsk_create_tuned: every stream of a batch handle its own tuning): declared with its
prototypes, exported, bound, and checked before any device work; without a device it fails loudly (no CPU fallback).  The
tuner recurrence the device walks is also exported as a host function, and is checked here against a Python restatement."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import java_sdr_amd as J

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jsdr_hip.h")
PROTOTYPES = {
    "jsdr_bpsk_create_tuned": "int jsdr_bpsk_create_tuned(jsdr_bpsk **h, int rate, int nsamples_per_frame, int nstreams, "
                              "const double *tuning_hz, int64_t max_batch_samples);",
    "jsdr_bpsk_set_stream_tuning": "int jsdr_bpsk_set_stream_tuning(jsdr_bpsk *h, int stream, double tuning_hz);",
    "jsdr_bpsk_set_stream_tunings": "int jsdr_bpsk_set_stream_tunings(jsdr_bpsk *h, int first, int count, const double *tuning_hz);",
    "jsdr_bpsk_get_stream_tuning": "int jsdr_bpsk_get_stream_tuning(jsdr_bpsk *h, int stream, double *tuning_hz);",
    "jsdr_bpsk_tuner_walk_host": "int jsdr_bpsk_tuner_walk_host(double tu0, double tu_inc, int64_t n, uint16_t *k9_out, double *tu_end);",
}


def _code(text):
    """the header without its comments, white space folded"""
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))


def test_stream_tuning_symbols_are_declared_exported_and_bound():
    code = _code(open(HDR).read())
    lib = J.lib()
    for name, proto in PROTOTYPES.items():
        assert name in J.EXPORTED_SYMBOLS, name
        assert _code(proto).strip() in code, proto
        assert hasattr(lib, name), name
    for m in ("set_stream_tuning", "set_stream_tunings", "stream_tuning", "batch_i16", "batch_f32", "pack_slots", "state"):
        assert callable(getattr(J.BpskTuned, m, None)), m
    assert issubclass(J.BpskTuned, J.Bpsk) and callable(J.tuner_walk_host)


def test_header_names_what_a_tuned_handle_does_not_cover():
    text = open(HDR).read()
    start = text.index("Tuned handle:")
    comment = re.sub(r"\s+", " ", text[start:text.index("*/", start)])
    assert "Not covered" in comment
    tail = comment[comment.index("Not covered"):]
    for what in ("FFT-acquire", "FAST variant", "jsdr_group_*", "receive_*", "JNI / Java classes"):
        assert what in tail, what


@pytest.mark.parametrize("name,call", [
    ("jsdr_bpsk_set_stream_tuning", lambda lib: lib.jsdr_bpsk_set_stream_tuning(None, 0, C.c_double(12000.0))),
    ("jsdr_bpsk_set_stream_tunings", lambda lib: lib.jsdr_bpsk_set_stream_tunings(None, 0, 1, (C.c_double * 1)(12000.0))),
    ("jsdr_bpsk_get_stream_tuning", lambda lib: lib.jsdr_bpsk_get_stream_tuning(None, 0, C.byref(C.c_double()))),
])
def test_per_stream_calls_refuse_a_null_handle(name, call):
    assert call(J.lib()) != 0
    msg = J.lib().jsdr_last_error().decode()
    assert name in msg and "null" in msg, msg


@pytest.mark.parametrize("nstreams,tunings,what", [
    (2, None, "null tuning"),
    (0, [12000.0], "geometry"),
    (2, [12000.0, math.nan], "not a finite value below the rate"),
    (2, [math.inf, 12000.0], "not a finite value below the rate"),
    (2, [12000.0, 96000.0], "not a finite value below the rate"),
    (3, [0.0, -5000.0, 1e9], "stream 2"),
])
def test_create_tuned_refuses_bad_arguments_before_device_work(nstreams, tunings, what):
    h = C.c_void_p()
    tu = None if tunings is None else (C.c_double * len(tunings))(*tunings)
    assert J.lib().jsdr_bpsk_create_tuned(C.byref(h), 96000, 2048, nstreams, tu, C.c_int64(2048)) != 0 and not h.value
    msg = J.lib().jsdr_last_error().decode()
    assert "jsdr_bpsk_create_tuned" in msg and what in msg, msg
    assert J.lib().jsdr_bpsk_create_tuned(None, 96000, 2048, 1, (C.c_double * 1)(12000.0), C.c_int64(2048)) != 0
    assert "null handle pointer" in J.lib().jsdr_last_error().decode()


def test_create_tuned_fails_loudly_without_a_device():
    if J.have_gpu():
        pytest.skip("GPU present")
    with pytest.raises(J.JsdrError):
        J.BpskTuned(96000, 8192, [12000, 12010.5])


# ---- the recurrence, restated: Python floats are IEEE doubles, and Python never contracts a product and a sum
def _walk(tu, inc, n):
    two_pi = 2.0 * math.pi
    k9 = np.empty(n, np.uint16)
    for i in range(n):
        tu += inc
        if tu > two_pi:
            tu -= two_pi
        k9[i] = int(tu * 256.0 / two_pi) % 256 if tu > 0.0 else 256
    return k9, tu


N = 100000
CASES = [  # (tuning, rate, tu0)
    (12000.0, 96000, 0.0), (12000.0, 192000, 0.0), (12010.0, 96000, 0.0), (11990.5, 48000, 0.0), (8000.0, 44100, 0.0),
    (-250.5, 96000, 1.0),   # crosses 0 downward
    (12000.0, 96000, -3.0),  # crosses upward
    (0.0, 96000, 2.5),      # frozen
    (95999.5, 96000, 0.0),  # the largest increments: nearly every step wraps
]


@pytest.mark.parametrize("tuning,rate,tu0", CASES)
def test_tuner_walk_host_equals_the_restated_recurrence(tuning, rate, tu0):
    inc = 2.0 * math.pi * tuning / float(rate)
    k_ref, end_ref = _walk(tu0, inc, N)
    k, end = J.tuner_walk_host(tu0, inc, N)
    assert k.dtype == np.uint16 and len(k) == N
    assert np.array_equal(k, k_ref) and end == end_ref
    assert int(k.max()) <= 256
    if tuning == -250.5:
        assert k[0] < 256 and k[-1] == 256  # mixed, then passed through
    if tu0 == -3.0:
        assert k[0] == 256 and k[-1] < 256
    if tuning == 0.0:
        assert end == tu0 and len(set(k.tolist())) == 1
    # ... and from where that walk ended: the state after 10^5 steps as a start
    k2_ref, end2_ref = _walk(end_ref, inc, N)
    k2, end2 = J.tuner_walk_host(end, inc, N)
    assert np.array_equal(k2, k2_ref) and end2 == end2_ref


def test_tuner_walk_host_takes_no_samples_and_refuses_a_null_buffer():
    k, end = J.tuner_walk_host(1.25, 0.5, 0)
    assert len(k) == 0 and end == 1.25
    assert J.lib().jsdr_bpsk_tuner_walk_host(C.c_double(0.0), C.c_double(0.1), C.c_int64(4), None, None) != 0
    assert "jsdr_bpsk_tuner_walk_host" in J.lib().jsdr_last_error().decode()
    assert J.lib().jsdr_bpsk_tuner_walk_host(C.c_double(0.0), C.c_double(0.1), C.c_int64(-1), None, None) != 0
