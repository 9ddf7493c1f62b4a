"""The tuned channel handle's C ABI (jsdr_bpsk_create_tuned_channels: ninputs x nchannels demodulators, every channel of every
input its own tuning, the channels of an input reading one input row): declared with its prototype, exported, bound, and every
argument checked before any device work -- so all of this runs without a device."""
import ctypes as C
import math
import os
import re

import pytest

import java_sdr_amd as J

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jsdr_hip.h")
NAME = "jsdr_bpsk_create_tuned_channels"
PROTOTYPE = ("int jsdr_bpsk_create_tuned_channels(jsdr_bpsk **h, int rate, int nsamples_per_frame, int ninputs, int nchannels, "
             "const double *tuning_hz, int64_t max_batch_samples);")


def _code(text):
    """the header without its comments, white space folded"""
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))


def test_the_symbol_is_declared_exported_and_bound():
    assert NAME in J.EXPORTED_SYMBOLS
    assert _code(PROTOTYPE).strip() in _code(open(HDR).read())
    assert hasattr(J.lib(), NAME)
    assert issubclass(J.BpskTunedChannels, J.BpskTuned)
    for m in ("plan_tunings", "plan_ramps", "planned", "set_stream_tuning", "set_stream_tunings", "stream_tuning", "channel_info",
              "batch_i16", "batch_f32", "pack_slots"):
        assert callable(getattr(J.BpskTunedChannels, m, None)), m


def test_header_names_what_the_handle_refuses_and_does_not_cover():
    text = open(HDR).read()
    start = text.index("Tuned channel handle:")
    comment = re.sub(r"\s+", " ", text[start:text.index("*/", start)])
    for what in ("set_variant(FAST)", "receive_i16", "set_channel_tuning", "jsdr_bpsk_save", "do_fft = 1"):
        assert what in comment, what
    tail = comment[comment.index("Not covered"):]
    for what in ("FFT-acquire", "FAST variant", "checkpoints", "jsdr_group_*", "receive_*", "JNI / Java classes"):
        assert what in tail, what


def _create(h, ninputs, nchannels, tunings, rate=96000):
    tu = None if tunings is None else (C.c_double * len(tunings))(*tunings)
    return J.lib().jsdr_bpsk_create_tuned_channels(h, rate, 2048, ninputs, nchannels, tu, C.c_int64(2048))


@pytest.mark.parametrize("ninputs,nchannels,tunings,what", [
    (2, 2, None, "null tuning array"),
    (2, 0, [12000.0] * 4, "nchannels 0 outside 1 .. 16"),
    (2, 17, [12000.0] * 34, "nchannels 17 outside 1 .. 16"),
    (4096, 16, [12000.0] * 65536, "4096 inputs x 16 channels"),  # 65536 streams
    (0, 2, [12000.0] * 2, "geometry"),
    (2, 2, [12000.0, 12010.5, math.nan, 0.0], "channel 0 of input 1 is not a finite value below the rate"),
    (2, 2, [12000.0, math.inf, 12000.0, 0.0], "channel 1 of input 0 is not a finite value below the rate"),
    (2, 2, [12000.0, -5000.0, 0.0, 96000.0], "channel 1 of input 1 is not a finite value below the rate"),
])
def test_create_refuses_bad_arguments_before_device_work(ninputs, nchannels, tunings, what):
    h = C.c_void_p(1)
    assert _create(C.byref(h), ninputs, nchannels, tunings) != 0
    assert not h.value  # the handle pointer is cleared
    msg = J.lib().jsdr_last_error().decode()
    assert NAME in msg and what in msg, msg


def test_create_refuses_a_null_handle_pointer():
    assert _create(None, 2, 2, [12000.0] * 4) != 0
    msg = J.lib().jsdr_last_error().decode()
    assert NAME in msg and "null handle pointer" in msg, msg


def test_the_python_class_wants_one_tuning_per_channel_of_every_input():
    with pytest.raises(ValueError, match="ninputs \\* nchannels"):
        J.BpskTunedChannels(96000, 8192, 2, 3, [12000.0] * 5)
