"""The live channel handle's C ABI (jsdr_bpsk_create_live_channels): declared, exported, and checked before any device
work; without a device it fails loudly (no CPU fallback)."""
import ctypes as C
import math
import os

import pytest

import java_sdr_amd as J

NEW = ["jsdr_bpsk_create_live_channels"]


def test_live_channel_symbol_is_declared_and_exported():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jsdr_hip.h")).read()
    lib = J.lib()
    for s in NEW:
        assert s in J.EXPORTED_SYMBOLS, s
        assert s + "(" in hdr, s
        assert hasattr(lib, s), s


def _create(nch, tunings, frame=2048, do_fft=None):
    h = C.c_void_p()
    tu = None if tunings is None else (C.c_double * max(len(tunings), 1))(*tunings)
    ff = None if do_fft is None else (C.c_int * max(len(do_fft), 1))(*do_fft)
    rc = J.lib().jsdr_bpsk_create_live_channels(C.byref(h), 96000, frame, 1, nch, tu, ff, None, C.c_int64(frame))
    return rc, h


@pytest.mark.parametrize("nch,tunings,frame,do_fft,what", [
    (0, [12000.0], 2048, None, "nchannels 0 outside"),
    (17, [12000.0] * 17, 2048, None, "nchannels 17 outside"),
    (2, None, 2048, None, "null tuning"),
    (2, [12000.0, math.nan], 2048, None, "not finite"),
    (2, [math.inf, 12000.0], 2048, [1, 0], "not finite"),
    # the frame rule holds whatever the initial modes: every channel may come to acquire
    (2, [12000.0, 13000.0], 400, None, "needs a frame of 416"),
    (2, [12000.0, 13000.0], 400, [0, 1], "needs a frame of 416"),
])
def test_create_live_channels_refuses_bad_arguments_before_device_work(nch, tunings, frame, do_fft, what):
    rc, h = _create(nch, tunings, frame, do_fft)
    assert rc != 0 and not h.value
    msg = J.lib().jsdr_last_error().decode()
    assert what in msg and "jsdr_bpsk_create_live_channels" in msg, msg


def test_create_live_channels_fails_loudly_without_a_device():
    if J.have_gpu():
        pytest.skip("GPU present")
    with pytest.raises(J.JsdrError):
        J.BpskChannels(96000, 8192, [12000, 24000], live=True)
