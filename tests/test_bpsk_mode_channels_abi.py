"""The C ABI of a channel handle with FFT-acquire channels (jsdr_bpsk_create_mode_channels, jsdr_bpsk_acq_last_launch):
declared, exported, and checked before any device work; without a device it fails loudly (no CPU fallback)."""
import ctypes as C
import math
import os

import pytest

import java_sdr_amd as J

NEW = ["jsdr_bpsk_create_mode_channels", "jsdr_bpsk_acq_last_launch"]


def test_mode_channel_symbols_are_declared_and_exported():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jsdr_hip.h")).read()
    lib = J.lib()
    for s in NEW:
        assert s in J.EXPORTED_SYMBOLS, s
        assert s + "(" in hdr, s
        assert hasattr(lib, s), s


def _create(nch, tunings, do_fft, frame=2048, nin=1):
    h = C.c_void_p()
    tu = None if tunings is None else (C.c_double * max(len(tunings), 1))(*tunings)
    ff = None if do_fft is None else (C.c_int * max(len(do_fft), 1))(*do_fft)
    rc = J.lib().jsdr_bpsk_create_mode_channels(C.byref(h), 96000, frame, nin, nch, tu, ff, None, C.c_int64(frame))
    return rc, h


@pytest.mark.parametrize("nch,tunings,do_fft,frame,what", [
    (0, [12000.0], [1], 2048, "nchannels"),
    (17, [12000.0] * 17, [1] * 17, 2048, "nchannels"),
    (2, None, [1, 0], 2048, "null tuning"),
    (2, [12000.0, math.nan], [1, 0], 2048, "not finite"),
    (2, [math.inf, 12000.0], None, 2048, "not finite"),
    (2, [12000.0, 24000.0], [0, 1], 400, "below 416"),
])
def test_create_mode_channels_refuses_bad_arguments_before_device_work(nch, tunings, do_fft, frame, what):
    rc, h = _create(nch, tunings, do_fft, frame)
    assert rc != 0 and not h.value
    assert what in J.lib().jsdr_last_error().decode()


def test_acq_last_launch_refuses_null_arguments():
    a = C.c_int64()
    assert J.lib().jsdr_bpsk_acq_last_launch(None, C.byref(a), C.byref(a)) != 0
    assert "null" in J.lib().jsdr_last_error().decode()


def test_create_mode_channels_fails_loudly_without_a_device():
    if J.have_gpu():
        pytest.skip("GPU present")
    with pytest.raises(J.JsdrError):
        J.BpskChannels(96000, 8192, [12000, 24000], do_fft=[1, 0])
    with pytest.raises(J.JsdrError):
        J.BpskChannels(96000, 8192, [12000, 24000], do_fft=[0, 0])
