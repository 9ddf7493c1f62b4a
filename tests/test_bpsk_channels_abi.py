"""The channel handle's C ABI (jsdr_bpsk_create_channels and its controls): declared, exported, and checked before any
device work; without a device it fails loudly (no CPU fallback)."""
import ctypes as C
import math
import os

import pytest

import java_sdr_amd as J

NEW = ["jsdr_bpsk_create_channels", "jsdr_bpsk_channel_info", "jsdr_bpsk_set_channel_tuning", "jsdr_bpsk_set_channel_mode",
       "jsdr_bpsk_get_channel_control"]


def test_channel_symbols_are_declared_and_exported():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jsdr_hip.h")).read()
    lib = J.lib()
    for s in NEW:
        assert s in J.EXPORTED_SYMBOLS, s
        assert s + "(" in hdr, s
        assert hasattr(lib, s), s


def _create(nch, tunings, nin=1):
    h = C.c_void_p()
    tu = None if tunings is None else (C.c_double * max(len(tunings), 1))(*tunings)
    rc = J.lib().jsdr_bpsk_create_channels(C.byref(h), 96000, 2048, nin, nch, tu, None, C.c_int64(2048))
    return rc, h


@pytest.mark.parametrize("nch,tunings,what", [
    (0, [12000.0], "nchannels"),
    (17, [12000.0] * 17, "nchannels"),
    (2, None, "null tuning"),
    (2, [12000.0, math.nan], "not finite"),
    (2, [math.inf, 12000.0], "not finite"),
])
def test_create_channels_refuses_bad_arguments_before_device_work(nch, tunings, what):
    rc, h = _create(nch, tunings)
    assert rc != 0 and not h.value
    assert what in J.lib().jsdr_last_error().decode()


def test_create_channels_fails_loudly_without_a_device():
    if J.have_gpu():
        pytest.skip("GPU present")
    with pytest.raises(J.JsdrError):
        J.BpskChannels(96000, 8192, [12000, 24000])
