"""The demod channel handle's C ABI (jsdr_demod_create_channels and its per-channel controls): declared, exported and bound,
and checked before any device work; without a device it fails loudly (no CPU fallback)."""
import ctypes as C
import os

import pytest

import java_sdr_amd as J

NEW = ["jsdr_demod_create_channels", "jsdr_demod_channel_info", "jsdr_demod_configure_channel", "jsdr_demod_channel_weights",
       "jsdr_demod_get_channel", "jsdr_demod_channel_state"]


def test_demod_channel_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jsdr_hip.h")).read()
    lib = J.lib()
    for s in NEW:
        assert s in J.EXPORTED_SYMBOLS, s
        assert s + "(" in hdr, s
        assert hasattr(lib, s), s
    for m in ("configure_channel", "channel_weights", "channel_control", "channel_state", "channel_info", "batch_i16",
              "batch_f32", "batch_host_i16", "receive", "frame_stats"):
        assert callable(getattr(J.DemodChannels, m, None)), m


def _create(nin, nch, max_batch=2048, n=2048):
    h = C.c_void_p()
    rc = J.lib().jsdr_demod_create_channels(C.byref(h), 96000, n, nin, nch, C.c_int64(max_batch))
    return rc, h


@pytest.mark.parametrize("nin,nch,max_batch,what", [
    (1, 0, 2048, "nchannels"),
    (1, 17, 2048, "nchannels"),
    (0, 2, 2048, "ninputs"),
    (2, 2, 3000, "whole frames"),
    (65535, 2, 2048, "streams"),
    (4096, 16, 2048, "streams"),
    (1, 2, 2048 * 65536, "frames"),
])
def test_create_channels_refuses_bad_arguments_before_device_work(nin, nch, max_batch, what):
    rc, h = _create(nin, nch, max_batch)
    assert rc != 0 and not h.value
    msg = J.lib().jsdr_last_error().decode()
    assert what in msg and "jsdr_demod_create_channels" in msg, msg


def test_create_channels_refuses_a_null_handle_pointer():
    assert J.lib().jsdr_demod_create_channels(None, 96000, 2048, 1, 2, C.c_int64(2048)) != 0
    assert "null" in J.lib().jsdr_last_error().decode()


def test_per_channel_calls_refuse_a_null_handle():
    lib = J.lib()
    a, b = C.c_int(), C.c_int()
    f = C.c_float()
    assert lib.jsdr_demod_channel_info(None, C.byref(a), C.byref(b)) != 0
    assert lib.jsdr_demod_configure_channel(None, 0, 3, 1, 1, 1) != 0
    assert lib.jsdr_demod_channel_weights(None, 0, 1000, 9000, None, None) != 0
    assert lib.jsdr_demod_channel_state(None, 0, C.byref(f), C.byref(f)) != 0
    v = [C.c_int() for _ in range(6)]
    assert lib.jsdr_demod_get_channel(None, 0, *[C.byref(x) for x in v]) != 0


def test_create_channels_fails_loudly_without_a_device():
    if J.have_gpu():
        pytest.skip("GPU present")
    with pytest.raises(J.JsdrError):
        J.DemodChannels(96000, 2048, ninputs=2, nchannels=3)
