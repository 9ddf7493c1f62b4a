"""The C ABI of the BPSK scope (jsdr_bpsk_scope_i16 / _f32, jsdr_bpsk_scope_layout, jsdr_bpsk_scope_kernel): declared with the
prototypes the header documents, exported, bound, and refusing before any device work.  Without a device no handle can exist, so
what is refused of a handle here is refused of a stand-in: a zeroed block, which reads as an ordinary exact handle in the tune
mode with a rate of 0 Hz, and which no refused call may write to; on a box without a GPU a refusal that reached device code would
carry HIP's message, not the reason.  The refusals that need a real handle (channel, tuned and fast handles, FFT-acquire, frames,
strides, alignment, a ring length L < 1, a real handle of a rate below 9600) are test_gpu_bpsk_scope.py's, as is what the calls
compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import java_sdr_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("jsdr_bpsk_scope_i16", "jsdr_bpsk_scope_f32", "jsdr_bpsk_scope_layout", "jsdr_bpsk_scope_kernel")
PROTOS = (
    "int jsdr_bpsk_scope_i16(jsdr_bpsk *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc, "
    "double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev, void *stream);",
    "int jsdr_bpsk_scope_f32(jsdr_bpsk *h, const float *iq_in_dev, int64_t stream_stride_f32, int64_t nsamples, "
    "double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev, void *stream);",
    "int jsdr_bpsk_scope_layout(jsdr_bpsk *h, int64_t nsamples, int *ring_len, int64_t *origin, int64_t *g_first, int cap);",
    "const char *jsdr_bpsk_scope_kernel(jsdr_bpsk *h);",
)


def _header():
    hdr = open(os.path.join(ROOT, "include", "jsdr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return re.sub(r"\s+", " ", hdr).replace(" ,", ",").replace(" ;", ";")


def test_the_four_symbols_are_declared_exported_and_bound():
    hdr = _header()
    for sym, proto in zip(SYMS, PROTOS):
        assert sym in J.EXPORTED_SYMBOLS, sym
        assert proto in hdr, proto
        assert hasattr(J.lib(), sym), sym
    for sym in SYMS[:3]:
        assert getattr(J.lib(), sym).restype is C.c_int
    assert J.lib().jsdr_bpsk_scope_kernel.restype is C.c_char_p
    for m in ("scope_i16", "scope_f32", "scope_layout", "scope_kernel"):
        assert callable(getattr(J.Bpsk, m)), m


def test_the_header_states_every_refusal_and_the_unit_is_built():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "jsdr_hip.h")).read().replace(" * ", " "))
    for word in ("n_in not a multiple of n", "L < 1", "rate < 9600", "do_fft set or a mode switch pending", "every channel handle and "
                 "tuned handle", "the FAST variant", "tuned_dev: 16 bytes", "jsdr_bpsk_restore leaves origin"):
        assert word in hdr, word
    build = open(os.path.join(ROOT, "java-sdr_amd", "build.py")).read()
    assert '"bpsk_scope.hip": ["-ffp-contract=off"]' in build


def _call(form, h, src, stride=64, nsamples=8, outs=(None,) * 6):
    L = J.lib()
    if form == "i16":
        return L.jsdr_bpsk_scope_i16(h, src, C.c_int64(stride), C.c_int64(nsamples), 0, 0, *outs, None)
    return L.jsdr_bpsk_scope_f32(h, src, C.c_int64(stride), C.c_int64(nsamples), *outs, None)


def _refused(rc, name, word):
    assert rc != 0, word
    msg = J.lib().jsdr_last_error().decode()
    assert msg.startswith(name + ":") and word in msg, (word, msg)


@pytest.mark.parametrize("form", ["i16", "f32"])
def test_refusals_name_their_reason_and_write_nothing(form):
    stand_in = (C.c_ubyte * 65536)()
    h = C.cast(stand_in, C.c_void_p)
    buf = np.zeros(256, np.float64)
    p = buf.ctypes.data_as(C.c_void_p)
    name = "jsdr_bpsk_scope_" + form
    src = "raw_dev" if form == "i16" else "iq_in_dev"
    _refused(_call(form, None, p), name, "null handle")
    _refused(_call(form, h, None), name, "null input " + src)
    _refused(_call(form, h, p, outs=(p,) * 6), name, "rate=0 below 9600")
    _refused(_call(form, h, p), name, "rate=0 below 9600")  # (the checks come before the all-NULL call becomes the batch call)
    assert not any(stand_in) and not buf.any()


def test_layout_refuses_and_kernel_names_nothing_without_a_handle():
    stand_in = (C.c_ubyte * 65536)()
    h = C.cast(stand_in, C.c_void_p)
    ring, origin = C.c_int(-1), C.c_int64(-1)
    g = np.full(4, -1, np.int64)
    gp = g.ctypes.data_as(C.c_void_p)
    _refused(J.lib().jsdr_bpsk_scope_layout(None, C.c_int64(8), C.byref(ring), C.byref(origin), gp, 4), "jsdr_bpsk_scope_layout",
             "null handle")
    _refused(J.lib().jsdr_bpsk_scope_layout(h, C.c_int64(8), C.byref(ring), C.byref(origin), gp, 4), "jsdr_bpsk_scope_layout",
             "rate=0 below 9600")
    assert ring.value == -1 and origin.value == -1 and (g == -1).all() and not any(stand_in)
    assert J.lib().jsdr_bpsk_scope_kernel(None) == b""


def test_without_a_device_no_handle_can_be_made_to_scope_with():
    """(nothing of the scope: a scope call needs a handle, and without a device creating one is the loud failure)"""
    if J.have_gpu():
        return  # (a device is present: test_gpu_bpsk_scope.py runs the calls)
    with pytest.raises(J.JsdrError):
        J.Bpsk(rate=96000, blen=8192, nstreams=1, max_batch_samples=4096)
