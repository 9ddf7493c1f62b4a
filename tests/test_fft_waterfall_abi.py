"""The C ABI of the fused fft.receive + waterfall.paintLine calls (jsdr_fft_waterfall_i16 / _f32 / _kernel): declared with the
prototypes the header documents, exported, bound, and refusing bad arguments before any device work.  Without a device no handle
can exist, so the refusals past the null handle are made with a stand-in: a zeroed block the calls must never look into, and on a
box without a GPU a refusal that reached device code would carry HIP's message, not the argument's name.  What the calls compute
is test_gpu_fft_waterfall.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import java_sdr_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("jsdr_fft_waterfall_i16", "jsdr_fft_waterfall_f32", "jsdr_fft_waterfall_kernel")
PROTOS = (
    "int jsdr_fft_waterfall_i16(jsdr_fft *h, const int16_t *raw_dev, int64_t nframes, int ic, int qc, int width, "
    "uint32_t peak_rgb, uint32_t *pix_dev, float *max_dev, float *peak_dev, void *stream);",
    "int jsdr_fft_waterfall_f32(jsdr_fft *h, const float *iq_dev, int64_t nframes, int width, uint32_t peak_rgb, "
    "uint32_t *pix_dev, float *max_dev, float *peak_dev, void *stream);",
    "const char *jsdr_fft_waterfall_kernel(jsdr_fft *h);",
)


def _header():
    hdr = open(os.path.join(ROOT, "include", "jsdr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return re.sub(r"\s+", " ", hdr).replace(" ,", ",")  # (a comment between a parameter and its comma leaves a space)


def test_the_three_symbols_are_declared_exported_and_bound():
    hdr = _header()
    for sym, proto in zip(SYMS, PROTOS):
        assert sym in J.EXPORTED_SYMBOLS, sym
        assert proto in hdr, proto
        assert hasattr(J.lib(), sym), sym
    assert callable(J.Fft.waterfall_i16) and callable(J.Fft.waterfall_f32) and callable(J.Fft.waterfall_kernel)
    assert J.lib().jsdr_fft_waterfall_kernel.restype is C.c_char_p
    assert J.lib().jsdr_fft_waterfall_kernel(None) == b""


def _call(form, h, src, nframes, width, pix):
    L = J.lib()
    if form == "i16":
        return L.jsdr_fft_waterfall_i16(h, src, C.c_int64(nframes), 0, 0, width, C.c_uint32(0x00FFFF), pix, None, None, None)
    return L.jsdr_fft_waterfall_f32(h, src, C.c_int64(nframes), width, C.c_uint32(0x00FFFF), pix, None, None, None)


@pytest.mark.parametrize("form", ["i16", "f32"])
def test_every_refusal_names_its_argument_and_touches_neither_handle_nor_device(form):
    stand_in = (C.c_ubyte * 4096)()  # never a handle: a refusal must not look into it
    h = C.cast(stand_in, C.c_void_p)
    buf = np.zeros(256, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    name = "jsdr_fft_waterfall_" + form
    for args, word in (((None, p, 1, 8, p), "null handle"),
                       ((h, None, 1, 8, p), "null raw_dev" if form == "i16" else "null iq_dev"),
                       ((h, p, 1, 8, None), "null pix_dev"),
                       ((h, p, 1, 0, p), "width=0"),
                       ((h, p, 1, -3, p), "width=-3"),
                       ((h, p, -1, 8, p), "nframes=-1")):
        assert _call(form, *args) != 0, word
        msg = J.lib().jsdr_last_error().decode()
        assert msg.startswith(name + ":") and word in msg, (word, msg)
    assert bytes(stand_in) == bytes(4096)
    # no frames: nothing is launched, whatever the handle -- the call succeeds on a box without a device as well
    assert _call(form, h, p, 0, 8, p) == 0


def test_without_a_device_the_calls_fail_loudly():
    if J.have_gpu():
        return  # (with a device the calls are test_gpu_fft_waterfall.py's)
    with pytest.raises(J.JsdrError):
        J.Fft(2048, 96000).waterfall_i16(0, 1, 1024, 0)
    with pytest.raises(J.JsdrError):
        J.Fft(800, 48000).waterfall_f32(0, 1, 400, 0)
