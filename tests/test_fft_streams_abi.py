"""The C ABI of the strided batch and waterfall calls (jsdr_fft_batch_streams_i16 / _f32, jsdr_fft_waterfall_streams_i16 / _f32):
declared with the prototypes the header documents, exported, bound, and refusing bad arguments before any device work.  Without
a device no handle can exist, so the refusals past the null handle are made with a stand-in: a zeroed block, which reads as a
handle of frame size 0 -- the refusals that need the frame size (a stride below a stream's frames, a PSD stride below its rows)
are reached with values that are too small for any frame size -- and which no call may write to; on a box without a GPU a
refusal that reached device code would carry HIP's message, not the argument's name.  What the calls compute is
test_gpu_fft_streams.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import java_sdr_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("jsdr_fft_batch_streams_i16", "jsdr_fft_batch_streams_f32", "jsdr_fft_waterfall_streams_i16",
        "jsdr_fft_waterfall_streams_f32")
PROTOS = (
    "int jsdr_fft_batch_streams_i16(jsdr_fft *h, const int16_t *raw_dev, int nstreams, int64_t stream_stride_i16, "
    "int64_t frames_per_stream, int ic, int qc, float *psd_dev, int64_t psd_stream_stride_f32, void *stream);",
    "int jsdr_fft_batch_streams_f32(jsdr_fft *h, const float *iq_dev, int nstreams, int64_t stream_stride_f32, "
    "int64_t frames_per_stream, float *psd_dev, int64_t psd_stream_stride_f32, void *stream);",
    "int jsdr_fft_waterfall_streams_i16(jsdr_fft *h, const int16_t *raw_dev, int nstreams, int64_t stream_stride_i16, "
    "int64_t frames_per_stream, int ic, int qc, int width, uint32_t peak_rgb, uint32_t *pix_dev, float *max_dev, "
    "float *peak_dev, void *stream);",
    "int jsdr_fft_waterfall_streams_f32(jsdr_fft *h, const float *iq_dev, int nstreams, int64_t stream_stride_f32, "
    "int64_t frames_per_stream, int width, uint32_t peak_rgb, uint32_t *pix_dev, float *max_dev, float *peak_dev, "
    "void *stream);",
)


def _header():
    hdr = open(os.path.join(ROOT, "include", "jsdr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return re.sub(r"\s+", " ", hdr).replace(" ,", ",")


def test_the_four_symbols_are_declared_exported_and_bound():
    hdr = _header()
    for sym, proto in zip(SYMS, PROTOS):
        assert sym in J.EXPORTED_SYMBOLS, sym
        assert proto in hdr, proto
        assert hasattr(J.lib(), sym), sym
        assert getattr(J.lib(), sym).restype is C.c_int
    for m in ("batch_streams_i16", "batch_streams_f32", "waterfall_streams_i16", "waterfall_streams_f32"):
        assert callable(getattr(J.Fft, m)), m


def _batch(form, h, src, nstreams, stride, fps, psd, psd_stride):
    L = J.lib()
    if form == "i16":
        return L.jsdr_fft_batch_streams_i16(h, src, nstreams, C.c_int64(stride), C.c_int64(fps), 0, 0, psd, C.c_int64(psd_stride),
                                            None)
    return L.jsdr_fft_batch_streams_f32(h, src, nstreams, C.c_int64(stride), C.c_int64(fps), psd, C.c_int64(psd_stride), None)


def _waterfall(form, h, src, nstreams, stride, fps, width, pix):
    L = J.lib()
    if form == "i16":
        return L.jsdr_fft_waterfall_streams_i16(h, src, nstreams, C.c_int64(stride), C.c_int64(fps), 0, 0, width,
                                                C.c_uint32(0x00FFFF), pix, None, None, None)
    return L.jsdr_fft_waterfall_streams_f32(h, src, nstreams, C.c_int64(stride), C.c_int64(fps), width, C.c_uint32(0x00FFFF), pix,
                                            None, None, None)


def _refused(rc, name, word):
    assert rc != 0, word
    msg = J.lib().jsdr_last_error().decode()
    assert msg.startswith(name + ":") and word in msg, (word, msg)


@pytest.mark.parametrize("form", ["i16", "f32"])
def test_every_batch_refusal_names_its_argument_and_writes_neither_handle_nor_device(form):
    stand_in = (C.c_ubyte * 4096)()
    h = C.cast(stand_in, C.c_void_p)
    buf = np.zeros(256, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    name = "jsdr_fft_batch_streams_" + form
    src, stride = ("raw_dev", "stream_stride_i16") if form == "i16" else ("iq_dev", "stream_stride_f32")
    for args, word in (((None, p, 2, 64, 1, p, 0), "null handle"),
                       ((h, None, 2, 64, 1, p, 0), "null " + src),
                       ((h, p, 2, 64, 1, None, 0), "null psd_dev"),
                       ((h, p, 0, 64, 1, p, 0), "nstreams=0"),
                       ((h, p, -2, 64, 1, p, 0), "nstreams=-2"),
                       ((h, p, 2, 64, -1, p, 0), "frames_per_stream=-1"),
                       ((h, p, 2, 63, 1, p, 0), stride + "=63"),    # odd
                       ((h, p, 2, -4, 1, p, 0), stride + "=-4"),    # below a stream's frames, whatever the frame size
                       ((h, p, 2, 64, 3, p, 5), "psd_stream_stride_f32=5"),  # three rows take at least six floats
                       ((h, p, 2, 64, 3, p, -8), "psd_stream_stride_f32=-8")):
        _refused(_batch(form, *args), name, word)
    assert bytes(stand_in) == bytes(4096) and not buf.any()
    # no frames: nothing is launched, whatever the handle -- the call succeeds on a box without a device as well
    assert _batch(form, h, p, 3, 64, 0, p, 0) == 0
    assert _batch(form, h, p, 1, 7, 0, p, 0) == 0  # (one stream: its stride says nothing)


@pytest.mark.parametrize("form", ["i16", "f32"])
def test_every_waterfall_refusal_names_its_argument_and_writes_neither_handle_nor_device(form):
    stand_in = (C.c_ubyte * 4096)()
    h = C.cast(stand_in, C.c_void_p)
    buf = np.zeros(256, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    name = "jsdr_fft_waterfall_streams_" + form
    src, stride = ("raw_dev", "stream_stride_i16") if form == "i16" else ("iq_dev", "stream_stride_f32")
    for args, word in (((None, p, 2, 64, 1, 8, p), "null handle"),
                       ((h, None, 2, 64, 1, 8, p), "null " + src),
                       ((h, p, 2, 64, 1, 8, None), "null pix_dev"),
                       ((h, p, 0, 64, 1, 8, p), "nstreams=0"),
                       ((h, p, 2, 64, -5, 8, p), "frames_per_stream=-5"),
                       ((h, p, 2, 31, 1, 8, p), stride + "=31"),
                       ((h, p, 2, -2, 1, 8, p), stride + "=-2"),
                       ((h, p, 2, 64, 1, 0, p), "width=0"),
                       ((h, p, 2, 64, 1, -3, p), "width=-3")):
        _refused(_waterfall(form, *args), name, word)
    assert bytes(stand_in) == bytes(4096) and not buf.any()
    assert _waterfall(form, h, p, 3, 64, 0, 8, p) == 0


def test_without_a_device_the_calls_fail_loudly():
    if J.have_gpu():
        return  # (with a device the calls are test_gpu_fft_streams.py's)
    with pytest.raises(J.JsdrError):
        J.Fft(2048, 96000).batch_streams_i16(0, 2, 8192, 1, 0)
    with pytest.raises(J.JsdrError):
        J.Fft(800, 48000).waterfall_streams_f32(0, 2, 4000, 1, 400, 0)
