"""The C ABI of jsdr_bpsk_batch_f32 (float IQ batches through the BPSK demodulator): declared, exported, bound, and its
handle-free refusal checked; without a device a handle cannot exist, so every other refusal is in test_gpu_bpsk_batch_f32.py."""
import ctypes as C
import os

import numpy as np
import pytest

import java_sdr_amd as J

SYM = "jsdr_bpsk_batch_f32"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_f32_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "jsdr_hip.h")).read()
    assert SYM in J.EXPORTED_SYMBOLS
    assert "int " + SYM + "(jsdr_bpsk *h, const float *iq_dev, int64_t stream_stride_f32, int64_t nsamples, void *stream);" in hdr
    assert hasattr(J.lib(), SYM)
    assert callable(J.Bpsk.batch_f32) and callable(J.BpskChannels.batch_f32)
    assert J.BpskChannels.batch_f32 is not J.Bpsk.batch_f32  # the override: its stride is between inputs


def test_the_header_names_what_batch_f32_does_not_cover():
    hdr = open(os.path.join(ROOT, "include", "jsdr_hip.h")).read()
    doc = hdr[:hdr.index("int " + SYM + "(")]
    doc = doc[doc.rindex("/*"):]
    for word in ("jsdr_group", "FAST", "JNI", "Java"):
        assert word in doc, word
    assert "float input through batch calls" not in hdr


def test_batch_f32_refuses_a_null_handle_with_a_message():
    buf = np.zeros(8, np.float32)
    rc = J.lib().jsdr_bpsk_batch_f32(None, buf.ctypes.data_as(C.c_void_p), C.c_int64(8), C.c_int64(4), None)
    assert rc != 0
    assert "null" in J.lib().jsdr_last_error().decode()


def test_batch_f32_fails_loudly_without_a_device():
    if J.have_gpu():
        return  # (with a device the call is test_gpu_bpsk_batch_f32.py's)
    with pytest.raises(J.JsdrError):
        J.Bpsk(nstreams=3, max_batch_samples=4096).batch_f32(0, 8192, 4096)
