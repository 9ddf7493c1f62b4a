"""The C ABI of the BPSK scope's spectra (jsdr_bpsk_scope_spectra_i16 / _f32, jsdr_bpsk_scope_spec_layout,
jsdr_bpsk_scope_chunk): declared, exported, bound; the host-only column layout against tests/bpsk_scope_spectra.py's on a grid,
with its refusals; and the refusals of the spectra calls that need no device, on a stand-in handle as in
test_bpsk_scope_abi.py (a zeroed block reads as an exact tune-mode handle with a rate of 0 Hz, which no refused call may write
to).  What needs a real handle -- plot widths, alignment, lengths no kernel serves, and what the calls compute -- is
test_gpu_bpsk_scope_spectra.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bpsk_scope_spectra as SP
import java_sdr_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("jsdr_bpsk_scope_spectra_i16", "jsdr_bpsk_scope_spectra_f32", "jsdr_bpsk_scope_spec_layout", "jsdr_bpsk_scope_chunk")
TAIL = ("int plot_width, int32_t *tspec_dev, double *tpeak_dev, double *tpsd_dev, int32_t *dspec_dev, double *dpeak_dev, "
        "double *dpsd_dev, void *stream);")
PROTOS = (
    "int jsdr_bpsk_scope_spectra_i16(jsdr_bpsk *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc, "
    "double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev, " + TAIL,
    "int jsdr_bpsk_scope_spectra_f32(jsdr_bpsk *h, const float *iq_in_dev, int64_t stream_stride_f32, int64_t nsamples, "
    "double *tuned_dev, double *ds_dev, double *iq_dev, double *max_dev, int32_t *pts_dev, int8_t *bits_dev, " + TAIL,
    "int jsdr_bpsk_scope_spec_layout(int len, int plot_width, int32_t *first, int32_t *count, int cap);",
    "int jsdr_bpsk_scope_chunk(jsdr_bpsk *h, int frames_per_pass);",
)
LENGTHS = sorted({2, 3, 64, 9600} | {c["n"] for c in SP.CASES.values()} | {c["n"] * 9600 // c["rate"] for c in SP.CASES.values()})
WIDTHS = (1, 2, 17, 100, 749, 1024, 2048, 4097, 32768)


def _header():
    hdr = open(os.path.join(ROOT, "include", "jsdr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return re.sub(r"\s+", " ", hdr).replace(" ,", ",").replace(" ;", ";")


def test_the_symbols_are_declared_exported_and_bound():
    hdr = _header()
    for sym, proto in zip(SYMS, PROTOS):
        assert sym in J.EXPORTED_SYMBOLS, sym
        assert proto in hdr, proto
        assert hasattr(J.lib(), sym) and getattr(J.lib(), sym).restype is C.c_int, sym
    for m in ("scope_spectra_i16", "scope_spectra_f32", "scope_chunk"):
        assert callable(getattr(J.Bpsk, m)), m
    assert callable(J.scope_spec_layout)
    build = open(os.path.join(ROOT, "java-sdr_amd", "build.py")).read()
    assert '"bpsk_scope_spec.hip": ["-ffp-contract=off"]' in build


def test_the_layout_on_a_grid():
    """every (len, Wp) of the grid is served by the layout, equals the Python doubles, and stays inside psd[]: no pair of the grid
    is a refusal"""
    assert {102, 204, 409, 819, 960, 1024, 2048, 4410, 4800, 8192} <= set(LENGTHS)
    refused = []
    for length in LENGTHS:
        for Wp in WIDTHS:
            first, count = J.scope_spec_layout(length, Wp)
            want = SP.layout(length, Wp)
            assert np.array_equal(first, want[0]) and np.array_equal(count, want[1]), (length, Wp)
            if not (first.astype(np.int64) + count <= length).all():
                refused.append((length, Wp))
    assert refused == []


def _refused(rc, name, word):
    assert rc != 0, word
    msg = J.lib().jsdr_last_error().decode()
    assert msg.startswith(name + ":") and word in msg, (word, msg)


def test_the_layout_refuses():
    L = J.lib()
    a = np.full(8, -1, np.int32)
    p = a.ctypes.data_as(C.c_void_p)
    name = "jsdr_bpsk_scope_spec_layout"
    _refused(L.jsdr_bpsk_scope_spec_layout(1, 4, p, p, 8), name, "len=1 below 2")
    _refused(L.jsdr_bpsk_scope_spec_layout(204, 0, p, p, 8), name, "plot_width=0 outside 1 .. 32768")
    _refused(L.jsdr_bpsk_scope_spec_layout(204, 32769, p, p, 40000), name, "plot_width=32769 outside 1 .. 32768")
    _refused(L.jsdr_bpsk_scope_spec_layout(204, 9, p, p, 8), name, "cap=8 below plot_width=9")
    assert (a == -1).all()
    assert L.jsdr_bpsk_scope_spec_layout(204, 8, p, None, 8) == 0 and a.tolist() == SP.layout(204, 8)[0].tolist()


def _call(form, h, src, stride=64, nsamples=8, outs=(None,) * 6, width=749, new=(None,) * 6):
    L = J.lib()
    if form == "i16":
        return L.jsdr_bpsk_scope_spectra_i16(h, src, C.c_int64(stride), C.c_int64(nsamples), 0, 0, *outs, width, *new, None)
    return L.jsdr_bpsk_scope_spectra_f32(h, src, C.c_int64(stride), C.c_int64(nsamples), *outs, width, *new, None)


@pytest.mark.parametrize("form", ["i16", "f32"])
def test_refusals_name_their_reason_and_write_nothing(form):
    stand_in = (C.c_ubyte * 65536)()
    h = C.cast(stand_in, C.c_void_p)
    buf = np.zeros(256, np.float64)
    p = buf.ctypes.data_as(C.c_void_p)
    name = "jsdr_bpsk_scope_spectra_" + form
    src = "raw_dev" if form == "i16" else "iq_in_dev"
    _refused(_call(form, None, p), name, "null handle")
    _refused(_call(form, h, None), name, "null input " + src)
    _refused(_call(form, h, p, new=(p,) * 6), name, "rate=0 below 9600")   # (what the scope calls refuse, with their reason)
    _refused(_call(form, h, p, outs=(p,) * 6), name, "rate=0 below 9600")
    _refused(_call(form, h, p), name, "rate=0 below 9600")
    assert not any(stand_in) and not buf.any()


def test_chunk_refuses_without_a_handle():
    _refused(J.lib().jsdr_bpsk_scope_chunk(None, 1), "jsdr_bpsk_scope_chunk", "null handle")
    stand_in = (C.c_ubyte * 65536)()
    _refused(J.lib().jsdr_bpsk_scope_chunk(C.cast(stand_in, C.c_void_p), -1), "jsdr_bpsk_scope_chunk", "negative")
    assert not any(stand_in)
