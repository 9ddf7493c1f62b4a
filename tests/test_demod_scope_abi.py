"""The C ABI of the demod scope (jsdr_demod_scope_layout, jsdr_demod_scope_i16 / _f32, jsdr_demod_scope_chunk,
jsdr_demod_scope_kernel): declared with the prototypes the header documents, exported, bound, and refusing bad arguments before
any device work; the host-only column schedules against tests/demod_scope.py's restatement; the restatement against the Java
loops letter by letter; and the census that keeps the trace cases meaningful.  Without a device no handle can exist, so the
refusals past the null handle are made with a stand-in: a zeroed block, which reads as an ordinary handle of frame size 0, no
streams and no room, and which no refused call may write to; on a box without a GPU a refusal that reached device code would
carry HIP's message, not the argument's name.  (The refusal of a channel handle needs a real one: test_gpu_demod_scope.py.)
What the calls compute is test_gpu_demod_scope.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import demod_scope as DS
import java_sdr_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("jsdr_demod_scope_layout", "jsdr_demod_scope_i16", "jsdr_demod_scope_f32", "jsdr_demod_scope_chunk",
        "jsdr_demod_scope_kernel")
PROTOS = (
    "int jsdr_demod_scope_layout(int n, int width, int32_t *trace_first, int32_t *trace_count, int32_t *spec_first, "
    "int32_t *spec_count, int cap);",
    "int jsdr_demod_scope_i16(jsdr_demod *h, const int16_t *raw_dev, int64_t stream_stride_i16, int64_t nsamples, int ic, int qc, "
    "int16_t *audio_dev, int64_t audio_stride_i16, int width, int height, int32_t *trace_dev, int32_t *spec_dev, float *dbg_dev, "
    "void *stream);",
    "int jsdr_demod_scope_f32(jsdr_demod *h, const float *iq_dev, int64_t stream_stride_f32, int64_t nsamples, "
    "int16_t *audio_dev, int64_t audio_stride_i16, int width, int height, int32_t *trace_dev, int32_t *spec_dev, float *dbg_dev, "
    "void *stream);",
    "int jsdr_demod_scope_chunk(jsdr_demod *h, int frames_per_pass);",
    "const char *jsdr_demod_scope_kernel(jsdr_demod *h);",
)


def _header():
    hdr = open(os.path.join(ROOT, "include", "jsdr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return re.sub(r"\s+", " ", hdr).replace(" ,", ",").replace(" ;", ";")


def test_the_five_symbols_are_declared_exported_and_bound():
    hdr = _header()
    for sym, proto in zip(SYMS, PROTOS):
        assert sym in J.EXPORTED_SYMBOLS, sym
        assert proto in hdr, proto
        assert hasattr(J.lib(), sym), sym
    for sym in SYMS[:4]:
        assert getattr(J.lib(), sym).restype is C.c_int
    assert J.lib().jsdr_demod_scope_kernel.restype is C.c_char_p
    for m in ("scope_i16", "scope_f32", "scope_chunk", "scope_kernel"):
        assert callable(getattr(J.Demod, m)), m
    assert callable(J.demod_scope_layout)


def _scope(form, h, src, stride, nsamples, audio, astride, width, height, trace=None, spec=None, dbg=None):
    L = J.lib()
    if form == "i16":
        return L.jsdr_demod_scope_i16(h, src, C.c_int64(stride), C.c_int64(nsamples), 0, 0, audio, C.c_int64(astride), width, height,
                                      trace, spec, dbg, None)
    return L.jsdr_demod_scope_f32(h, src, C.c_int64(stride), C.c_int64(nsamples), audio, C.c_int64(astride), width, height, trace,
                                  spec, dbg, None)


def _refused(rc, name, word):
    assert rc != 0, word
    msg = J.lib().jsdr_last_error().decode()
    assert msg.startswith(name + ":") and word in msg, (word, msg)


@pytest.mark.parametrize("form", ["i16", "f32"])
def test_every_refusal_names_its_argument_and_writes_neither_handle_nor_device(form):
    stand_in = (C.c_ubyte * 16384)()
    h = C.cast(stand_in, C.c_void_p)
    buf = np.zeros(256, np.float32)
    assert buf.ctypes.data % 16 == 0
    p = buf.ctypes.data_as(C.c_void_p)
    name = "jsdr_demod_scope_" + form
    src, stride = ("raw_dev", "stream_stride_i16") if form == "i16" else ("iq_dev", "stream_stride_f32")
    #          handle, input, stride, nsamples, audio, audio stride, width, height, trace, spec, dbg
    for args, word in (((None, p, 64, 8, p, 64, 8, 8, p, p, p), "null handle"),
                       ((h, None, 64, 8, p, 64, 8, 8, p, p, p), "null " + src),
                       ((h, p, 64, 8, None, 64, 8, 8, p, p, p), "null audio_dev"),
                       ((h, p, 64, 8, p, 64, 0, 8, p, None, None), "width=0"),
                       ((h, p, 64, 8, p, 64, -5, 8, None, None, p), "width=-5"),
                       ((h, p, 64, 8, p, 64, DS.WIDTH_CAP + 1, 8, p, None, None), "width=%d" % (DS.WIDTH_CAP + 1)),
                       ((h, p, 64, 8, p, 64, 8, -1, p, None, None), "height=-1"),
                       ((h, p, 64, 8, p, 64, 8, 8, p, p, p), "spec_dev with a frame of 0 samples"),  # (what jsdr_fft_create refuses)
                       ((h, p, 63, 8, p, 64, 8, 8, p, None, p), stride + "=63"),             # odd
                       ((h, p, 14, 8, p, 64, 8, 8, p, None, p), stride + "=14"),             # below 2 * nsamples
                       ((h, p, 64, 8, p, 61, 8, 8, p, None, p), "audio_stride_i16=61"),
                       ((h, p, 64, 8, p, 12, 8, 8, p, None, p), "audio_stride_i16=12"),
                       ((h, p, 64, 8, p, 64, 8, 8, None, None, p), "nsamples=8"),            # no whole frames of a 0-sample frame
                       ((h, p, 64, 0, p, 64, 8, 8, None, None, p), "nsamples=0"),
                       ((h, p, 64, -8, p, 64, 8, 8, None, None, None), "nsamples=-8"),       # (with no output as well)
                       ((h, p, 2 ** 40, 2 ** 36, p, 2 ** 40, 8, 8, None, None, p), "nsamples=%d" % 2 ** 36)):  # above max_batch_samples
        _refused(_scope(form, *args), name, word)
    assert bytes(stand_in) == bytes(16384) and not buf.any()
    L = J.lib()
    _refused(L.jsdr_demod_scope_chunk(None, 4), "jsdr_demod_scope_chunk", "null handle")
    _refused(L.jsdr_demod_scope_chunk(h, -1), "jsdr_demod_scope_chunk", "frames_per_pass=-1")
    assert bytes(stand_in) == bytes(16384)
    assert L.jsdr_demod_scope_kernel(None) == b""


def test_layout_refusals_write_nothing():
    L = J.lib()
    a = np.full(8, -7, np.int32)
    pa = a.ctypes.data_as(C.c_void_p)
    _refused(L.jsdr_demod_scope_layout(0, 4, pa, pa, pa, pa, 8), "jsdr_demod_scope_layout", "n=0")
    _refused(L.jsdr_demod_scope_layout(64, 0, pa, pa, pa, pa, 8), "jsdr_demod_scope_layout", "width=0")
    _refused(L.jsdr_demod_scope_layout(64, DS.WIDTH_CAP + 1, None, None, None, None, 0), "jsdr_demod_scope_layout",
             "width=%d" % (DS.WIDTH_CAP + 1))
    _refused(L.jsdr_demod_scope_layout(64, 9, pa, None, None, None, 8), "jsdr_demod_scope_layout", "cap=8")
    assert (a == -7).all()
    assert L.jsdr_demod_scope_layout(64, 9, None, None, None, None, 0) == 0  # the check alone
    # each array alone
    want = DS.layout(64, 8)
    for k in range(4):
        out = np.full(8, -7, np.int32)
        args = [None] * 4
        args[k] = out.ctypes.data_as(C.c_void_p)
        assert L.jsdr_demod_scope_layout(64, 8, *args, 8) == 0
        assert np.array_equal(out, want[k]), k


LAYOUT_CASES = sorted({(n, w) for n in DS.LAYOUT_N for w in DS.widths(n)})


def test_layout_is_the_float_arithmetic_on_the_grid():
    assert len(LAYOUT_CASES) > 80
    for n, W in LAYOUT_CASES:
        assert DS.layout_inside(n, W), (n, W)  # (the sweep found no pair that leaves sam[] or psd[]; the library's check agrees)
        got = J.demod_scope_layout(n, W)
        for g, w, what in zip(got, DS.layout(n, W), ("trace_first", "trace_count", "spec_first", "spec_count")):
            assert np.array_equal(g, w), (n, W, what)
        tf, tc, sf, sc = got
        assert (tc[:W - 1] == n // W).all() and tc[W - 1] == 0 and tf[W - 1] == 0
        assert sf[0] == 0 and sc[0] == 0 and (np.diff(sf[1:]) >= 0).all() and (np.diff(tf[:W - 1]) >= 0).all()
    # pi = 9.6: windows of 9 bins that start 9 or 10 apart, so one bin in every ten-odd is never looked at
    _, _, sf, sc = J.demod_scope_layout(9600, 1000)
    assert sc[1] == 9 and set(np.diff(sf[1:]).tolist()) == {9, 10} and sf[-1] + 9 <= 9600
    tf, tc, _, _ = J.demod_scope_layout(9600, 1000)
    assert tc[0] == 9 and tf[998] == 998 * 9  # scale is the INT quotient: samples behind 9 * 999 are never drawn


def test_the_restatement_is_the_java_loops():
    rng = np.random.default_rng(5)
    for n, W in ((2, 1), (2, 2), (2, 4), (7, 1), (7, 2), (7, 3), (7, 7), (7, 8), (7, 14), (64, 3), (64, 9), (64, 31), (64, 32), (64, 33),
                 (64, 64), (64, 65), (100, 7), (100, 24), (100, 50), (100, 51)):
        for a, b in zip(DS.layout(n, W), DS.layout_java(n, W)):
            assert np.array_equal(a, b), (n, W)
        for H, kind in ((0, 0), (3, 1), (400, 2), (1001, 3)):
            sam = rng.standard_normal(2 * n).astype(np.float32)
            psd = (rng.standard_normal(n) * 30 - 40).astype(np.float32)
            if kind == 1:    # NaN finals, NaN and infinite Qs, -inf and NaN bins
                sam[0::4] = np.nan
                sam[1::6] = np.inf
                sam[3::10] = np.nan
                psd[::3] = -np.inf
                psd[1::7] = np.nan
            elif kind == 2:  # saturating casts and wrapping sums
                with np.errstate(over="ignore"):
                    sam[2::4] *= np.float32(3e38)
                    sam[1::4] *= np.float32(1e8)
                    psd[::2] *= np.float32(1e36)
            elif kind == 3:  # exact ties: strict > keeps the first
                sam = np.round(sam * 2).astype(np.float32)
                psd = np.round(psd / 8).astype(np.float32)
            assert np.array_equal(DS.trace(sam, W, H), DS.trace_java(sam, W, H)), (n, W, H, "trace")
            assert np.array_equal(DS.spec(psd, W, H), DS.spec_java(psd, W, H)), (n, W, H, "spectrum")
    # getAbsMax as written: c follows r, the walk starts at o + 1 and steps over the finals
    a = [np.float32(v) for v in (1.0, -3.0, 100.0, 2.0, 100.0, -3.5)]
    assert DS.get_abs_max_java(a, 0, 6, 2) == np.float32(-3.5) and DS.get_abs_max_java(a, 0, 5, 2) == np.float32(-3.0)
    assert DS.get_abs_max_java(a, 0, 1, 2) == np.float32(1.0) and DS.get_abs_max_java(a, 0, 0, 2) == np.float32(1.0)
    nan = np.float32(np.nan)
    assert np.isnan(DS.get_abs_max_java([nan, np.float32(5.0)], 0, 2, 2))          # nothing beats a NaN r
    assert DS.get_abs_max_java([np.float32(1.0), nan], 0, 2, 2) == np.float32(1.0)  # and a NaN beats nothing


def test_java_int_and_wrap():
    x = np.array([0.0, -0.0, 1.9, -1.9, 2147483520.0, 2147483648.0, -2147483648.0, -3e9, 3e38, -3e38, np.inf, -np.inf, np.nan, 1e-40],
                 np.float32)
    want = [0, 0, 1, -1, 2147483520, DS.INT_MAX, DS.INT_MIN, DS.INT_MIN, DS.INT_MAX, DS.INT_MIN, DS.INT_MAX, DS.INT_MIN, 0, 0]
    assert DS.java_int(x).tolist() == want
    assert DS.wrap32([100 - DS.INT_MIN, 250 + DS.INT_MAX, 5 - 7]).tolist() == [DS.INT_MIN + 100, DS.INT_MIN + 249, -2]


def test_the_census_that_keeps_the_trace_cases_meaningful():
    golden = DS.load()
    assert sorted(golden) == sorted(DS.CENSUS_CASES)
    for name, (n, W, mode, sw, band, designed) in DS.CENSUS_CASES.items():
        assert n // W >= 2 and mode != DS.OFF, name
        c = DS.census_of(name)
        assert c == golden[name], (name, c, golden[name])
        assert c["final"] + c["first_q"] + c["later_q"] == c["columns"] == DS.S * sum(DS.CALLS) * (W - 1), name
        for outcome in designed:
            assert c[outcome] >= 1, (name, outcome, c)
        if (n // W) // 2 < 2:
            assert c["later_q"] == 0, name  # one Q a column: no later one exists


def test_without_a_device_the_calls_fail_loudly():
    if J.have_gpu():
        return  # (with a device the calls are test_gpu_demod_scope.py's)
    with pytest.raises(J.JsdrError):
        J.Demod(96000, 2048, 1, 2048)
