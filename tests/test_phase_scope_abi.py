"""The C ABI of the batched phase scope (jsdr_phase_layout, jsdr_phase_scope_i16 / _f32, jsdr_phase_scope_kernel): declared with
the prototypes the header documents, exported, bound, and refusing bad arguments before any device work; and the host-only
schedule, jsdr_phase_layout, against the oracle's pix and a Python restatement of the float recurrence.  Without a device no
handle can exist, so the refusals past the null handle are made with a stand-in: a zeroed block, which reads as a handle of frame
size 0 and which no call may write to; on a box without a GPU a refusal that reached device code would carry HIP's message, not
the argument's name.  What the calls compute is test_gpu_phase_scope.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O
import phase_scope as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("jsdr_phase_layout", "jsdr_phase_scope_i16", "jsdr_phase_scope_f32", "jsdr_phase_scope_kernel")
PROTOS = (
    "int jsdr_phase_layout(int n, int bx, int32_t *pix_host, int32_t *first_host, int32_t *count_host, int cap, int *ncol);",
    "int jsdr_phase_scope_i16(jsdr_phase *h, const int16_t *raw_dev, int nstreams, int64_t stream_stride_i16, "
    "int64_t frames_per_stream, int ic, int qc, int bx, int half_size, int quarter_height, float *max_dev, float *avg_dev, "
    "int32_t *pts_dev, void *stream);",
    "int jsdr_phase_scope_f32(jsdr_phase *h, const float *iq_dev, int nstreams, int64_t stream_stride_f32, "
    "int64_t frames_per_stream, int bx, int half_size, int quarter_height, float *max_dev, float *avg_dev, int32_t *pts_dev, "
    "void *stream);",
    "const char *jsdr_phase_scope_kernel(jsdr_phase *h);",
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
    for sym in SYMS[:3]:
        assert getattr(J.lib(), sym).restype is C.c_int
    assert J.lib().jsdr_phase_scope_kernel.restype is C.c_char_p
    for m in ("scope_i16", "scope_f32", "scope_kernel"):
        assert callable(getattr(J.Phase, m)), m
    assert callable(J.phase_layout)


def _scope(form, h, src, nstreams, stride, fps, bx, mx, avg=None, pts=None):
    L = J.lib()
    if form == "i16":
        return L.jsdr_phase_scope_i16(h, src, nstreams, C.c_int64(stride), C.c_int64(fps), 0, 0, bx, 100, 50, mx, avg, pts, None)
    return L.jsdr_phase_scope_f32(h, src, nstreams, C.c_int64(stride), C.c_int64(fps), bx, 100, 50, mx, avg, pts, None)


def _refused(rc, name, word):
    assert rc != 0, word
    msg = J.lib().jsdr_last_error().decode()
    assert msg.startswith(name + ":") and word in msg, (word, msg)


@pytest.mark.parametrize("form", ["i16", "f32"])
def test_every_refusal_names_its_argument_and_writes_neither_handle_nor_device(form):
    stand_in = (C.c_ubyte * 4096)()
    h = C.cast(stand_in, C.c_void_p)
    buf = np.zeros(256, np.float32)
    assert buf.ctypes.data % 16 == 0
    p = buf.ctypes.data_as(C.c_void_p)
    off = lambda k: C.c_void_p(buf.ctypes.data + k)  # noqa: E731
    name = "jsdr_phase_scope_" + form
    src, stride = ("raw_dev", "stream_stride_i16") if form == "i16" else ("iq_dev", "stream_stride_f32")
    for args, word in (((None, p, 2, 64, 1, 8, p), "null handle"),
                       ((h, None, 2, 64, 1, 8, p), "null " + src),
                       ((h, p, 2, 64, 1, 8, None), "null max_dev"),
                       ((h, p, 0, 64, 1, 8, p), "nstreams=0"),
                       ((h, p, -2, 64, 1, 8, p), "nstreams=-2"),
                       ((h, p, 2, 64, -1, 8, p), "frames_per_stream=-1"),
                       ((h, p, 2, 2 ** 40, 2 ** 30, 8, p), "rows"),          # 2 x 2^30 rows do not fit 31 bits
                       ((h, p, 1, 64, 2 ** 31, 8, p), "rows"),
                       ((h, p, 2, 64, 1, -1, p), "bx=-1"),
                       ((h, p, 2, 63, 1, 8, p), stride + "=63"),            # odd
                       ((h, p, 2, -4, 1, 8, p), stride + "=-4"),            # below a stream's frames, whatever the frame size
                       ((h, off(2), 2, 64, 1, 8, p), src + " is not aligned"),
                       ((h, p, 2, 64, 1, 8, p, p, off(8)), "pts_dev"),      # a row entry of pts_dev is 16 bytes
                       ((h, p, 2, 64, 1, 8, p, off(4), p), "avg_dev")):
        _refused(_scope(form, *args), name, word)
    assert bytes(stand_in) == bytes(4096) and not buf.any()
    # no frames: nothing is launched, whatever the handle -- the call succeeds on a box without a device as well
    assert _scope(form, h, p, 3, 64, 0, 8, p, p, p) == 0
    assert _scope(form, h, p, 1, 7, 0, 0, p) == 0  # (one stream: its stride says nothing)
    assert bytes(stand_in) == bytes(4096) and not buf.any()


def test_layout_refusals_and_ncol_is_always_set():
    L = J.lib()
    ncol = C.c_int(77)
    _refused(L.jsdr_phase_layout(600, 4, None, None, None, 0, None), "jsdr_phase_layout", "null ncol")
    _refused(L.jsdr_phase_layout(0, 4, None, None, None, 0, C.byref(ncol)), "jsdr_phase_layout", "n=0")
    assert ncol.value == 0
    _refused(L.jsdr_phase_layout(600, -3, None, None, None, 0, C.byref(ncol)), "jsdr_phase_layout", "bx=-3")
    pix = np.full(8, -7, np.int32)
    ncol.value = 77
    _refused(L.jsdr_phase_layout(600, 63, pix.ctypes.data_as(C.c_void_p), None, None, 8, C.byref(ncol)), "jsdr_phase_layout", "cap=8")
    k63 = PS.layout(600, 63)[0].size
    assert ncol.value == k63 > 8 and (pix == -7).all()  # the count is reported, nothing is written
    # each array alone
    for k in range(3):
        out = np.full(k63, -7, np.int32)
        args = [None, None, None]
        args[k] = out.ctypes.data_as(C.c_void_p)
        assert L.jsdr_phase_layout(600, 63, *args, k63, C.byref(ncol)) == 0
        assert np.array_equal(out, PS.layout(600, 63)[k])


LAYOUT_CASES = sorted({(n, bx) for n in PS.GRID_N for bx in PS.grid_bx(n)} | set(PS.CENSUS) | {(9600, 1), (8194, 512), (19200, 1024)})


def test_layout_is_the_float_recurrence_on_the_grid():
    for n, bx in LAYOUT_CASES:
        pix, first, count = J.phase_layout(n, bx)
        opix, _, _ = O.phase_columns(np.zeros(2 * n, np.float32), bx)
        assert np.array_equal(pix, opix), (n, bx, "pix against the oracle")
        ppix, pfirst, pcount = PS.layout(n, bx)
        assert np.array_equal(pix, ppix) and np.array_equal(first, pfirst) and np.array_equal(count, pcount), (n, bx)
        # columns tile the samples from 0 on, in order, one sample at least, n at most in all
        assert (count >= 1).all() and np.array_equal(first, np.concatenate([[0], np.cumsum(count)[:-1]])[:count.size])
        assert count.sum() <= n and pix.size <= n


def test_the_census_that_keeps_the_grid_meaningful():
    for (n, bx), (ncol, left) in PS.CENSUS.items():
        pix, first, count = J.phase_layout(n, bx)
        assert pix.size == ncol, (n, bx, pix.size)
        if left is not None:
            assert n - int(count.sum()) == left, (n, bx, n - int(count.sum()))
    # 600 additions of 1/600 in float stay below 1: no column at all, where the rational schedule closes one
    assert PS.layout_exact(600, 1)[0].size == 1
    # the float schedule is not the rational one
    for n, bx in ((9600, 700), (9600, 1024)):
        _, first, count = J.phase_layout(n, bx)
        efirst, ecount = PS.layout_exact(n, bx)
        assert first.size == efirst.size == bx and not np.array_equal(first, efirst), (n, bx)
    # one-sample columns whose pix jumps past lpix + 1
    for bx in (65, 128, 200):
        pix, first, count = J.phase_layout(64, bx)
        assert (count == 1).all() and (np.diff(np.concatenate([[0], pix])) > 1).any(), bx
    # more columns than a workgroup has threads
    assert J.phase_layout(2048, 2048)[0].size == 2048 > 256


def test_java_int_is_javas_cast():
    x = np.array([0.0, -0.0, 1.9, -1.9, 2147483520.0, 2147483648.0, -2147483648.0, -3e9, 3e38, -3e38, np.inf, -np.inf, np.nan, 1e-40],
                 np.float32)
    want = [0, 0, 1, -1, 2147483520, PS.INT_MAX, PS.INT_MIN, PS.INT_MIN, PS.INT_MAX, PS.INT_MIN, PS.INT_MAX, PS.INT_MIN, 0, 0]
    assert PS.java_int(x).tolist() == want


def test_the_denormal_row_holds_both_saturations():
    PS.check_denormal_row(PS.denormal_frame(600), 63, 100, 50)


def test_without_a_device_the_calls_fail_loudly():
    if J.have_gpu():
        return  # (with a device the calls are test_gpu_phase_scope.py's)
    with pytest.raises(J.JsdrError):
        J.Phase(2048).scope_i16(0, 2, 8192, 1, 0, 0, 512, 100, 50, 0)
