"""GPU: the strided batch and waterfall calls (jsdr_fft_batch_streams_* / jsdr_fft_waterfall_streams_*) against their definition by
composition, bit for bit: what stream s receives is what the same handle's jsdr_fft_batch_* / jsdr_fft_waterfall_* writes when
it is given that stream's frames.  PSD rows are checked against the oracle as well (check_psd).  Floats are compared as uint32.

Every output lies in a buffer pre-filled with a pattern, and the WHOLE buffer is compared: the gaps between a stream's last row
and the next stream's first, and the words behind the last row, must come back untouched.  The gaps of the input hold 0x7fff
(NaN for float input), which would show in any row that had read them.

Shapes: 5 streams x 3 frames -- a workgroup's group of frames (32, 16, 4, 2 or 1 of them) straddles streams and the last group
is short -- with an input stride of 3 * 2n + 14 and a PSD stride of 3 * (n + 2) + 5, at one frame size a kernel family."""
import ctypes as C

import numpy as np
import pytest

import java_sdr_amd as J
import oracle_lib as O
from test_gpu_fft import check_psd

pytestmark = pytest.mark.gpu

RATE = 96000
IC, QC = 321, -123
PAT = np.uint32(0xDEADBEEF)
S, F = 5, 3
# n -> the kernel that serves it: every family of jsdr_fft_create
FAMILIES = {64: "k_fft", 2048: "k_fft", 8192: "k_fft", 4800: "k_fft_mixed", 19200: "k_fft_mixed_dual", 4410: "k_fft_rt",
            800: "k_fft_rt", 1009: "k_dft_any"}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def in_dtype(form):
    return np.int16 if form == "i16" else np.float32


_frames = {}


def frames_of(form, n, count):
    """count frames [count][2n]: noise with a tone, every frame another"""
    key = (form, n, count)
    if key not in _frames:
        rng = np.random.default_rng(n * 31 + count)
        t = np.arange(n)
        x = rng.integers(-3000, 3000, (count, 2 * n)).astype(np.float64)
        for k in range(count):
            w = 2 * np.pi * ((7 + 13 * k) % n) / n
            x[k, 0::2] += 9000 * np.cos(w * t)
            x[k, 1::2] += 9000 * np.sin(w * t)
        x = x.astype(np.int16)
        if form == "f32":
            x = (O.convert_i16(x.ravel()) * np.float32(0.93)).astype(np.float32).reshape(count, 2 * n)
        x.setflags(write=False)
        _frames[key] = x
    return _frames[key]


def strided_input(form, n, nstreams, fps, stride):
    """host [nstreams * stride]: stream s's frames at s * stride, the rest extreme samples"""
    fr = frames_of(form, n, nstreams * fps)
    buf = np.full(nstreams * stride, 0x7FFF if form == "i16" else np.nan, in_dtype(form))
    for s in range(nstreams):
        buf[s * stride:s * stride + fps * 2 * n] = fr[s * fps:(s + 1) * fps].ravel()
    return buf, fr


def patterned(nwords):
    return J.DeviceBuffer.from_host(np.full(nwords, PAT, np.uint32))


def per_stream_psd(f, form, d_in, nstreams, fps, stride, ic=0, qc=0):
    """[nstreams][fps][n + 2]: the handle's contiguous batch call, a stream at a time"""
    n, item = f.n, np.dtype(in_dtype(form)).itemsize
    d = J.DeviceBuffer(4 * fps * (n + 2))
    out = np.empty((nstreams, fps, n + 2), np.float32)
    for s in range(nstreams):
        if form == "i16":
            f.batch_i16(d_in.ptr + s * stride * item, fps, d, ic, qc)
        else:
            f.batch_f32(d_in.ptr + s * stride * item, fps, d)
        J.binding.stream_sync()
        out[s] = d.to_host(np.float32).reshape(fps, n + 2)
    d.free()
    return out


def strided_psd(f, form, d_in, nstreams, fps, stride, pstride, ic=0, qc=0, tail=16):
    """the strided call into a patterned buffer; returns the whole buffer as uint32"""
    n = f.n
    ps = pstride if pstride else fps * (n + 2)
    d_out = patterned((nstreams - 1) * ps + fps * (n + 2) + tail)
    if form == "i16":
        f.batch_streams_i16(d_in, nstreams, stride, fps, d_out, pstride, ic, qc)
    else:
        f.batch_streams_f32(d_in, nstreams, stride, fps, d_out, pstride)
    J.binding.stream_sync()
    got = d_out.to_host(np.uint32)
    d_out.free()
    return got


def expected_buffer(rows, pstride, tail=16):
    """the patterned buffer with rows [nstreams][fps][n + 2] at their places"""
    nstreams, fps, w = rows.shape
    ps = pstride if pstride else fps * w
    want = np.full((nstreams - 1) * ps + fps * w + tail, PAT, np.uint32)
    for s in range(nstreams):
        want[s * ps:s * ps + fps * w] = u32(rows[s]).ravel()
    return want


def assert_same_words(got, want, where):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (where, "first differing word", int(bad[0]), "of", got.size, "differing", bad.size)


# ------------------------------------------------------------------ PSD rows, every kernel family
@pytest.mark.parametrize("form", ["i16", "f32"])
@pytest.mark.parametrize("n", sorted(FAMILIES))
def test_strided_psd_equals_the_per_stream_calls_in_every_kernel_family(n, form):
    stride, pstride = F * 2 * n + 2 * 7, F * (n + 2) + 5
    ic, qc = (IC, QC) if form == "i16" else (0, 0)
    host, fr = strided_input(form, n, S, F, stride)
    f = J.Fft(n, RATE)
    assert f.kernel_name() == FAMILIES[n]
    d_in = J.DeviceBuffer.from_host(host)
    want = per_stream_psd(f, form, d_in, S, F, stride, ic, qc)
    assert np.isfinite(want[:, :, :n]).all(), "a reference row read the gap"
    for ps in (pstride, 0):  # a strided and a packed output
        got = strided_psd(f, form, d_in, S, F, stride, ps, ic, qc)
        assert_same_words(got, expected_buffer(want, ps), (n, form, ps))
    # and the rows are right: the oracle on a first, a straddling and the last frame
    for s, j in ((0, 0), (1, 0), (2, 1), (S - 1, F - 1)):
        x = fr[s * F + j]
        ref = O.fft_receive(O.convert_i16(x, ic=ic, qc=qc) if form == "i16" else x, RATE)
        check_psd(want[s, j], ref, n, RATE)
    d_in.free()


# ------------------------------------------------------------------ persistent workgroups
def test_strided_psd_with_a_cu_share_runs_persistent_workgroups():
    """n = 64 held to one workgroup a CU: 5 x 1700 frames are 266 groups of 32 for at most 256 workgroups on this chip, so every
    workgroup walks on from its first group -- across stream ends (1700 is no multiple of 32)"""
    n, fps = 64, 1700
    stride, pstride = fps * 2 * n + 2 * 7, fps * (n + 2) + 5
    for form in ("i16", "f32"):
        host, _ = strided_input(form, n, S, fps, stride)
        f = J.Fft(n, RATE)
        f.set_cu_share(1)
        d_in = J.DeviceBuffer.from_host(host)
        want = per_stream_psd(f, form, d_in, S, fps, stride)
        got = strided_psd(f, form, d_in, S, fps, stride, pstride)
        items, wgs = f.last_launch()
        assert items == (S * fps + 31) // 32 and wgs < items, (items, wgs)
        assert_same_words(got, expected_buffer(want, pstride), form)
        d_in.free()


# ------------------------------------------------------------------ the waterfall
def per_stream_waterfall(f, form, d_in, nstreams, fps, stride, width, ic=0, qc=0):
    item = np.dtype(in_dtype(form)).itemsize
    d_pix, d_max, d_peak = J.DeviceBuffer(4 * fps * width), J.DeviceBuffer(4 * fps * width), J.DeviceBuffer(4 * fps * 2)
    pix = np.empty((nstreams, fps, width), np.uint32)
    mx = np.empty((nstreams, fps, width), np.float32)
    pk = np.empty((nstreams, fps, 2), np.float32)
    for s in range(nstreams):
        src = d_in.ptr + s * stride * item
        if form == "i16":
            f.waterfall_i16(src, fps, width, d_pix, ic, qc, max_dev=d_max, peak_dev=d_peak)
        else:
            f.waterfall_f32(src, fps, width, d_pix, max_dev=d_max, peak_dev=d_peak)
        J.binding.stream_sync()
        pix[s] = d_pix.to_host(np.uint32).reshape(fps, width)
        mx[s] = d_max.to_host(np.float32).reshape(fps, width)
        pk[s] = d_peak.to_host(np.float32).reshape(fps, 2)
    for d in (d_pix, d_max, d_peak):
        d.free()
    return pix, mx, pk


def strided_waterfall(f, form, d_in, nstreams, fps, stride, width, ic=0, qc=0, aux=True, tail=16):
    """the strided call into patterned buffers; (pix, max, peak) whole, as uint32 (max and peak None when not asked for)"""
    nf = nstreams * fps
    d_pix = patterned(nf * width + tail)
    d_max = patterned(nf * width + tail) if aux else None
    d_peak = patterned(nf * 2 + tail) if aux else None
    if form == "i16":
        f.waterfall_streams_i16(d_in, nstreams, stride, fps, width, d_pix, ic, qc, max_dev=d_max, peak_dev=d_peak)
    else:
        f.waterfall_streams_f32(d_in, nstreams, stride, fps, width, d_pix, max_dev=d_max, peak_dev=d_peak)
    J.binding.stream_sync()
    out = [d.to_host(np.uint32) if d is not None else None for d in (d_pix, d_max, d_peak)]
    for d in (d_pix, d_max, d_peak):
        if d is not None:
            d.free()
    return out


def packed_with_tail(rows, tail=16):
    return np.concatenate([u32(rows).ravel(), np.full(tail, PAT, np.uint32)])


def check_waterfall(f, form, d_in, nstreams, fps, stride, width, ic, qc, where):
    pix, mx, pk = per_stream_waterfall(f, form, d_in, nstreams, fps, stride, width, ic, qc)
    for aux in (True, False):
        gp, gm, gk = strided_waterfall(f, form, d_in, nstreams, fps, stride, width, ic, qc, aux)
        assert_same_words(gp, packed_with_tail(pix), (where, "pix", aux))
        if aux:
            assert_same_words(gm, packed_with_tail(mx), (where, "max"))
            assert_same_words(gk, packed_with_tail(pk), (where, "peak"))


@pytest.mark.parametrize("form", ["i16", "f32"])
@pytest.mark.parametrize("n", [64, 2048, 8192])
def test_strided_waterfall_equals_the_per_stream_calls_in_the_fused_kernel(n, form):
    stride = F * 2 * n + 2 * 7
    ic, qc = (IC, QC) if form == "i16" else (0, 0)
    host, _ = strided_input(form, n, S, F, stride)
    f = J.Fft(n, RATE)
    d_in = J.DeviceBuffer.from_host(host)
    for width in sorted({n, n // 2, 1000 if n == 2048 else 37}):
        check_waterfall(f, form, d_in, S, F, stride, width, ic, qc, (n, form, width))
    assert f.waterfall_kernel() == "k_fft_pix"
    d_in.free()


def test_strided_waterfall_with_a_cu_share_runs_persistent_workgroups():
    n, fps, width = 64, 1700, 48
    stride = fps * 2 * n + 2 * 7
    host, _ = strided_input("i16", n, S, fps, stride)
    f = J.Fft(n, RATE)
    f.set_cu_share(1)
    d_in = J.DeviceBuffer.from_host(host)
    check_waterfall(f, "i16", d_in, S, fps, stride, width, IC, QC, "share")
    items, wgs = f.last_launch()
    assert items == (S * fps + 31) // 32 and wgs < items, (items, wgs)
    d_in.free()


@pytest.mark.parametrize("form", ["i16", "f32"])
def test_strided_waterfall_fallback_chunks_run_across_stream_ends(form):
    """3 x 400 frames of 4800: the fallback's chunks of 1024 rows end inside stream 2, and the first holds the end of streams 0
    and 1 and the start of the next"""
    n, nstreams, fps, width = 4800, 3, 400, 600
    stride = fps * 2 * n + 2 * 7
    base = frames_of(form, n, 16)
    fr = base[np.arange(nstreams * fps) * 7 % 16]  # 1200 frames out of 16, no two neighbours alike
    host = np.full(nstreams * stride, 0x7FFF if form == "i16" else np.nan, in_dtype(form))
    for s in range(nstreams):
        host[s * stride:s * stride + fps * 2 * n] = fr[s * fps:(s + 1) * fps].ravel()
    f = J.Fft(n, RATE)
    d_in = J.DeviceBuffer.from_host(host)
    ic, qc = (IC, QC) if form == "i16" else (0, 0)
    check_waterfall(f, form, d_in, nstreams, fps, stride, width, ic, qc, (n, form))
    assert f.waterfall_kernel() == "k_fft_mixed+k_waterfall"
    d_in.free()


# ------------------------------------------------------------------ packed rows are the contiguous call
@pytest.mark.parametrize("n", [2048, 4800])
def test_a_packed_strided_call_is_the_contiguous_launch(n):
    host = frames_of("i16", n, S * F).ravel()
    f = J.Fft(n, RATE)
    d_in = J.DeviceBuffer.from_host(host)
    d_a, d_b = patterned(S * F * (n + 2)), patterned(S * F * (n + 2))
    f.batch_i16(d_in, S * F, d_a, IC, QC)
    J.binding.stream_sync()
    ref_launch, ref_name = f.last_launch(), f.kernel_name()
    for pstride in (0, F * (n + 2)):
        f.batch_streams_i16(d_in, S, F * 2 * n, F, d_b, pstride, IC, QC)
        J.binding.stream_sync()
        assert (f.last_launch(), f.kernel_name()) == (ref_launch, ref_name)
        assert np.array_equal(d_a.to_host(np.uint32), d_b.to_host(np.uint32))
    if n == 2048:
        width = 1000
        p_a, p_b = patterned(S * F * width), patterned(S * F * width)
        f.waterfall_i16(d_in, S * F, width, p_a, IC, QC)
        J.binding.stream_sync()
        ref_launch, ref_name = f.last_launch(), f.waterfall_kernel()
        f.waterfall_streams_i16(d_in, S, F * 2 * n, F, width, p_b, IC, QC)
        J.binding.stream_sync()
        assert (f.last_launch(), f.waterfall_kernel()) == (ref_launch, ref_name)
        assert np.array_equal(p_a.to_host(np.uint32), p_b.to_host(np.uint32))
    d_in.free()


def test_trivial_calls_succeed():
    n = 2048
    host = frames_of("i16", n, S * F).ravel()
    f = J.Fft(n, RATE)
    d_in = J.DeviceBuffer.from_host(host)
    d_out = patterned(F * (n + 2) + 16)
    f.batch_streams_i16(d_in, 4, 2 * F * 2 * n, 0, d_out)  # no frames: nothing launched, nothing written
    f.waterfall_streams_i16(d_in, 4, 2 * F * 2 * n, 0, 100, d_out)
    J.binding.stream_sync()
    assert (d_out.to_host(np.uint32) == PAT).all()
    want = per_stream_psd(f, "i16", d_in, 1, F, 0)
    f.batch_streams_i16(d_in, 1, 7, F, d_out)  # one stream: its stride says nothing
    J.binding.stream_sync()
    assert_same_words(d_out.to_host(np.uint32), expected_buffer(want, 0), "one stream")
    d_in.free()


# ------------------------------------------------------------------ past 32-bit offsets
def test_strided_offsets_past_2_to_31_elements():
    """2 streams x 3 frames at n = 2048 with stream_stride_i16 = 2^31 + 3 * 4096: one input allocation above 4 GiB of which six
    frames are touched; and a PSD stride of 2^31 + 5 floats, which puts stream 1's rows past 2^31 floats (an allocation above
    8 GiB, zeroed; the rows and the words around them are read back)."""
    n, nstreams, fps = 2048, 2, 3
    stride, pstride = 2 ** 31 + 2 * n * fps, 2 ** 31 + 5
    fr = frames_of("i16", n, nstreams * fps)
    f = J.Fft(n, RATE)
    d_in = J.DeviceBuffer(2 * (stride + fps * 2 * n))
    assert d_in.nbytes > 2 ** 32
    d_out = J.DeviceBuffer(4 * (pstride + fps * (n + 2) + 64))
    try:
        d_out.zero()
        for s in range(nstreams):
            rows = np.ascontiguousarray(fr[s * fps:(s + 1) * fps])
            J.binding._check(J.lib().jsdr_memcpy_h2d(J.binding._addr(d_in.ptr + 2 * s * stride), J.binding._addr(rows),
                                                     C.c_size_t(rows.nbytes)), "h2d")
        want = per_stream_psd(f, "i16", d_in, nstreams, fps, stride, IC, QC)
        assert not np.array_equal(want[0], want[1])
        f.batch_streams_i16(d_in, nstreams, stride, fps, d_out, pstride, IC, QC)
        J.binding.stream_sync()
        w = fps * (n + 2)
        for s in range(nstreams):
            got = d_out.to_host(np.uint32, w + 64, 4 * s * pstride)
            assert np.array_equal(got[:w], u32(want[s]).ravel()), ("stream", s)
            assert not got[w:].any(), ("words behind stream", s)
        assert not d_out.to_host(np.uint32, 64, 4 * (pstride - 64)).any(), "words in front of stream 1"
        # the fused waterfall reads through the same offsets
        width = 1000
        d_pix = patterned(nstreams * fps * width + 16)
        pix, _, _ = per_stream_waterfall(f, "i16", d_in, nstreams, fps, stride, width, IC, QC)
        f.waterfall_streams_i16(d_in, nstreams, stride, fps, width, d_pix, IC, QC)
        J.binding.stream_sync()
        assert_same_words(d_pix.to_host(np.uint32), packed_with_tail(pix), "pix")
        d_pix.free()
    finally:
        d_in.free()
        d_out.free()
