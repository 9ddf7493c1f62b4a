"""GPU: the fused fft.receive + waterfall.paintLine calls (jsdr_fft_waterfall_i16 / _f32) against their definition by composition,
bit for bit: pixel rows equal jsdr_waterfall_lines of the same handle's batch PSD, the pooled maxima equal a numpy restatement of
getMax over that PSD, the peak pair equals the PSD row's two trailing floats.  Floats are compared as uint32, so NaNs compare.
Every output of every call lies in a guarded buffer (tests/layouts.py) with a lead and a tail.

Shapes: every launcher plan of k_fft_pix (n = 64 .. 8192: threads per frame, frames per workgroup and radix count all differ), the
widths at which the pooling takes another path, and frame counts either side of a workgroup's frames."""
import gc
import os

import numpy as np
import pytest

import java_sdr_amd as J
import layouts as LY
import nonfinite as NF
import oracle_lib as O

from test_gpu_layouts import Guarded

pytestmark = pytest.mark.gpu

RATE = 96000
FPB = {64: 32, 256: 16, 1024: 4, 2048: 2, 4096: 1, 8192: 1}  # frames per workgroup of k_fft / k_fft_pix (pick_launcher)
IC, QC = 1234, -4321  # with the full-scale frame: both rails wrap


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def getmax_rows(psd, n, width):
    """fft.java:147 / waterfall.java:102-109 over every row of psd [nf][n+2]: float32 [nf][width], the bits of the bin taken"""
    step = np.float32(n) / np.float32(width)
    l = int(step)
    o = (np.arange(width, dtype=np.float32) * step).astype(np.int64)  # (int) of a non-negative float below 2^31: truncation
    r = psd[:, o].copy()
    for i in range(1, l):
        v = psd[:, o + i]
        with np.errstate(invalid="ignore"):
            take = v > r  # false with a NaN on either side: a NaN is never taken and never replaced
        r = np.where(take, v, r)
    return r


def widths_of(n):
    return sorted({1, 3, 255, 256, 1000, n, n + 1} | ({1280} if n == 2048 else set()))


def frame_counts(n):
    return sorted({1, FPB[n] - 1, FPB[n] + 1, 37} - {0})


_inputs = {}


def i16_frames(n):
    """37 frames: tones, an all-zero frame, a full-scale frame, tones"""
    if n not in _inputs:
        ct, _ = O.synth_tables(6000)
        x = O.synth_tones(0, 37, n, ct, 250, O.mix64(n)).reshape(37, 2 * n).copy()
        x[1] = 0
        x[2, 0::2] = np.where(np.arange(n) % 3 == 0, -32768, 32767)
        x[2, 1::2] = np.where(np.arange(n) % 5 == 0, 32767, -32768)
        x.setflags(write=False)
        _inputs[n] = x
    return _inputs[n]


def f32_frames(n, width=255):
    """the same frames off the int16 grid; frames 3 .. 6 hold a NaN, +Inf, -Inf and 1e30 -- at the sample indices of the first, a
    middle and the last bin of a pixel's run at that width (the whole spectrum of such a frame is NaN, Inf or a mix of the two)"""
    x = (O.convert_i16(i16_frames(n).ravel()) * np.float32(0.93)).astype(np.float32).reshape(37, 2 * n)
    step = np.float32(n) / np.float32(width)
    l = max(int(step), 1)
    p = width // 3
    o = int(np.float32(p) * step)
    spots = [(o, NF.I), (o + l // 2, NF.Q), (o + l - 1, NF.I)]
    for k, v in enumerate((NF.NAN, NF.PINF, NF.NINF, np.float32(1e30))):
        x[3 + k] = NF.poison(x[3 + k], [(s, rail, v) for s, rail in spots])
    return x


class Fused:
    """one fused call into guarded outputs; .pix / .max / .peak are the rows (None where the output was not asked for)"""

    def __init__(self, f, form, d_in, nf, width, ic=0, qc=0, rgb=0x00FFFF, want_max=True, want_peak=True, stream=None):
        pix = Guarded(LY.Layout(nf, width, lead=1, tail=3, itemsize=4), "fused pixels")
        mx = Guarded(LY.Layout(nf, width, lead=3, tail=1, itemsize=4), "fused maxima") if want_max else None
        pk = Guarded(LY.Layout(nf, 2, lead=1, tail=5, itemsize=4), "fused peaks") if want_peak else None
        if form == "i16":
            f.waterfall_i16(d_in, nf, width, pix.ptr, ic, qc, rgb, mx.ptr if mx else None, pk.ptr if pk else None, stream)
        else:
            f.waterfall_f32(d_in, nf, width, pix.ptr, rgb, mx.ptr if mx else None, pk.ptr if pk else None, stream)
        if stream is not None:
            J.binding.stream_sync(stream)  # (a non-blocking stream: the copies back are not ordered behind it)
        self.pix = pix.rows(np.uint32)
        self.max = mx.rows(np.float32) if mx else None
        self.peak = pk.rows(np.float32) if pk else None


def batch_psd(f, form, d_in, nf, ic=0, qc=0):
    n = f.n
    d_psd = J.DeviceBuffer(4 * nf * (n + 2))
    if form == "i16":
        f.batch_i16(d_in, nf, d_psd, ic, qc)
    else:
        f.batch_f32(d_in, nf, d_psd)
    J.binding.stream_sync()
    return d_psd, d_psd.to_host(np.float32).reshape(nf, n + 2)


def composed_pix(d_psd, nf, n, width, rgb=0x00FFFF):
    d_pix = J.DeviceBuffer(4 * nf * width)
    J.waterfall_lines_dev(d_psd, nf, n, width, d_pix, rgb)
    J.binding.stream_sync()
    return d_pix.to_host(np.uint32).reshape(nf, width)


def check_against_composition(got, d_psd, psd, nf, n, width, where, rgb=0x00FFFF):
    assert np.array_equal(got.pix, composed_pix(d_psd, nf, n, width, rgb)), (where, "pix")
    if got.max is not None:
        assert np.array_equal(u32(got.max), u32(getmax_rows(psd, n, width))), (where, "max")
    if got.peak is not None:
        assert np.array_equal(u32(got.peak), u32(psd[:, n:n + 2])), (where, "peak")


# ------------------------------------------------------------------ composition, bit for bit
@pytest.mark.parametrize("n", sorted(FPB))
def test_fused_rows_equal_the_two_call_composition(n):
    f = J.Fft(n, RATE)
    assert f.kernel_name() == "k_fft"
    raw, flt = i16_frames(n), f32_frames(n)
    for nf in frame_counts(n):
        cases = [("i16", J.DeviceBuffer.from_host(raw[:nf]), 0, 0), ("f32", J.DeviceBuffer.from_host(flt[:nf]), 0, 0)]
        if nf == 37:
            cases.append(("i16", cases[0][1], IC, QC))
        for form, d_in, ic, qc in cases:
            d_psd, psd = batch_psd(f, form, d_in, nf, ic, qc)
            for width in widths_of(n):
                got = Fused(f, form, d_in, nf, width, ic, qc)
                assert f.waterfall_kernel() == "k_fft_pix"
                check_against_composition(got, d_psd, psd, nf, n, width, (n, nf, form, ic, width))
            if nf >= 3:
                if form == "i16" and ic == 0:
                    # the all-zero frame: every dB -inf, every pixel black, and the peak of a frame without a maximum
                    assert np.all(psd[1, :n] == -np.inf) and np.all(got.pix[1] == 0xFF000000)
                    assert got.peak[1, 0] == np.float32(int(-RATE / (2 * n))) and got.peak[1, 1] == -NF.FLT_MAX
                if form == "f32" and nf >= 7:
                    assert np.isnan(psd[3, :n]).all() and not np.isfinite(psd[4:6, :n]).any()


def test_another_peak_colour_and_nothing_but_pixels():
    n, nf, width = 2048, 5, 801
    f = J.Fft(n, RATE)
    d_in = J.DeviceBuffer.from_host(i16_frames(n)[:nf])
    d_psd, psd = batch_psd(f, "i16", d_in, nf)
    for rgb in (0xFFFFFF, 0x123456):
        got = Fused(f, "i16", d_in, nf, width, rgb=rgb, want_max=False, want_peak=False)
        check_against_composition(got, d_psd, psd, nf, n, width, hex(rgb), rgb)


# ------------------------------------------------------------------ oracle spot check
def test_a_golden_frame_through_the_oracles_paint_line(golden_dir):
    raw = np.fromfile(os.path.join(golden_dir, "sine4410.raw"), dtype="<i2")[:4096]
    f = J.Fft(2048, RATE)
    psd = f.receive_raw(raw)
    d_in = J.DeviceBuffer.from_host(raw)
    for width in (1024, 801):
        got = Fused(f, "i16", d_in, 1, width)
        assert np.array_equal(got.pix[0], O.waterfall_line(psd, 2048, width)), width
        assert np.array_equal(u32(got.peak[0]), u32(psd[2048:]))
    # the tone shows as the brightest pixel, where the two-call path shows it (test_gpu_formats.py)
    row = Fused(f, "i16", d_in, 1, 1024).pix[0]
    assert int(np.argmax(row & 0xFF)) == (int(np.argmax(psd[:2048])) // 2 + 512) % 1024


# ------------------------------------------------------------------ guarded outputs, NULL outputs
@pytest.mark.parametrize("n,width,nf", [(2048, 801, 5), (64, 101, 33), (256, 7, 17), (8192, 1918, 2), (800, 399, 3)])
def test_null_outputs_change_nothing_in_the_others(n, width, nf):
    f = J.Fft(n, RATE)
    rng = np.random.default_rng(n + width)
    raw = rng.integers(-20000, 20000, (nf, 2 * n)).astype(np.int16)
    d_in = J.DeviceBuffer.from_host(raw)
    full = Fused(f, "i16", d_in, nf, width)
    for want_max, want_peak in ((False, True), (True, False), (False, False)):
        got = Fused(f, "i16", d_in, nf, width, want_max=want_max, want_peak=want_peak)
        assert np.array_equal(got.pix, full.pix), (want_max, want_peak)
        assert got.max is None or np.array_equal(u32(got.max), u32(full.max))
        assert got.peak is None or np.array_equal(u32(got.peak), u32(full.peak))


# ------------------------------------------------------------------ persistent stride, CU share
def test_a_held_cu_share_strides_over_the_frames_and_changes_no_row():
    n, width = 64, 37
    nf = 256 * 32 * 3 + 32 * 5 + 7  # more groups of 32 frames than a workgroup per CU on any part; the last group partial
    ct, _ = O.synth_tables(6000)
    d_in, d_ct = J.DeviceBuffer(nf * n * 4), J.DeviceBuffer.from_host(ct)
    J.synth_tones(d_in, 0, nf, n, d_ct, 250, O.mix64(11))
    f = J.Fft(n, RATE)
    free = Fused(f, "i16", d_in, nf, width)
    items, wgs = f.last_launch()
    assert items == (nf + 31) // 32
    f.set_cu_share(1)
    held = Fused(f, "i16", d_in, nf, width)
    items, wgs = f.last_launch()
    assert items == (nf + 31) // 32 and wgs < items, (items, wgs)
    for a, b in ((held.pix, free.pix), (u32(held.max), u32(free.max)), (u32(held.peak), u32(free.peak))):
        assert np.array_equal(a, b)
    f.set_cu_share(0)
    d_psd, psd = batch_psd(f, "i16", d_in, nf)
    check_against_composition(held, d_psd, psd, nf, n, width, "held")


# ------------------------------------------------------------------ the composed path
def tone_frames(n, nf, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(nf * n)
    ph = 2 * np.pi * t / 7.3
    iq = np.empty((nf * n, 2))
    iq[:, 0] = 9000 * np.cos(ph) + rng.standard_normal(nf * n) * 700
    iq[:, 1] = 9000 * np.sin(ph) + rng.standard_normal(nf * n) * 700
    return np.clip(np.round(iq), -32768, 32767).astype(np.int16).reshape(nf, 2 * n)


@pytest.mark.parametrize("n,rate,nf,kernel,width", [
    (800, 48000, 1024 + 3, "k_fft_rt", 399),   # crosses a chunk of the handle's PSD rows
    (4410, 44100, 5, "k_fft_rt", 1000),
    (9600, 96000, 5, "k_fft_mixed", 1920),
    (101, 48000, 7, "k_dft_any", 64),
])
def test_other_frame_sizes_run_the_pair_through_rows_the_handle_owns(n, rate, nf, kernel, width):
    gc.collect()
    before = J.live_resources()
    f = J.Fft(n, rate)
    created = J.live_resources()
    assert f.kernel_name() == kernel
    raw = tone_frames(n, nf, n)
    raw[1] = 0
    for form, host in (("i16", raw), ("f32", (O.convert_i16(raw.ravel()) * np.float32(0.93)).astype(np.float32))):
        d_in = J.DeviceBuffer.from_host(host)
        got = Fused(f, form, d_in, nf, width)
        assert f.waterfall_kernel() == kernel + "+k_waterfall"
        d_psd, psd = batch_psd(f, form, d_in, nf)
        check_against_composition(got, d_psd, psd, nf, n, width, (n, form))
    rows = min(nf, 1024)
    assert J.live_resources()[0] == created[0] + 1 and J.live_resources()[1] == created[1] + 4 * rows * (n + 2)
    del f
    gc.collect()
    assert J.live_resources() == before


# ------------------------------------------------------------------ the handle is unchanged
def test_a_fused_call_leaves_the_handles_batch_results_as_they_were():
    for n in (2048, 800):
        f = J.Fft(n, RATE if n == 2048 else 48000)
        raw = tone_frames(n, 9, 5)
        d_in = J.DeviceBuffer.from_host(raw)
        name = f.kernel_name()
        _, before = batch_psd(f, "i16", d_in, 9)
        Fused(f, "i16", d_in, 9, 333)
        Fused(f, "f32", J.DeviceBuffer.from_host(O.convert_i16(raw.ravel())), 9, 1024)
        _, after = batch_psd(f, "i16", d_in, 9)
        assert np.array_equal(u32(before), u32(after)) and f.kernel_name() == name


# ------------------------------------------------------------------ a stream of the caller's
def test_the_call_is_ordered_on_the_callers_stream():
    n, nf, width = 1024, 9, 300
    f = J.Fft(n, RATE)
    s = J.Stream()
    d_in = J.DeviceBuffer.from_host(i16_frames(n)[:nf])
    got = Fused(f, "i16", d_in, nf, width, stream=s.ptr)
    d_psd, psd = batch_psd(f, "i16", d_in, nf)
    check_against_composition(got, d_psd, psd, nf, n, width, "stream")


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("n", [2048, 800])
def test_refusals_name_the_argument_and_a_good_call_follows(n):
    f = J.Fft(n, 48000)
    nf, width = 3, 100
    d_in = J.DeviceBuffer.from_host(tone_frames(n, nf, 1))
    d_flt = J.DeviceBuffer.from_host(O.convert_i16(tone_frames(n, nf, 1).ravel()))
    pix = Guarded(LY.Layout(nf, width, lead=1, tail=3, itemsize=4), "pixels of refused calls")
    for call, word in ((lambda: f.waterfall_i16(None, nf, width, pix.ptr), "jsdr_fft_waterfall_i16: null raw_dev"),
                       (lambda: f.waterfall_f32(None, nf, width, pix.ptr), "jsdr_fft_waterfall_f32: null iq_dev"),
                       (lambda: f.waterfall_i16(d_in, nf, width, None), "jsdr_fft_waterfall_i16: null pix_dev"),
                       (lambda: f.waterfall_f32(d_flt, nf, width, None), "jsdr_fft_waterfall_f32: null pix_dev"),
                       (lambda: f.waterfall_i16(d_in, nf, 0, pix.ptr), "width=0"),
                       (lambda: f.waterfall_f32(d_flt, nf, -5, pix.ptr), "width=-5"),
                       (lambda: f.waterfall_i16(d_in, -1, width, pix.ptr), "nframes=-1"),
                       (lambda: f.waterfall_f32(d_flt, -2, width, pix.ptr), "nframes=-2")):
        with pytest.raises(J.JsdrError, match=word):
            call()
    rc = J.lib().jsdr_fft_waterfall_i16(None, J.binding._addr(d_in), J.binding.C.c_int64(nf), 0, 0, width,
                                        J.binding.C.c_uint32(0), J.binding.C.c_void_p(pix.ptr), None, None, None)
    assert rc != 0 and "jsdr_fft_waterfall_i16: null handle" in J.lib().jsdr_last_error().decode()
    f.waterfall_i16(d_in, 0, width, pix.ptr)  # no frames: fine, and nothing is written
    assert np.array_equal(pix.dev.to_host(np.uint8), LY.guard_fill(pix.lay.nbytes))
    got = Fused(f, "i16", d_in, nf, width)
    d_psd, psd = batch_psd(f, "i16", d_in, nf)
    check_against_composition(got, d_psd, psd, nf, n, width, "after the refusals")
