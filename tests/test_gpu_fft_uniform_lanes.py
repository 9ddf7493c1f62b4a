"""k_fft, k_fft_pix and k_fft_streams where a frame is whole waves: the frame's slot, number and row bases are scalars, the rows are
read and written as scalar base + 32-bit lane offset, and the first maximum of a wave is two reductions in registers (maximum,
then lowest bin among the lanes that hold it).  What can go wrong is an address (a row of another frame, a bin at another place)
or the search (the right value from the wrong bin, a lane or a row of 16 lanes left out), so the maximum is PLANTED:

  tones  a single strong tone on a chosen bin.  In the 2048-point kernel bin = r * 256 + butterfly * 128 + wave * 64 + lane
         (last pass: radix 8, two butterflies a thread, 128 threads a frame), so TONE_BINS puts the maximum in turn on lanes
         0, 1, 15, 16, 31, 32, 47, 48, 63 of either wave, on either butterfly, and on r = 0 and r = 7
  ties   the impulse at sample 0 (every bin the same number: the answer is bin 0) and the combs of tests/peak_ties.py, whose
         maximum is held by every r-th bin: equal maxima inside a row of 16 lanes, in both waves, in both butterflies

Every row of every call must (a) carry, bit for bit, the (Hz, max dB) that numpy's first argmax of the row's own bins gives with
the reference's Hz rule, (b) lie within 1e-5 of the frame peak of the oracle's row (FFT_RTOL, tests/test_gpu_fft.py), and (c) for
a tone, have its maximum on the planted bin.  The CPU test checks that the oracle alone puts each planted maximum where it is
meant to be, so that no case is vacuous.

Sizes 64 (8 threads a frame: the kernels' unchanged form), 2048 and 8192 (one frame a workgroup, eight waves); int16 and float
input; the packed, the strided and the waterfall entry point; 1, 2, 3 and 5 frames a call (an odd count leaves a surplus
part-workgroup that redoes the last frame), and 5 frames under set_cu_share(1).  Five frames never make a workgroup take a second
group of frames, whatever the share -- the grid is as large as the work -- so a last test runs enough frames under the share
that every workgroup loops and prefetches, and compares them bit for bit with the rows checked before."""
import numpy as np
import pytest

import java_sdr_amd as J
import nonfinite as NF
import oracle_lib as O
import peak_ties as PT
from test_gpu_fft import FFT_RTOL, lin

RATE = 96000
SIZES = (64, 2048, 8192)
FORMS = ("i16", "f32")
FPB = {64: 32, 2048: 2, 8192: 1}  # frames a workgroup (pick_launcher, fft_psd.hip)
TONE_BINS = (0, 1, 15, 16, 31, 32, 47, 48, 63, 64, 65, 79, 80, 95, 96, 111, 112, 127, 128, 255, 256, 1023, 1024, 1792 + 255, 2047,
             2048, 4095, 4096, 4096 + 513, 8191)
COUNTS = (1, 2, 3, 5)


def tone_frame(n, b):
    t = np.arange(n)
    x = np.zeros(2 * n, np.int16)
    x[0::2] = np.round(20000 * np.cos(2 * np.pi * b * t / n)).astype(np.int16)
    x[1::2] = np.round(20000 * np.sin(2 * np.pi * b * t / n)).astype(np.int16)
    return x


_pools = {}


def pool(n, form):
    """(frames [k][2n], kinds [k], oracle rows [k][n + 2]); kind: ("tone", bin) or ("comb", r), r = 1 being the impulse.  Made once
    and read-only."""
    if (n, form) not in _pools:
        bins = sorted(set(b for b in TONE_BINS if b < n))
        combs, periods = PT.comb_frames(n, n + 7)
        raw = np.stack([tone_frame(n, b) for b in bins] + list(combs))
        kinds = [("tone", b) for b in bins] + [("comb", r) for r in periods]
        x = raw if form == "i16" else (O.convert_i16(raw.ravel()) * np.float32(0.93)).astype(np.float32).reshape(raw.shape)
        as_float = O.convert_i16(raw.ravel()).reshape(raw.shape) if form == "i16" else x
        ref = np.stack([O.fft_receive(f, RATE) for f in as_float])
        for a in (x, ref):
            a.setflags(write=False)
        _pools[(n, form)] = (x, kinds, ref)
    return _pools[(n, form)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_the_oracle_puts_each_planted_maximum_on_its_bin(n, form):
    _, kinds, ref = pool(n, form)
    assert sum(k == ("comb", 1) for k in kinds) == 2 and len(kinds) >= 15
    for (what, v), row in zip(kinds, ref):
        hz, m = PT.psd_peak_of_row(row, n, RATE)
        assert PT.u32(row[n:]).tolist() == PT.u32(np.array([hz, m], np.float32)).tolist(), (what, v)
        first = int(np.argmax(row[:n]))
        if what == "tone":
            assert first == v and PT.multiplicity(row, n) == 1, (what, v, first)
            assert row[first] - np.partition(row[:n], -2)[-2] > 40.0, (what, v)  # far above every other bin: the kernel's 1e-5 cannot move it
        else:
            assert PT.multiplicity(row, n) >= 2, (what, v)
            if v == 1:
                assert first == 0 and PT.multiplicity(row, n) == n and row[n] == 0.0, (what, v)
    if n == 2048:  # the planted maxima reach every place the search is asked about
        tones = [b for what, b in kinds if what == "tone"]
        for wave in (0, 1):
            assert {b & 63 for b in tones if b < 128 and b >> 6 == wave} >= {0, 1, 15, 16, 31, 32, 47, 48, 63}, wave
        assert {(b >> 7) & 1 for b in tones} == {0, 1} and {b >> 8 for b in tones} >= {0, 7}


# ---------------------------------------------------------------------------------------------------------------- the device
def check_row(row, n, kind, ref, where):
    row = np.asarray(row, np.float32)
    k = int(np.argmax(row[:n]))  # numpy: the first maximal element (bench.py validate_fft)
    want = np.array([NF.hz_rule(2 * k, n, RATE), row[k]], np.float32)
    assert PT.u32(row[n:n + 2]).tolist() == PT.u32(want).tolist(), (where, kind, "stored", row[n], row[n + 1], "own row gives", want, k)
    PT.assert_row_peak(row, n, RATE, (where, kind))
    a, b = lin(row[:n]), lin(ref[:n])
    assert np.abs(a - b).max() <= FFT_RTOL * b.max(), (where, kind, float(np.abs(a - b).max() / b.max()))
    if kind[0] == "tone":
        assert k == kind[1], (where, kind, k)
    elif kind[1] == 1:
        assert k == 0 and np.all(PT.u32(row[:n]) == PT.u32(row[0])), (where, kind, k)


def run_packed(f, form, d_in, nf):
    d_psd = J.DeviceBuffer(4 * nf * (f.n + 2))
    (f.batch_i16 if form == "i16" else f.batch_f32)(d_in, nf, d_psd)
    J.binding.stream_sync()
    return d_psd.to_host(np.float32).reshape(nf, f.n + 2)


def run_waterfall(f, form, d_in, nf):
    """width = n: a pixel's pooled maximum is its bin, the peak pair the row's two trailing floats"""
    n = f.n
    d_pix, d_max, d_peak = J.DeviceBuffer(4 * nf * n), J.DeviceBuffer(4 * nf * n), J.DeviceBuffer(4 * nf * 2)
    (f.waterfall_i16 if form == "i16" else f.waterfall_f32)(d_in, nf, n, d_pix, max_dev=d_max, peak_dev=d_peak)
    J.binding.stream_sync()
    assert f.waterfall_kernel() == "k_fft_pix"
    return np.concatenate([d_max.to_host(np.float32).reshape(nf, n), d_peak.to_host(np.float32).reshape(nf, 2)], axis=1)


PAD_IN, PAD_OUT = 14, 5


def run_strided(f, form, frames):
    """a stream a frame at a padded stride, rows at a padded stride: the strided instantiation (under JSDR_FFT_STREAMS_FORCE a single
    stream takes it too, which is packed by definition)"""
    n, nf = f.n, len(frames)
    stride, pstride = 2 * n + PAD_IN, n + 2 + PAD_OUT
    buf = np.full(nf * stride, 0x7FFF if form == "i16" else np.nan, frames.dtype)
    for s in range(nf):
        buf[s * stride:s * stride + 2 * n] = frames[s]
    d_in, d_out = J.DeviceBuffer.from_host(buf), J.DeviceBuffer.from_host(np.full(nf * pstride, np.float32(-7.5), np.float32))
    (f.batch_streams_i16 if form == "i16" else f.batch_streams_f32)(d_in, nf, stride, 1, d_out, pstride)
    J.binding.stream_sync()
    got = d_out.to_host(np.float32).reshape(nf, pstride)
    assert np.all(got[:, n + 2:] == np.float32(-7.5)), "a store fell between two rows"
    return got[:, :n + 2]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_planted_maxima_at_every_entry_point_and_frame_count(n, form, monkeypatch):
    x, kinds, ref = pool(n, form)
    f = J.Fft(n, RATE)
    assert f.kernel_name() == "k_fft"
    rows_seen = 0
    for nf in COUNTS + ("5 under a share",):
        if nf == "5 under a share":
            f.set_cu_share(1)
            nf = 5
        where0 = (n, form, nf)
        for first in range(0, len(kinds), nf):
            idx = [(first + i) % len(kinds) for i in range(nf)]
            frames = np.ascontiguousarray(x[idx])
            d_in = J.DeviceBuffer.from_host(frames)
            packed = run_packed(f, form, d_in, nf)
            items, wgs = f.last_launch()
            assert items == -(-nf // FPB[n]) == wgs, (items, wgs)
            with monkeypatch.context() as m:  # (read at every call: packed rows take the strided kernels as well)
                m.setenv("JSDR_FFT_STREAMS_FORCE", "1")
                strided, strided_pix = run_strided(f, form, frames), run_waterfall(f, form, d_in, nf)
            for entry, rows in (("packed", packed), ("strided", strided), ("waterfall", run_waterfall(f, form, d_in, nf)),
                                ("waterfall, strided kernel", strided_pix)):
                assert rows.shape == (nf, n + 2)
                for i, row in zip(idx, rows):
                    check_row(row, n, kinds[i], ref[i], where0 + (entry, "frame", i))
                    rows_seen += 1
                # the three entry points run one arithmetic: the same bits
                assert np.array_equal(PT.u32(rows), PT.u32(packed)), where0 + (entry, "differs from the packed call")
            d_in.free()
    assert rows_seen >= 4 * 5 * len(kinds)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_planted_maxima_where_every_workgroup_loops(n, form):
    """one workgroup a CU and more than two groups of frames for each: every workgroup fetches a frame ahead, takes a second and
    some a third group, and the odd count leaves the last workgroup a part group.  The rows are those of the packed call without
    a share, which the test above checks one by one."""
    x, kinds, ref = pool(n, form)
    f = J.Fft(n, RATE)
    free = run_packed(f, form, J.DeviceBuffer.from_host(np.ascontiguousarray(x)), len(kinds))
    for i, row in enumerate(free):
        check_row(row, n, kinds[i], ref[i], (n, form, "pool", i))
    f.set_cu_share(1)
    probe = run_packed(f, form, J.DeviceBuffer.from_host(np.ascontiguousarray(x[:1])), 1)
    assert np.array_equal(PT.u32(probe[0]), PT.u32(free[0]))
    nf = None
    for cus in (256, 304, 512):  # (the share's grid is a workgroup a CU: found from a launch, not assumed)
        cand = 2 * cus * FPB[n] + 5
        d = J.DeviceBuffer.from_host(np.ascontiguousarray(x[np.arange(cand) % len(kinds)]))
        held = run_packed(f, form, d, cand)
        items, wgs = f.last_launch()
        if 2 * wgs < items:
            nf = cand
            break
    assert nf is not None and nf % 2 == 1, (items, wgs)
    idx = np.arange(nf) % len(kinds)
    assert np.array_equal(PT.u32(held), PT.u32(free[idx])), (n, form, "packed under a share", int(np.flatnonzero((PT.u32(held) != PT.u32(free[idx])).any(axis=1))[0]))
    w = run_waterfall(f, form, d, nf)
    items, wgs = f.last_launch()
    assert 2 * wgs < items, (items, wgs)
    assert np.array_equal(PT.u32(w), PT.u32(free[idx])), (n, form, "waterfall under a share", int(np.flatnonzero((PT.u32(w) != PT.u32(free[idx])).any(axis=1))[0]))
