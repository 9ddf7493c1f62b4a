"""CPU: the expectations of the tie tests, pinned on the oracle (tests/peak_ties.py has the constructions and the reasons).

1. peak_ties.psd_peak_of_row -- the numpy restatement of fft.java:201-224 that the GPU tests apply to the kernels' own rows --
   equals the oracle's C loop bit for bit, on rows whose maximum is held many times over, on rows without a maximum, on maxima in
   the upper half (negative Hz) and where p * rate wraps.
2. The maximum of an r-comb's row is held by n / r bins: the comb frames ARE ties.
3. The census of peak_ties.tie_stream in FFT-acquire: in every size, band and input form at least 10 of the 14 frames are tied
   AND taken (the runner-up of the boxcar search equals maxBin and the centre-bin rule fired, so that binPos reaches
   aveCentreBin), the first position of the searched range (offset 0) wins at least once, and at least 4 other offsets occur.
   Conditions, not tolerances: a size that misses one needs a longer stream, not a lower number."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
import peak_ties as PT

_rows = {}


def oracle_rows(n):
    """the oracle's psd rows of comb_frames(n, n) and of the extra frames, computed once (the oracle's transform of a frame that is
    no power of two is the O(n^2) long double DFT: the frames of a size go through a few threads, the C call holds no lock)"""
    if n not in _rows:
        rate = PT.psd_rate(n)
        combs, periods = PT.comb_frames(n, n)
        bufs = [O.convert_i16(x) for x in combs] + [np.zeros(2 * n, np.float32), PT.upper_tones_frame(n), O.convert_i16(PT.real_tone_frame(n))]
        with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as ex:
            rows = list(ex.map(lambda b: O.fft_receive(b, rate), bufs))
        _rows[n] = (rows, periods + ["zero", "upper tones", "real tone"])
    return _rows[n]


@pytest.mark.parametrize("n,family", PT.PSD_SIZES)
def test_the_restated_peak_rule_equals_the_oracles_loop(n, family):
    rate = PT.psd_rate(n)
    rows, kinds = oracle_rows(n)
    for row, kind in zip(rows, kinds):
        hz, m = PT.psd_peak_of_row(row, n, rate)
        assert PT.u32(hz) == PT.u32(row[n]) and PT.u32(m) == PT.u32(row[n + 1]), (n, kind, hz, m, row[n], row[n + 1])
        PT.assert_row_peak(row, n, rate, (n, kind))
    zero, upper = rows[kinds.index("zero")], rows[kinds.index("upper tones")]
    assert np.all(np.isneginf(zero[:n])) and zero[n + 1] == -PT.FLT_MAX and zero[n] == np.float32(int(-rate / (2 * n)))
    assert int(np.argmax(upper[:n])) == (3 * n) // 4 and upper[n] < 0  # a maximum in the upper half: negative Hz


def test_the_restated_peak_rule_where_the_product_wraps():
    """n = 8192 at 384 kHz: p * rate leaves int32 from bin 2797 on, on both sides of the spectrum"""
    n, rate = 8192, 384000
    t = np.arange(n)
    frames = [PT.upper_tones_frame(n)]
    for k in (3000, 3500, 4095, 4096, 4500, 6000):  # (6000: negative Hz without a wrap)
        x = 0.5 * np.exp(2j * np.pi * k * t / n)
        buf = np.empty(2 * n, np.float32)
        buf[0::2], buf[1::2] = x.real, x.imag
        frames.append(buf)
    combs, _ = PT.comb_frames(n, n)
    frames += [O.convert_i16(x) for x in combs]
    wrapped = 0
    for i, buf in enumerate(frames):
        row = O.fft_receive(buf, rate)
        PT.assert_row_peak(row, n, rate, (n, rate, i))
        k = int(np.argmax(row[:n]))
        p = 2 * k - (2 * n if k >= n // 2 else 0)
        wrapped += abs(p * rate) >= 1 << 31
    assert wrapped >= 4


@pytest.mark.parametrize("n,family", PT.PSD_SIZES)
def test_a_comb_rows_maximum_is_held_by_n_over_r_bins(n, family):
    rows, kinds = oracle_rows(n)
    seen = []
    for row, r in zip(rows, kinds):
        if isinstance(r, int):
            seen.append((r, PT.multiplicity(row, n)))
            assert PT.multiplicity(row, n) == n // r, (n, r, PT.multiplicity(row, n))
            if r == 1:
                assert np.all(PT.u32(row[:n]) == PT.u32(row[0])) and row[n] == 0.0 and row[n + 1] == row[0], (n, "impulse")
    print("n = %d (%s): (r, bins that hold the maximum) %s" % (n, family, seen))


@pytest.mark.parametrize("nsf,rate", PT.ACQ_SIZES)
def test_the_tie_stream_ties_in_fft_acquire(nsf, rate):
    for do_up in (0, 1):
        for form in ("i16", "f32"):
            c = PT.acq_census(nsf, rate, do_up, form)
            print("nsf = %d, rate %d, do_up %d, %s: %d of %d frames tied and taken, offsets %s" %
                  (nsf, rate, do_up, form, c["tied_taken"], c["frames"], c["offsets"]))
            assert c["frames"] == PT.ACQ_FRAMES
            assert c["tied_taken"] >= 10, (nsf, do_up, form, c)
            assert 0 in c["offsets"], (nsf, do_up, form, c)
            assert len([v for v in c["offsets"] if v != 0]) >= 4, (nsf, do_up, form, c)
