"""CPU: the round-off-level FFT cases (tests/fft_accuracy.py) hit what they claim, the yardstick they are measured with is as
good as its own table, and the reference's dB rule passes part C on its own."""
import math

import numpy as np
import pytest

import fft_accuracy as A
import oracle_lib as O


def test_sizes_and_families():
    assert len(set(A.SIZES)) == len(A.SIZES) == 28
    assert A.K_RT == (12, 60, 210, 800, 3200, 4000, 4410, 9800, 1102, 97 * 97)
    # (22 = 2.11, 143 = 11.13, 2.4099: composite, but their prime factors above 7 are not small beside n -- fft_rt.hip rt_plan)
    assert A.K_ANY == (22, 143, 2 * 4099, 37, 9601, 17640, 19997)
    # the plan shapes the sizes were chosen for
    assert A.plan(12) == (4, 3)
    assert sorted(A.plan(210)) == [2, 3, 5, 7]
    assert A.plan(3200) == (16, 8, 5, 5)
    assert A.plan(4410) == (14, 21, 15)
    assert A.plan(97 * 97) == (97, 97)      # first and last pass both generic
    assert A.plan(1102) == (2, 19, 29)      # generic passes behind a butterfly
    # 4000 is the threshold of the composite radices: one sample below, the same factors stay apart
    assert any(r in (6, 10, 14, 15, 21, 25) for r in A.plan(4000))
    assert not any(r in (6, 10, 14, 15, 21, 25) for r in A.rt_plan(3990))
    for n in A.SIZES:
        p = A.plan(n)
        assert (p == ()) == (A.kernel_for(n) == "k_dft_any"), n
        if p:
            assert math.prod(p) == n, (n, p)


@pytest.mark.parametrize("n", A.SIZES)
def test_impulse_positions_hold_every_plan_prefix(n):
    pos = A.impulse_positions(n)
    assert pos == sorted(set(pos)) and all(0 < t < n for t in pos)
    for t in (1, 2, 3, 5, 7, n - 1):
        assert t in pos
    if n % 2 == 0:
        assert n // 2 in pos
    prod = 1
    for r in A.plan(n)[:-1]:
        prod *= r
        assert prod in pos, (n, A.plan(n), prod)
    if n == 19200:  # ... and of the half plan on its own
        assert {16, 128, 640, 3200} <= set(pos)
    f = A.impulse_frames(n)
    assert f.shape == (len(pos), 2 * n) and np.count_nonzero(f) == len(pos)
    assert all(f[i, 2 * t] == 1.0 for i, t in enumerate(pos))
    # the expectation is the DFT of the frame: against the exact DFT at one position
    i = len(pos) // 2
    assert np.abs(A.impulse_want(n)[i] - A.exact_dft(f[i])).max() < 1e-12


@pytest.mark.parametrize("n", A.SIZES)
def test_int16_frames_are_on_the_grid(n):
    raw = A.square_i16(n)
    assert raw.dtype == np.int16 and set(np.unique(raw)) == {-32768, 32767}
    assert np.array_equal(raw[0:28:2], np.array([32767] * 7 + [-32768] * 7, np.int16)[:n])
    f = A.frames(n)
    assert f.dtype == np.float32 and f.shape == (5, 2 * n) and np.array_equal(f[A.SQUARE], O.convert_i16(raw))
    assert np.array_equal(f[3, 0::2], np.ones(n, np.float32)) and not f[3, 1::2].any()
    lv = A.level_frames_i16(n)
    assert lv.dtype == np.int16 and np.array_equal(lv[:, 0], np.array(A.LEVELS_I16, np.int16)) and not lv[:, 1:].any()
    # the bin-centred tone sits on its bin; the off-bin one, 46 dB below, is the largest thing left when that bin is taken out
    w = np.abs(A.want(n)[2])
    assert abs(w[n // 7] - 0.3 * n) < 0.01 * n
    w[n // 7] = 0
    k2 = int(np.argmax(w))
    assert min(abs(k2 - (n - n / 9.0 - 0.5)), abs(k2 + n - (n - n / 9.0 - 0.5))) <= 1 and -52 < 20 * math.log10(w[k2] / (0.3 * n)) < -46


@pytest.mark.parametrize("n", A.SIZES)
def test_pw_is_a_normal_float_at_every_level(n):
    """the condition of part C: the reference rule's own float product p (2/n)^2 neither underflows nor overflows"""
    tiny = np.finfo(np.float32).tiny
    for a in (A.levels_f32(n), A.levels_i16_as_float()):
        assert a.dtype == np.float32
        pw = A.level_pw(n, a)
        assert pw.dtype == np.float32 and np.all(np.isfinite(pw)) and np.all(pw >= tiny), n
        assert np.all(np.isfinite(A.level_power(a))) and np.all(A.level_power(a) >= tiny)
    a = A.levels_f32(n)
    assert a.size == 109 * ((16 if n <= 2048 else 3) + 3)
    assert a.min() == np.float32(2.0 ** -48) and a.max() == np.float32(2.0 ** 60 * (1 + (15 if n <= 2048 else 11) / 16))
    grid = {np.float32(math.ldexp(1 + m / 16.0, e)) for e in range(-48, 61) for m in (range(16) if n <= 2048 else (0, 5, 11))}
    assert grid <= set(a.tolist())
    # the grid's squares are short (nine bits); the three further levels a binade have squares that use the whole mantissa
    low_bits = A.level_power(a).view(np.uint32) & np.uint32(0x3fff)
    assert np.count_nonzero(low_bits) == 3 * 109
    # the int16 levels reach the practical floor, -96 dB - 20 log10(n/2) ... (one count: -90.3 dBFS, times 2/n)
    t = A.level_target(n, A.levels_i16_as_float())
    assert abs(t.min() - (20 * math.log10(1 / 32767.0) - 20 * math.log10(n / 2.0))) < 1e-3


@pytest.mark.parametrize("n", A.SIZES)
def test_yardstick_stays_within_its_own_table(n):
    """a torch build with a worse float32 CPU FFT is noticed here instead of silently widening the GPU tests' bars: E2 within
    3 eps on every frame, the impulses' bins within 12 eps, Emax within 12 eps on the noise frame.  Emax is the error over |x|_2,
    and a bin may hold sqrt(n) |x|_2 (a tone, the square wave's lines): the rounding of such a bin alone is up to sqrt(n) / 2
    eps in that unit (133 eps measured at n = 19997), so 12 eps is a figure of the flat spectrum; on the other frames Emax is
    held through E2, Emax <= E2 sqrt(n) by Parseval."""
    m = A.yardstick_measures(n)
    e2, emax, imp = max(e for e, _ in m) / A.EPS, max(e for _, e in m) / A.EPS, A.impulse_yardstick_error(n) / A.EPS
    print("yardstick n=%d E2=%.2f eps Emax=%.2f eps (noise %.2f) impulse=%.2f eps" % (n, e2, emax, m[A.NOISE][1] / A.EPS, imp))
    assert e2 <= 3.0, (n, e2)
    assert m[A.NOISE][1] / A.EPS <= 12.0, (n, m[A.NOISE][1] / A.EPS)
    assert emax <= 3.0 * math.sqrt(n), (n, emax)
    assert imp <= 12.0, (n, imp)
    b2, bm = A.bars(n)
    assert b2 == max(4 * e2 * A.EPS, A.EPS) and bm == max(4 * emax * A.EPS, A.EPS) and A.impulse_bar(n) == max(4 * imp * A.EPS, A.EPS)


@pytest.mark.parametrize("n", A.SIZES)
def test_reference_db_rule_passes_the_level_sweep(n):
    """jo_fft_psd_from_spectrum (fft.java:196-207) on bins (a, 0): within 1.5 ulp32(M) of T = 10 log10(p 4 / n^2) at every level"""
    worst = 0.0
    for a in (A.levels_f32(n), A.levels_i16_as_float()):
        rows = -(-a.size // n)
        bins = np.full(rows * n, a[-1], np.float32)
        bins[:a.size] = a
        got = np.concatenate([O.fft_psd_from_spectrum(A.interleave(r.astype(np.complex64)), 10 * n)[:n]
                              for r in bins.reshape(rows, n)])[:a.size].astype(np.float64)
        err = np.abs(got - A.level_target(n, a)) / A.level_bound(n, a, 1.0)
        worst = max(worst, float(err.max()))
    print("reference dB rule n=%d: %.2f ulp32(M)" % (n, worst))
    assert worst <= 1.5, (n, worst)


def test_ulp32():
    for x in (1.0, 1.5, 0.75, 96.3, 1e-30, 3e38):
        assert A.ulp32(x) == float(np.spacing(np.float32(x))), x
    assert A.ulp32(-2.0) == 2.0 ** -22
