"""Host: the premises of k_fm's form for the 8-phase tuner (bpsk_fm.hip, k_fm<PH>), checked on the library's own tables.

1. Every dsFilter tap is k 2^-15 with an integer |k| < 2^14 (the kernel's static_assert says the same of its compile-time copy).
2. At 12 kHz / 96 kHz the tuner walks the table entries 32, 64, .., 224, 0, and five of their sixteen (cos, sin) factors are exactly
   1.0, -1.0 or 0.0 -- the rest are not, cos(pi/2) = 6.1e-17 among them.  These are the classes bpsk_tuner.h states; a libm that
   returned other values would make the host scheduler fall back to the generic kernel, and this test says so loudly.
3. A converted int16 sample d (a float, so 24 significant bits at most) times a tap is exact in double, so for every int16 value,
   every distinct tap and either sign, fma(d, +-t, a) is the double a + RN(RN(d * +-1.0) * t) that the generic arithmetic rounds:
   exhaustively, with the fma evaluated in exact integer arithmetic (a, d t and their sum are integers times 2^-SCALE)."""
import numpy as np
import pytest

import java_sdr_amd as J


def taps():
    return J.bpsk_table(0)


def converted_i16():
    """fm_convert_2p15 (common.h) of all 65 536 int16 values: RN_float(a + a * c), c = 0x1.0002p-15f, as one fused operation --
    a * (1 + c) has 17 + 17 significant bits and is exact in double, and float64 -> float32 rounds it once"""
    a = np.arange(-32768, 32768, dtype=np.float64)
    c = float(np.float32(float.fromhex("0x1.0002p-15")))
    exact = a + a * c
    assert np.all((exact - a) == a * c)  # (the double sum lost nothing)
    return exact.astype(np.float32).astype(np.float64)


def test_every_tap_is_a_short_multiple_of_2pm15():
    t = taps()
    assert t.shape == (27,) and np.array_equal(t, t[::-1])
    k = t * 32768.0
    assert np.array_equal(k, np.rint(k)) and np.all(np.abs(k) < 2 ** 14), k
    assert len(set(np.abs(k[:14]).tolist())) == 14  # fourteen distinct magnitudes


def test_the_eight_tuner_entries_have_the_stated_classes():
    cos, sin = J.bpsk_table(3), J.bpsk_table(4)
    assert cos.shape == sin.shape == (256,)

    def cls(v):
        return "ONE" if v == 1.0 else "MONE" if v == -1.0 else "ZERO" if v == 0.0 else "GEN"

    got = [(cls(cos[32 * p]), cls(sin[32 * p])) for p in range(8)]
    want = [("ONE", "ZERO"), ("GEN", "GEN"), ("GEN", "ONE"), ("GEN", "GEN"), ("MONE", "GEN"), ("GEN", "GEN"), ("GEN", "MONE"), ("GEN", "GEN")]
    assert got == want, got
    # the inexact neighbours of the exact ones are tiny, not zero: the kernel keeps their products
    assert 0 < abs(cos[64]) < 1e-15 and 0 < abs(sin[128]) < 1e-15 and 0 < abs(cos[192]) < 1e-15
    # and the walk is that 8-cycle: the host recurrence (bpsk_tuner.h) from tuPhase 0
    k, _ = J.tuner_walk_host(0.0, 2.0 * np.pi * 12000 / 96000, 4096)
    assert np.array_equal(np.asarray(k[:8]), [32, 64, 96, 128, 160, 192, 224, 0]) and np.array_equal(k[8:], k[:-8])


def rn_double_of_scaled_int(n, scale):
    """round-to-nearest-even double of the integer n times 2^-scale, for |n| < 2^120 or so"""
    if n == 0:
        return 0.0
    sign, m = (-1.0, -n) if n < 0 else (1.0, n)
    sh = m.bit_length() - 53
    if sh > 0:
        q, r = m >> sh, m & ((1 << sh) - 1)
        half = 1 << (sh - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
        m, scale = q, scale - sh
    return sign * float(np.ldexp(float(m), -scale))


@pytest.mark.parametrize("acc", [0.0, 1.0, -0.7071067811865476 * 3.25e4, 12345.678901234567, -2.0 ** -20, 9.87654321e8])
def test_fma_is_the_separately_rounded_pair_for_every_int16_and_tap(acc):
    d = converted_i16()
    t14 = taps()[:14]
    # d * t exactly: d = m 2^-e with |m| < 2^24, t = k 2^-15 -- the double product has at most 38 bits
    for t in np.concatenate([t14, -t14]):
        prod = d * t
        k = int(round(float(t) * 32768))
        # (every converted value is an integer times 2^-24: 0, or a float of magnitude 1 and more)
        di = (d * 2.0 ** 24).astype(np.int64)
        assert np.array_equal(di.astype(np.float64), d * 2.0 ** 24)
        assert np.array_equal(prod * 2.0 ** 39, (di * k).astype(np.float64))  # d t 2^39 = (d 2^24)(t 2^15), an integer below 2^53
        pair = acc + prod  # a + RN(d t): the generic arithmetic.  RN(d t) = d t for all 65 536 values, so it IS the fma's RN(a + d t);
        # the fma once more from exact integers, on every 97th value, the extremes and the smallest
        SCALE = 100
        a_int = int(np.ldexp(acc, SCALE)) if acc != 0.0 else 0
        assert float(np.ldexp(float(a_int), -SCALE)) == acc
        idx = list(range(0, 65536, 97)) + [0, 1, 32767, 32768, 32769, 65535]
        for i in idx:
            p_int = int(di[i]) * k << (SCALE - 39)
            assert rn_double_of_scaled_int(a_int + p_int, SCALE) == pair[i], (acc, float(t), i)
