"""CPU: the one-instruction int16 conversion of k_fm and k_fft (common.h: i16_to_float_java_2p15, fm_convert_2p15).

The reference rule is q = (float)s / 32767f (JavaAudio.java:281-288).  The kernels form RN(a + a*c) with c = 0x1.0002p-15f in
one fused multiply-add and claim that it is EXACTLY 2^15 * q for every int16 a.  Proved here over all 65 536 inputs in exact
rational arithmetic: RN24 is round-to-nearest-even to a 24-bit significand (no input comes near the subnormal or the overflow
range, so the exponent range does not enter)."""
from fractions import Fraction as F

import numpy as np

C = F(float.fromhex("0x1.0002p-15"))
ULP_C = F(2) ** -38  # c lies in [2^-15, 2^-14): one unit in its last place
ALL = range(-32768, 32768)


def rn24(x):
    """x (a Fraction) rounded to the nearest value with a 24-bit significand, ties to even -> (m, e): the value is m * 2^e with
    2^23 <= |m| < 2^24, or (0, 0).  Integer arithmetic throughout: nothing here is itself rounded."""
    if x == 0:
        return (0, 0)
    s = 1 if x > 0 else -1
    p, q = abs(x.numerator), x.denominator
    e = p.bit_length() - q.bit_length() - 23  # 2^e: the last place, give or take one
    while True:
        n, d = (p, q << e) if e >= 0 else (p << -e, q)
        fl, rem = divmod(n, d)
        if fl >= 2 ** 24:
            e += 1
        elif fl < 2 ** 23:
            e -= 1
        else:
            break
    if 2 * rem > d or (2 * rem == d and fl % 2):
        fl += 1
    if fl == 2 ** 24:  # rounded up to the next binade
        fl, e = 2 ** 23, e + 1
    return (s * fl, e)


def value(f):
    return F(f[0]) * F(2) ** f[1]


def times_2p15(f):
    return (f[0], f[1] + 15) if f[0] else f


QUOT = [rn24(F(a, 32767)) for a in ALL]  # the reference rule's quotients, computed once


def mismatches(c):
    return [a for a, q in zip(ALL, QUOT) if rn24(a + a * c) != times_2p15(q)]


def test_rn24_itself():
    assert rn24(F(1)) == (2 ** 23, -23) and rn24(F(-3, 4)) == (-3 * 2 ** 22, -24)
    assert rn24(F(2 ** 24 + 1)) == (2 ** 23, 1)          # tie: to even (down)
    assert rn24(F(2 ** 24 + 3)) == (2 ** 23 + 2, 1)      # tie: to even (up)
    assert rn24(F(2 ** 25 - 1)) == (2 ** 23, 2)          # up into the next binade
    assert value(rn24(F(1, 3))) == F(float(np.float32(1.0) / np.float32(3.0)))


def test_the_constant_is_the_rounded_reciprocal():
    assert C == value(rn24(F(1, 32767)))
    assert np.float32(float(C)) == np.float32(1.0) / np.float32(32767.0)


def test_rn24_of_the_quotient_is_the_reference_rule():
    """RN24(a / 32767) is numpy's float32(a) / float32(32767): the rule tested below is the one the reference applies"""
    a = np.arange(-32768, 32768, dtype=np.int32)
    want = a.astype(np.float32) / np.float32(32767.0)
    assert want.dtype == np.float32
    got = np.array([float(value(q)) for q in QUOT], np.float64)  # (24 bits: exact in a double)
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)  # ... and every one is a float32
    assert got.astype(np.float32).tobytes() == want.tobytes()


def test_one_fma_gives_the_quotient_times_two_to_the_fifteen_for_every_int16():
    assert mismatches(C) == []


def test_the_two_instruction_form_passes_the_same_check():
    """q = fma(a, rh, a * rl) with rh = 0x1.0002p-15f, rl = 0x1.0002p-45f (i16_to_float_java): every other caller's form"""
    rl = F(float.fromhex("0x1.0002p-45"))
    assert [a for a, q in zip(ALL, QUOT) if rn24(a * C + value(rn24(a * rl))) != q] == []


def test_how_much_room_the_constant_has():
    """one unit in the last place lower still holds; one higher fails for four inputs: the constant must be this one or the
    one below it, and the kernels use the rounded reciprocal itself"""
    assert mismatches(C - ULP_C) == []
    assert len(mismatches(C + ULP_C)) == 4
