"""Correctly rounded sin / cos of a double, in exact rational arithmetic (no libm).

Kept apart from java_restatement.py, which parses the reference's sources when it is imported: the tests use this
function on its own, and must run where the reference does not exist."""
from fractions import Fraction


def _round_fraction(q):
    return float(q)  # Fraction -> float is correctly rounded (round-half-even) in CPython


def _sincos_exact(x):
    """correctly rounded (sin x, cos x) of the double x, via Taylor series in exact rationals"""
    q = Fraction(x)
    s = Fraction(0)
    c = Fraction(0)
    term = Fraction(1)
    n = 0
    # |x| <= 2 pi: 80 terms leave a remainder far below 2^-200
    while n < 80:
        if n % 2 == 0:
            c += term if (n // 2) % 2 == 0 else -term
        else:
            s += term if (n // 2) % 2 == 0 else -term
        n += 1
        term = term * q / n
    return _round_fraction(s), _round_fraction(c)
