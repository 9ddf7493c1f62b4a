"""Engineered slicer ties for the fast BPSK variant: what tests/golden/make_fast_tie_fixtures.py, tests/test_fast_ties_oracle.py and
tests/test_gpu_fast_ties.py share.

A detector decision of FUNcubeBPSKDemod (:539-545) is the sign of di = -(lastI*fi + lastQ*fq).  With (lastI, lastQ) held -- they
are the doubles the previous detector instant left -- di is LINEAR in the int16 input samples through the tuner, the 27-tap
low-pass, HOWARD, the VCO and the 65-tap matched filter, and every factor is a finite double: the real-number value of di is a
rational number that fractions.Fraction gives exactly.  The fixture (tests/golden/fast_tie_fixtures.npz) holds small patches to
O.make_dbpsk_stream bases that bring that rational number of chosen decisions to within 1e-10 or so of zero, far below the
rounding error of any double evaluation: the sign the reference takes there is the sign of ITS OWN rounding, in ITS order of
operations -- what an implementation that promises the reference's bits has to reproduce, and what one that sums in another
order, or with fused multiply-adds, gets wrong about every other time.

Everything here is CPU only (numpy, fractions and the C oracle).
"""
import hashlib
import math
import os
from fractions import Fraction

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "fast_tie_fixtures.npz")

# The stream families: which branch of the fast tail's exact redo each reaches.  The carriers sit 300 Hz above tuning + 1200: the
# differential phase of a symbol is then near 90 degrees and di near zero against energy2 on every decision, so that patches of
# a percent of the amplitude suffice to finish the tie.  With the tuner bypassed (d: tuPhase never rises above 0, :385) both
# rails carry the same baseband cosine; the carrier is 20 Hz off so that it walks through its zero.  e: 1280 Hz at 96 kHz is a
# tuner whose table index has an exact period of 75 samples from sample 0 on (most tunings have none: 1000 Hz does not) -- the
# redo's long unwrapped (cos, sin) table and its modulo phase.
FAMILIES = {
    "a": dict(rate=96000, tuning=12000, ic=0, qc=0, carrier=13500.0, n=32768, seed=20021201, stream=1, noise_sigma=300.0, want=11),
    "b": dict(rate=48000, tuning=12000, ic=37, qc=-21, carrier=13500.0, n=20480, seed=20021202, stream=2, noise_sigma=300.0, want=11),
    "c": dict(rate=192000, tuning=12000, ic=0, qc=0, carrier=13500.0, n=40000, seed=20021203, stream=3, noise_sigma=300.0, want=11),
    "d": dict(rate=96000, tuning=0, ic=0, qc=0, carrier=1220.0, n=32768, seed=20021204, stream=4, noise_sigma=300.0, want=11),
    "e": dict(rate=96000, tuning=1280, ic=0, qc=0, carrier=2780.0, n=32768, seed=20021205, stream=5, noise_sigma=300.0, want=11),
    "f": dict(rate=96000, tuning=12010, ic=0, qc=0, carrier=13510.0, n=32768, seed=20021206, stream=6, noise_sigma=300.0, want=6),
}
AMP = 3000
REDOABLE = ("a", "b", "c", "d", "e")  # f's tuner has no period: the fast tail cannot redo, it must flag

# Grades of an engineered decision.  Both need energy2 > 1e4 (energy2 > 100 plays no part).
INSIDE_REL = 1e-10  # inside: |di| <= 1e-10 * energy2 in the oracle's double
# true tie: |exact rational di| <= TIE_ABS.  Measured basis (make_fast_tie_fixtures.py prints it): over the 61 engineered decisions
# the oracle's double di differs from the exact rational di by a median of 9.4e-10 (lower decile 2.7e-11, largest 1.1e-8; di is a
# difference of two products of 1e7, whose ulp is 1.9e-9): the evaluation's own rounding.  A real-number di nine times below that
# median leaves the sign to the rounding.  The generator reaches 3.6e-12 in the median, 4.6e-11 at worst.
TIE_ABS = 1e-10

HOWARD = 0.9 * 32768.0
TWO_PI = 2.0 * math.pi
CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK")


def base_stream(fam):
    p = FAMILIES[fam]
    raw, _, _ = O.make_dbpsk_stream(p["seed"], p["stream"], p["n"], rate=p["rate"], carrier_hz=p["carrier"], amp=AMP,
                                    noise_sigma=p["noise_sigma"])
    return raw


def sha(raw):
    return hashlib.sha256(np.ascontiguousarray(raw, np.int16).tobytes()).hexdigest()


def apply_patches(raw, sample, rail, delta):
    out = raw.copy()
    idx = 2 * np.asarray(sample, np.int64) + np.asarray(rail, np.int64)
    v = out[idx].astype(np.int64) + np.asarray(delta, np.int64)
    assert v.min() >= -32768 and v.max() <= 32767
    out[idx] = v.astype(np.int16)
    return out


def patched_stream(fam, fx=None):
    fx = np.load(FIXTURE) if fx is None else fx
    base = base_stream(fam)
    assert sha(base) == str(fx[fam + "_base_sha256"]), "the synthetic base of family %s changed" % fam
    return apply_patches(base, fx[fam + "_sample"], fx[fam + "_rail"], fx[fam + "_delta"])


def oracle_for(fam, n=None, trace=False):
    """an oracle object with frames of one sample (receive_i16 takes whole frames only): calls of any length"""
    p = FAMILIES[fam]
    n = p["n"] if n is None else n
    o = O.Bpsk(rate=p["rate"], blen=4, tuning=p["tuning"], trace=n if trace else 0)
    o.declog_enable(n)
    return o


def run_oracle(fam, raw, trace=True):
    p = FAMILIES[fam]
    o = oracle_for(fam, raw.size // 2, trace)
    o.receive_i16(raw, p["ic"], p["qc"])
    g, de = o.declog_pos()
    res = dict(o=o, g=g.copy(), di=de[:, 0].copy(), e2=de[:, 1].copy())
    if trace:
        res["trace"] = o.trace().copy()
        res["trace_ds"] = o.trace_ds().copy()
    return res


# ------------------------------------------------------------------------------ the input-independent schedules, restated
def tuner_indices(fam, n):
    """table index of RxMixTuner per input sample (:382-390), -1 where the sample bypasses the mix (tuPhase <= 0)"""
    p = FAMILIES[fam]
    inc = 2.0 * math.pi * float(p["tuning"]) / float(p["rate"])
    k = np.empty(n, np.int32)
    ph = 0.0
    for i in range(n):
        ph += inc
        if ph > TWO_PI:
            ph -= TWO_PI
        k[i] = int(ph * 256.0 / TWO_PI) % 256 if ph > 0.0 else -1
    return k


def vco_indices(nds):
    """table index of RxDemodulate's VCO per 9600 Hz sample (:511-516)"""
    inc = 2.0 * math.pi * 1200.0 / 9600.0
    k = np.empty(nds, np.int32)
    ph = 0.0
    for i in range(nds):
        ph += inc
        if ph > TWO_PI:
            ph -= TWO_PI
        k[i] = int(ph * 256.0 / TWO_PI) % 256
    return k


_tables = {}


def tables():
    if not _tables:
        s, c = O.bpsk_sincos()
        _tables.update(sin=s, cos=c, ds=O.bpsk_table(0)[:27].copy(), dm=O.bpsk_table(1)[:65].copy())
    return _tables


def convert(v, c):
    """fm_convert / jo_convert_i16: the int16 sum with the DC correction, as float / 32767f, widened"""
    s = (np.asarray(v, np.int64) + c).astype(np.int16)
    return (s.astype(np.float32) / np.float32(32767)).astype(np.float64)


class Chain:
    """the real-number chain of one family: exact rational coefficients of the input samples in (fi, fq) of a 9600 Hz sample"""

    def __init__(self, fam):
        p = FAMILIES[fam]
        self.fam, self.p = fam, p
        self.decim = p["rate"] // 9600
        self.kt = tuner_indices(fam, p["n"])
        self.kv = vco_indices(p["n"] // self.decim + 1)
        t = tables()
        F = Fraction
        self.ds = [F(float(x)) for x in t["ds"]]
        self.dm = [F(float(x)) for x in t["dm"]]
        self.cos = [F(float(x)) for x in t["cos"]]
        self.sin = [F(float(x)) for x in t["sin"]]
        self.how = F(HOWARD)

    def coeffs(self, g):
        """{n: [cI, cQ]}: fi(g) = sum cI[n] * xI[n], fq(g) = sum cQ[n] * xQ[n] over the input samples n, exactly"""
        D = self.decim
        out = {}
        for j in range(g - 64, g + 1):
            aI = self.dm[g - j] * self.cos[self.kv[j]] * self.how
            aQ = self.dm[g - j] * self.sin[self.kv[j]] * self.how
            newest = D * (j + 1) - 1
            for age in range(27):
                n = newest - age
                k = self.kt[n]
                tI = self.ds[age] if k < 0 else self.ds[age] * self.cos[k]
                tQ = self.ds[age] if k < 0 else self.ds[age] * self.sin[k]
                c = out.setdefault(n, [Fraction(0), Fraction(0)])
                c[0] += aI * tI
                c[1] += aQ * tQ
        return out

    def exact_fifq(self, raw, g, co=None):
        co = self.coeffs(g) if co is None else co
        ns = sorted(co)
        xi = convert(raw[2 * np.array(ns)], self.p["ic"])
        xq = convert(raw[2 * np.array(ns) + 1], self.p["qc"])
        fi = sum(co[n][0] * Fraction(float(a)) for n, a in zip(ns, xi))
        fq = sum(co[n][1] * Fraction(float(a)) for n, a in zip(ns, xq))
        return fi, fq

    def exact_di(self, raw, g, lastI, lastQ, co=None):
        """the real-number di of the decision at g, with dmLastIQ the doubles (lastI, lastQ)"""
        fi, fq = self.exact_fifq(raw, g, co)
        return -(Fraction(float(lastI)) * fi + Fraction(float(lastQ)) * fq)

    def free_samples(self, g, gp):
        """input samples of g's window that no window up to gp's reaches: patches there leave every earlier decision alone"""
        return range(self.decim * (gp + 1), self.decim * (g + 1))


def age_order_fifq(trace_ds, kv, g):
    """(fi, fq) of 9600 Hz sample g from the down-sampler's outputs, the matched filter summed in plain ascending-age order
    (newest first) instead of the reference's ring-slot order: same real number, another rounding"""
    t = tables()
    fi = fq = 0.0
    for age in range(65):
        j = g - age
        fi += (trace_ds[j, 0] * t["cos"][kv[j]]) * t["dm"][age]
        fq += (trace_ds[j, 1] * t["sin"][kv[j]]) * t["dm"][age]
    return fi, fq


def ring_order_fifq(trace_ds, kv, g):
    """the reference's own order (:518-523): ring slots 0 .. 64, slot of sample j = (64 - j) mod 65"""
    t = tables()
    fi = fq = 0.0
    pos = (64 - g) % 65  # dmPos when sample g is stored
    for n in range(65):
        age = (n - pos) % 65
        j = g - age
        fi += (trace_ds[j, 0] * t["cos"][kv[j]]) * t["dm"][age]
        fq += (trace_ds[j, 1] * t["sin"][kv[j]]) * t["dm"][age]
    return fi, fq


def kernel_di(prv, cur):
    """the detector's expression (:539) on two (fi, fq) pairs, as the tail kernels write it"""
    return -((prv[0] * cur[0]) + (prv[1] * cur[1]))
