"""The BPSK scope's spectra (jsdr_bpsk_scope_spectra_i16 / _f32): what the tests share.

Two statements of the second half of FUNcubeBPSKDemod.paintComponent (FUNcubeBPSKDemod.java:270-327) over a ring image:

  spectra_of   the CONTRACT of include/jsdr_hip.h: jo_fft_f64 of the row (the C oracle), math.sqrt of Python floats, the strict
               first maximum, the columns in Python doubles, Java's cast through bpsk_scope.jint;
  literal_of   the Java text again, loop for loop: the in-place transform of the ring, the psd loop with its running maximum
               (:276-282), pi, ys, ly and the column loop with getMax as written (:293-300, :348-355).

tests/test_bpsk_scope_spectra_oracle.py holds the two to each other on every case and width and counts what the cases contain;
tests/test_gpu_bpsk_scope_spectra.py holds the library to them.  Everything is bit for bit (bpsk_scope.same).
"""
import ctypes as C
import json
import math
import os

import numpy as np

import bpsk_scope as B
import oracle_lib as O

F64, F32 = np.float64, np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS = os.path.join(HERE, "golden", "bpsk_scope_spectra_census.json")
NEW = ("tspec", "tpeak", "tpsd", "dspec", "dpeak", "dpsd")


# ---------------------------------------------------------------------------------------------------------------- the contract
def layout(length, Wp):
    """(first, count) of every column: i = (int)(pi m), l = (int)pi in Python doubles, (0, 0) at m = 0"""
    pi = float(length // 2) / float(Wp)
    first = np.array([0] + [int(pi * float(m)) for m in range(1, Wp)], np.int32)
    count = np.array([0] + [int(pi)] * (Wp - 1), np.int32)
    return first, count


def spectra_of(row, plot_width):
    """row [len][2] doubles -> dict(spec int32 [Wp], peak f64 [2] = (max, mo), psd f64 [len])"""
    row = np.ascontiguousarray(row, F64)
    n = row.shape[0]
    Y = O.fft_f64(row.reshape(-1)).tolist()
    psd = [math.sqrt(Y[2 * k] * Y[2 * k] + Y[2 * k + 1] * Y[2 * k + 1]) for k in range(n)]
    mx, mo = 0.0, 0
    for k in range(n):
        if mx < psd[k]:
            mx, mo = psd[k], k
    first, count = layout(n, plot_width)
    pooled = [psd[0]]
    for m in range(1, plot_width):
        i, l = int(first[m]), int(count[m])
        d = psd[i]
        for j in range(i + 1, i + l):
            if d < psd[j]:
                d = psd[j]
        pooled.append(d)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ys = F64(100.0) / F64(mx)
        spec = B.jint(np.array(pooled, F64) * ys)
    return dict(spec=spec, peak=np.array([mx, float(mo)], F64), psd=np.array(psd, F64))


# ---------------------------------------------------------------------------------------------------------------- the Java text
def _jcast(x):
    """(int) of a double"""
    if x != x:
        return 0
    return max(B.INT_MIN, min(B.INT_MAX, int(x))) if abs(x) != math.inf else (B.INT_MAX if x > 0 else B.INT_MIN)


def _getMax(d, o, l):  # :348-355
    m = d[o]
    for i in range(o + 1, o + l):
        if m < d[i]:
            m = d[i]
    return m


def literal_of(ring, width_minus_xo):
    """:270-282 / :293-300 (the same text again at :304-326) over a ring of interleaved doubles; getWidth() - xo is given"""
    tuned = np.array(ring, F64).reshape(-1)          # (the painter's ring, transformed in place)
    O.lib().jo_fft_f64(O.ptr(tuned), tuned.size // 2, 0, 0)  # DoubleFFT_1D(tuned.length/2).complexForward(tuned)
    tuned = tuned.tolist()
    psd = [0.0] * (len(tuned) // 2)
    mx = 0.0
    mo = 0
    for n in range(0, len(tuned), 2):
        psd[n // 2] = math.sqrt(tuned[n] * tuned[n] + tuned[n + 1] * tuned[n + 1])
        if mx < psd[n // 2]:
            mx = psd[n // 2]
            mo = n // 2
    pi = float(len(psd) // 2) / float(width_minus_xo)
    with np.errstate(divide="ignore"):
        ys = float(F64(100.0) / F64(mx))
    ly = _jcast(psd[0] * ys)
    y_of = [ly]
    for n in range(1, width_minus_xo):
        i = int(pi * float(n))
        y = _jcast(_getMax(psd, i, int(pi)) * ys)
        y_of.append(y)  # drawLine(xo+n-1, getHeight()-1-ly, xo+n, getHeight()-1-y)
        ly = y
    return dict(spec=np.array(y_of, np.int32), peak=np.array([mx, float(mo)], F64), psd=np.array(psd, F64))


def spectra_equal(a, b):
    return np.array_equal(a["spec"], b["spec"]) and B.same(a["peak"], b["peak"]) and B.same(a["psd"], b["psd"])


# ---------------------------------------------------------------------------------------------------------------- the cases
# bpsk_scope.CASES by reference, and the new ones.  Every (rate, n) below is one a tune-mode handle accepts.
CASES = {k: B.CASES[k] for k in ("96k", "48k", "44k1", "silence", "untuned", "nan")}
CASES.update({
    # the carrier below the tuning, 10800 - 12000 = -1200 Hz.  The reference's mixer is (i cosTab, q sinTab) (:389-390), not a complex
    # rotation: a tone at f leaves it as real cosines at f - t and f + t, so the bins at +-1200 Hz carry equal power and rounding
    # picks the half mo falls in (the census records it).  neg_raw is the case in which the peak is surely never on the polyline:
    # no tuner at all (:395) and the carrier itself at -1200 Hz, so mo >= n / 2 in every frame.
    "neg":       dict(rate=96000, n=2048, tuning=12000, carrier=10800.0, frames=2, kind="signal"),
    "neg_raw":   dict(rate=96000, n=2048, tuning=0, carrier=-1200.0, frames=2, kind="signal"),
    # frame 0 is one sample (x, 0) at slot 0: every bin of the green spectrum is x exactly, mo must be 0
    "impulse":   dict(rate=96000, n=2048, tuning=0, carrier=0.0, frames=2, kind="impulse"),
    "r192k":     dict(rate=192000, n=2048, tuning=12000, carrier=13200.0, frames=2, kind="signal"),   # L = 102 = 2 3 17
    "r48k_2048": dict(rate=48000, n=2048, tuning=12000, carrier=13200.0, frames=2, kind="signal"),    # L = 409, a prime
    "p1024":     dict(rate=96000, n=1024, tuning=12000, carrier=13200.0, frames=2, kind="signal"),    # L = 102
    "p8192":     dict(rate=96000, n=8192, tuning=12000, carrier=13200.0, frames=2, kind="signal"),    # L = 819 = 3 3 7 13
})
IMPULSE_X = 0.5
# plot widths: at n = 2048 / L = 204 the reference's 1024-pixel window (749: pi = 1.367, l = 1; L: l = 0), pi = 1 exactly, l = 10,
# one column, pi = 0.5 (l = 0), and 17 (L: pi = 6); at n = 4800 the reference's window (l = 3)
WIDTHS = {"96k": (749, 1024, 100, 1, 2048, 17)}


def widths(case):
    return WIDTHS.get(case, (749,))


def frames_of(case):
    """frames looked at: the first few of the shared cases are enough here"""
    return min(CASES[case]["frames"], 4)


def case_input(case, stream=0):
    """as bpsk_scope.case_input: ("i16", int16 [2 total]) or ("f32", float32 [2 total])"""
    c = CASES[case]
    if case in B.CASES:
        form, data = B.case_input(case, stream)
        return form, data[:2 * frames_of(case) * c["n"]]
    total = c["frames"] * c["n"]
    if c["kind"] == "impulse":
        x = np.zeros(2 * total, F32)
        x[0] = IMPULSE_X
        x[2 * c["n"] + 2 * (7 + stream)] = 0.25  # (frame 1: another impulse, off slot 0)
        return "f32", x
    return "i16", O.make_dbpsk_stream(11, stream, total, rate=c["rate"], carrier_hz=c["carrier"])[0]


def run_case(case, stream=0):
    """the case through bpsk_scope's restatement: name -> rows [frames][...] of the six scope outputs"""
    c = CASES[case]
    form, data = case_input(case, stream)
    x = B.as_float(form, data)
    n, nf = c["n"], frames_of(case)
    r = B.Restated(c["rate"], n, c["tuning"], nf)
    t = B.Tuner(c["tuning"], c["rate"])
    for f in range(nf):
        r.receive(x[2 * f * n:2 * (f + 1) * n], t.step(n))
    return r.rows(0, nf)


def radices(n):
    """the oracle's radix list of a row of n points ([] for a power of two: the radix-2 network)"""
    if n & (n - 1) == 0:
        return []
    L = O.lib()
    L.jo_fft_mixed_radices.argtypes = [C.c_int, C.c_void_p]
    rad = np.zeros(32, np.int32)
    k = L.jo_fft_mixed_radices(n, rad.ctypes.data)
    return [int(v) for v in rad[:k]]


def census_of(case):
    """what the case contains, from the oracle alone (stream 0)"""
    c = CASES[case]
    rows = run_case(case)
    n, L = c["n"], B.ring_len(c["rate"], c["n"])
    out = dict(n=n, L=L, radices_n=radices(n), radices_L=radices(L), widths=list(widths(case)))
    ls = set()
    for key, name, length in (("t", "tuned", n), ("d", "ds", L)):
        zero = nan = upper = ties = y100 = 0
        for f in range(rows[name].shape[0]):
            for Wp in widths(case):
                s = spectra_of(rows[name][f], Wp)
                ls.add(int(layout(length, Wp)[1][-1]) if Wp > 1 else 0)
                y100 += int((s["spec"] == 100).sum())
            mx, mo = s["peak"]
            zero += int(mx == 0.0)
            nan += int(np.isnan(s["psd"]).any())
            upper += int(mo >= length // 2)
            ties += int((s["psd"] == mx).sum() > 1)
        out[key] = dict(frames_with_max_zero=zero, frames_with_nan=nan, frames_with_mo_in_upper_half=upper,
                        frames_with_tied_max=ties, columns_at_100=y100)
    out["l_values"] = sorted(ls)
    return out


def census():
    return {case: census_of(case) for case in CASES}


def load_census():
    with open(CENSUS) as f:
        return json.load(f)
