"""Exact ties in the two "first strict maximum" searches whose result is an index: what tests/test_peak_ties_oracle.py (CPU),
tests/test_gpu_psd_peak_ties.py, tests/test_gpu_acq_ties.py and check_psd of tests/test_gpu_fft.py share.

fft.receive (fft.java:201-224) keeps the first bin of the row's maximum -- `if (m < psd[s/2])` -- and publishes it as Hz in
psd[n], with the maximum in psd[n+1].  doBufferFFT (FUNcubeBPSKDemod.java:433-443) keeps the first position of the largest
100-bin boxcar sum of a quarter band -- `if (maxBin < avePsd[i])` -- and that position becomes the centre bin.  On the device
neither is a loop: each kernel family merges (value, index) candidates across threads, lanes, waves and chunks, and a merge that
is right about the larger value but wrong about who wins among EQUALS shows only on input whose maximum is held more than once.

Where exact ties come from: a frame whose non-zero samples sit only at multiples of n / r has a spectrum of period r -- in any
FFT whose butterflies add zeros and multiply by the unit twiddle exactly, and in the DFT by definition.  r = 1 is an impulse at
sample 0: all n bins are one number.  The boxcar sums of such a frame tie in the oracle's doubles, so that every lane, wave and
chunk of a search holds a copy of the maximum.

Everything here is CPU only (numpy and the C oracle)."""
import numpy as np

import nonfinite as NF
import oracle_lib as O

FLT_MAX = NF.FLT_MAX
COMB_PERIODS = (1, 2, 4, 8, 16, 3, 5, 7)
COMB_AMPS = (20000, 3)

# The frame sizes of the PSD tests, by the kernel family that serves them, and the rates they run at (10 n where that fits an
# audio rate, the reference's frame rule; the power-of-two frames at 96 kHz).
PSD_FAMILIES = {
    "k_fft": (64, 128, 256, 512, 1024, 2048, 4096, 8192),
    "k_fft_mixed": (4800, 9600),
    "k_fft_mixed_dual": (19200,),
    # (1102 = 2.19.29: the generic prime pass; 343 = 7^3 is a run-time plan too, not the direct DFT's)
    "k_fft_rt": (4410, 800, 1102, 343),
    # (101 is prime; 106 = 2.53 and 505 = 5.101: a prime factor too large beside n for a pass of its own -- frames of the direct DFT
    #  that have combs of period 2 and 5; 16384: a power of two above k_fft's largest)
    "k_dft_any": (101, 106, 505, 16384),
}
PSD_SIZES = [(n, fam) for fam, ns in PSD_FAMILIES.items() for n in ns]


def psd_rate(n):
    return 96000 if (n & (n - 1)) == 0 else 10 * n


# The FFT-acquire census: (frame, rate).  1024 .. 8192 and 9600 at 96 kHz, the rest at 10 nsf.
ACQ_SIZES = [(800, 8000), (1024, 96000), (2048, 96000), (3200, 32000), (4096, 96000), (4410, 44100), (4800, 48000), (8192, 96000),
             (9600, 96000), (16384, 163840), (17640, 176400), (19200, 192000)]
ACQ_RATE = dict(ACQ_SIZES)
ACQ_FRAMES = 14


# ---------------------------------------------------------------------------------------------------------------- inputs
def tie_stream(nsf, nfr=ACQ_FRAMES):
    """int16 IQ, nfr frames of nsf samples: frame f is an r-comb, r cycling over 1 and the periods that divide nsf; the amplitude
    grows from frame to frame so that the centre-bin rule (:447) keeps firing"""
    rng = np.random.default_rng(nsf)
    rs = [1] + [r for r in (2, 4, 8, 16, 32, 64, 3, 5, 7, 6, 10) if nsf % r == 0]
    raw = np.zeros(2 * nsf * nfr, np.int16)
    for f in range(nfr):
        r = rs[f % len(rs)]
        amp = int(min(30000, 1500 * 1.35 ** f))
        for j in range(r):
            t = f * nsf + j * (nsf // r)
            raw[2 * t] = rng.integers(-amp, amp + 1)
            raw[2 * t + 1] = rng.integers(-amp, amp + 1)
        if r == 1:
            raw[2 * f * nsf] = amp
    return raw


def tie_stream_f32(nsf, nfr=ACQ_FRAMES):
    """the float form: the same frames off the int16 grid"""
    return (O.convert_i16(tie_stream(nsf, nfr)) * np.float32(0.93)).astype(np.float32)


def comb_periods(n):
    return [r for r in COMB_PERIODS if n % r == 0]


def comb_frames(n, seed):
    """(frames int16 [k][2n], periods [k]): for every r of COMB_PERIODS that divides n two frames with random int16 values at the
    comb positions j n / r, one of amplitude 20000 and one of amplitude 3.  The impulse (r = 1) is never silent: its I is the
    amplitude itself.  The r values are drawn again while the largest magnitude of their own r-point spectrum is not alone by 1e-3
    of itself (at amplitude 3 two of the r residues are easily equal: (1, 0) and (0, 1) at r = 2): the row's maximum is then
    held by the n / r bins of ONE residue, which is what the tests count."""
    rng = np.random.default_rng(seed)
    rows, periods = [], []
    for r in comb_periods(n):
        for amp in COMB_AMPS:
            while True:
                v = rng.integers(-amp, amp + 1, (r, 2))
                if r == 1:
                    v[0, 0] = amp
                mag = np.sort(np.abs(np.fft.fft(v[:, 0] + 1j * v[:, 1])))
                if r == 1 or mag[-1] - mag[-2] > 1e-3 * mag[-1]:
                    break
            x = np.zeros(2 * n, np.int16)
            x[0::2][::n // r][:r] = v[:, 0]
            x[1::2][::n // r][:r] = v[:, 1]
            rows.append(x)
            periods.append(r)
    return np.stack(rows), periods


def upper_tones_frame(n):
    """float IQ: three bin-centred tones in the upper half of the spectrum (negative Hz), the strongest not the first"""
    t = np.arange(n)
    ks = (n // 2 + 1, (3 * n) // 4, n - 1)
    x = sum(a * np.exp(2j * np.pi * k * t / n) for a, k in zip((0.1, 0.45, 0.2), ks))
    buf = np.empty(2 * n, np.float32)
    buf[0::2], buf[1::2] = x.real, x.imag
    return buf


def real_tone_frame(n):
    """int16 IQ with Q = 0: a bin-centred real tone, whose two mirror bins k and n - k are equal in exact arithmetic"""
    k = max(1, n // 5)
    x = np.zeros(2 * n, np.int16)
    x[0::2] = np.round(12000 * np.cos(2 * np.pi * k * np.arange(n) / n)).astype(np.int16)
    return x


# ---------------------------------------------------------------------------------------------------------------- the rule
def psd_peak_of_row(row, n, rate):
    """fft.java:201-224 on the row's own float32 bins: (Hz as float32, the maximum as float32)"""
    row = np.asarray(row[:n], np.float32)
    with np.errstate(invalid="ignore"):
        ok = row > -FLT_MAX  # false for NaN and -inf, true for +inf
    if not ok.any():
        p, m = -1, np.float32(-FLT_MAX)
    else:
        m = row[ok].max()
        p = 2 * int(np.flatnonzero(row == m)[0])
    return NF.hz_rule(p, n, rate), np.float32(m)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def multiplicity(row, n):
    """how many bins hold the row's maximum (0: no bin is above -FLT_MAX)"""
    row = np.asarray(row[:n], np.float32)
    with np.errstate(invalid="ignore"):
        ok = row > -FLT_MAX
    return int((row == row[ok].max()).sum()) if ok.any() else 0


def reported_bin(hz, n, rate):
    """the bins whose Hz value (by the reference's int rule) is the float the kernel reported, -1 for "no maximum" among them"""
    return [k for k in range(-1, n) if NF.hz_rule(2 * k if k >= 0 else -1, n, rate) == hz][:4]


def assert_row_peak(row, n, rate, where):
    """row: n bins and the two trailing floats.  Both floats must be, bit for bit, what the reference's loop gives for these bins."""
    row = np.asarray(row, np.float32)
    hz, m = psd_peak_of_row(row, n, rate)
    got = u32(row[n:n + 2])
    want = u32(np.array([hz, m], np.float32))
    if not np.array_equal(got, want):
        bins = row[:n]
        first = int(np.flatnonzero(bins == m)[0]) if multiplicity(row, n) else -1
        raise AssertionError((where, "psd[n], psd[n+1] = %r, %r; the row's own bins give %r, %r" % (row[n], row[n + 1], hz, m),
                              "the maximum is held by %d bins, the first is bin %d" % (multiplicity(row, n), first),
                              "the kernel's Hz is that of bin(s) %s" % reported_bin(row[n], n, rate)))


# ---------------------------------------------------------------------------------------------------------------- census
def acq_census(nsf, rate, do_up, form, nfr=ACQ_FRAMES):
    """the oracle over tie_stream(nsf): per frame (binPos, tied, taken), and the offsets binPos - (beg + 75) of the frames that
    are tied AND taken -- only then does binPos reach aveCentreBin (state double 7)"""
    o = O.Bpsk(rate=rate, blen=4 * nsf, do_fft=1, do_up=do_up)
    o.fft_probe_enable(nfr)
    if form == "i16":
        o.receive_i16(tie_stream(nsf, nfr))
    else:
        x = tie_stream_f32(nsf, nfr)
        for f in range(nfr):
            o.receive(x[2 * nsf * f:2 * nsf * (f + 1)])
    pr = o.fft_probe()
    assert pr.shape[0] == nfr
    beg = nsf // 4 if do_up else 0
    tied_taken = [(int(r[0]) - (beg + 75)) for r in pr if r[2] == r[1] and r[4] == 1.0]
    return dict(frames=nfr, tied_taken=len(tied_taken), offsets=sorted(set(tied_taken)), binpos=[int(r[0]) for r in pr],
                centre=[int(r[5]) for r in pr])
