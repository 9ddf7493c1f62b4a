"""Non-finite and huge float input: the comparison rule, the poisons and the shared inputs of test_nonfinite_oracle.py (CPU:
the expectations, pinned on the oracle and the Python restatement) and the GPU tests that feed the same floats to the kernels.

Every float entry point takes its samples as the reference takes buf[], and the reference takes ANY float.  Java defines what
follows: a comparison with a NaN is false, (int)NaN == 0, an IIR carries a NaN for ever.  Java cannot tell one NaN from another,
and x86 and gfx950 produce different default NaNs for an invalid operation, so doubles and floats are compared by same_f64 /
same_f32 -- identical bit patterns, or both NaN -- where a tobytes() comparison would fail for no reason.  That rule covers the
(fi, fq) trace, the 18 state doubles and frame statistics; bits, counters, FEC rc / bit index / bytes and decoded[] stay exact.

Plain module (no device, no fixtures): imported by CPU and GPU tests alike."""
import numpy as np

import oracle_lib as O

CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK", "centreBin")

NAN = np.float32(np.nan)
PINF = np.float32(np.inf)
NINF = np.float32(-np.inf)
HUGE = np.float32(3e38)
NZERO = np.float32(-0.0)
SUBN = np.float32(1e-41)
I, Q = 0, 1  # rails

SEED, STREAM, NSAMP = 20020109, 3, 2048 * 260  # the stream the named positions belong to (noise_sigma 900, 96 kHz, tuning 12 kHz)

NAN_HI = 6149
"""A NaN on I of sample 6149 of the float form of make_dbpsk_stream(20020109, 3, 2048 * 260, noise_sigma=900.0), tune mode at
12 kHz / 96 kHz.  The oracle alone: all eight dmEnergy slots and dmEnergyOut are NaN from output ~680 to the end; dmPeakPos =
dmNewPeak freeze at 4 (the clean stream ends at 4 as well); the slicer goes on at the frozen peak -- cntBit ends a few bits short
of the clean stream's -- and one FEC frame is decoded after the NaN with rc >= 0."""

INF_MID = 204877
"""A +Inf on I of sample 204 877 of the same stream.  The oracle alone: the 27-tap and 65-tap windows turn the one Inf into
+Inf, -Inf and NaN outputs; the energies end as one +Inf slot among NaN slots ([nan nan nan nan inf nan nan nan]); the peak search
passes over the NaN slots and takes the +Inf one, dmNewPeak = 4 (a search that starts from a NaN slot 0 answers 0)."""


def _same(a, b, ut):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return (a.view(ut) == b.view(ut)) | (np.isnan(a) & np.isnan(b))


def same_f64(a, b):
    """per element: the same bit pattern, or both NaN whatever their sign and payload"""
    return _same(np.asarray(a, np.float64), np.asarray(b, np.float64), np.uint64)


def same_f32(a, b):
    return _same(np.asarray(a, np.float32), np.asarray(b, np.float32), np.uint32)


def assert_same(a, b, where):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (where, a.shape, b.shape)
    ok = same_f64(a, b) if a.dtype == np.float64 else same_f32(a, b)
    if not ok.all():
        i = int(np.flatnonzero(~ok.ravel())[0])
        raise AssertionError((where, "first of %d differences at flat index %d" % (int((~ok).sum()), i), a.ravel()[i], b.ravel()[i]))


def poison(x, spec):
    """a copy of the interleaved float IQ array x with value written at (sample, rail) for every (sample, rail, value) of spec"""
    x = np.array(x, np.float32, copy=True)
    for sample, rail, value in spec:
        x[2 * sample + rail] = np.float32(value)
    return x


def offgrid(raw, k=0.93):
    """floats off the int16 grid, as the float tests of test_gpu_bpsk.py make them"""
    return (O.convert_i16(raw) * np.float32(k)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- results
class Acc:
    """what S streams of a handle produced, accumulated over its calls (arrays, not bytes: they are compared by same_f64)"""

    def __init__(self, S, get=None):
        self.S = S
        self.bits = [[] for _ in range(S)]
        self.trace = [[] for _ in range(S)]
        self.fec = [[] for _ in range(S)]
        self.nbits = [0] * S
        self.get = get or (lambda s: (s,))

    def take(self, d, only=None):
        for s in (range(self.S) if only is None else only):
            a = self.get(s)
            b = d.bits(*a).copy()
            self.bits[s].append(b)
            self.trace[s].append(d.trace(*a).copy())
            # (the library counts the trigger bit within the call, the oracle within the stream)
            self.fec[s].extend((rc, self.nbits[s] + bi, data.copy()) for rc, bi, data in d.fec_results(*a))
            self.nbits[s] += b.size

    def of(self, d, s):
        a = self.get(s)
        c = d.counters(*a)
        return dict(trace=np.concatenate(self.trace[s]).reshape(-1, 2), bits=np.concatenate(self.bits[s]), counters=[c[k] for k in CKEYS],
                    state=d.state(*a).copy(), fec=[(rc, int(bi), data.tobytes()) for rc, bi, data in self.fec[s]], decoded=d.decoded(*a).tobytes())


def of_oracle(o):
    c = o.counters()
    return dict(trace=o.trace().reshape(-1, 2), bits=o.bits().copy(), counters=[c[k] for k in CKEYS], state=o.state(),
                fec=[(rc, int(bi), data.tobytes()) for rc, bi, data in o.fec_results()], decoded=o.decoded().tobytes())


def assert_results(got, want, where, fft=True):
    """every part of two results (Acc.of / of_oracle); fft=False leaves out what only FFT-acquire keeps alive: centreBin and the
    state doubles 6, 7 (avePeakPower, aveCentreBin)"""
    assert got["bits"].tobytes() == want["bits"].tobytes(), (where, "bits", got["bits"].size, want["bits"].size)
    assert_same(got["trace"], want["trace"], (where, "(fi,fq)"))
    for k, a, b in zip(CKEYS, got["counters"], want["counters"]):
        if k != "centreBin" or fft:
            assert a == b, (where, k, a, b)
    keep = [i for i in range(18) if fft or i not in (6, 7)]
    assert_same(got["state"][keep], want["state"][keep], (where, "state", keep))
    assert got["fec"] == want["fec"], (where, "fec", [f[:2] for f in got["fec"]], [f[:2] for f in want["fec"]])
    assert got["decoded"] == want["decoded"], (where, "decoded")


def run_oracle(x, rate=96000, tuning=12000, frame=None, do_fft=0, do_up=0, upto=None):
    """one O.Bpsk over the floats x: tune mode in one frame (the chain is sample-sequential), FFT-acquire frame by frame"""
    n = x.size // 2
    D = rate // 9600
    if frame is None:
        o = O.Bpsk(rate=rate, blen=4 * n, tuning=tuning, trace=n // D + 8)
        o.receive(x)
    else:
        o = O.Bpsk(rate=rate, blen=4 * frame, tuning=tuning, do_fft=do_fft, do_up=do_up, trace=n // D + 8)
        for k in range((n if upto is None else upto) // frame):
            o.receive(x[2 * frame * k:2 * frame * (k + 1)])
    return o


# ---------------------------------------------------------------------------------------------------------------- tune mode
# The ragged calls of the batch test: 3 tiles of k_fm_f32 and a bit; shorter than the 26-sample history; a long one; the rest.
TUNE_CALLS = [3 * 40300 + 1237, 19, 200000 - 3, NSAMP - (3 * 40300 + 1237) - 19 - (200000 - 3)]
_C0, _C1, _C2 = TUNE_CALLS[0], TUNE_CALLS[0] + TUNE_CALLS[1], TUNE_CALLS[0] + TUNE_CALLS[1] + TUNE_CALLS[2]

# name -> (generator stream, off-grid factor, poison spec).  Twelve streams of the batch: k_tail8 puts streams 0..7 and 8..11 into
# one wave each, and every wave holds clean streams (2, 6 / 10) beside poisoned ones.
TUNE_CASES = [
    ("nan_i_hi", 3, 0.93, [(NAN_HI, I, NAN)]),
    ("nan_q", 2, 0.91, [(100003, Q, NAN)]),
    ("clean_a", 3, 0.93, []),
    ("inf_i_mid", 3, 0.93, [(INF_MID, I, PINF)]),
    ("ninf_q", 4, 0.89, [(300001, Q, NINF)]),
    ("huge_pair", 3, 0.93, [(150000, I, HUGE), (150000, Q, -HUGE), (150001, I, -HUGE), (150001, Q, HUGE)]),
    ("clean_b", 2, 0.91, []),
    ("nan_call_end", 4, 0.89, [(_C0 - 5, I, NAN)]),     # in the last 26 samples of call 0; the 19-sample call follows
    ("nan_call_first", 2, 0.91, [(_C2, Q, NAN)]),       # the first sample of call 3
    ("zeros_subnormals", 4, 0.89, [(7000, I, NZERO), (7000, Q, SUBN), (7001, I, -SUBN), (7001, Q, NZERO)]),
    ("clean_c", 4, 0.89, []),
    ("nan_late", 3, 0.93, [(400000, Q, NAN)]),
]
# Q = +Inf at each of eight consecutive samples: each of the eight phases of the 12 kHz tuner at 96 kHz once -- the table entry
# whose sine is exactly 0 (Inf x 0 = NaN) and the pass-through branch tuPhase <= 0 among them
INF_Q_FIRST = 250016
PHASE_CASES = [("inf_q_phase%d" % k, 2 + k % 3, (0.91, 0.93, 0.89)[k % 3], [(INF_Q_FIRST + k, Q, PINF)]) for k in range(8)]

_base = {}


def base_stream(stream, k, nsamp=NSAMP, rate=96000, seed=SEED, carrier_hz=13200.0):
    key = (seed, stream, k, nsamp, rate, carrier_hz)
    if key not in _base:
        x = offgrid(O.make_dbpsk_stream(seed, stream, nsamp, rate=rate, carrier_hz=carrier_hz, noise_sigma=900.0)[0], k)
        x.setflags(write=False)
        _base[key] = x
    return _base[key]


def tune_inputs(cases):
    """the float streams of TUNE_CASES / PHASE_CASES, in order"""
    return [poison(base_stream(g, k), spec) for _, g, k, spec in cases]


def first_poison(spec):
    return min(s for s, _, _ in spec) if spec else None


# ---------------------------------------------------------------------------------------------------------------- FFT-acquire
# (frame, rate): one frame size for each front-end family -- the 2^k LDS kernels (fused and three-phase), the mixed-radix ones at
# 9600 and 19200, the 4410 one, and the any-frame passes (512).  +-Inf is left out: which bins of a frame turn to Inf and which to
# NaN depends on the order of the transform's additions, JTransforms' order is unknown, so nothing could be pinned to the reference.
FFT_SIZES = [(2048, 96000), (9600, 96000), (19200, 96000), (4410, 44100), (512, 48000)]
FFT_FRAMES = 12
FFT_POISON_FRAME = 3


# (the generator stream of the NaN case where stream 5's peak happens to stand at 0 when the NaN arrives: a peak frozen at 0 could
#  not tell the reference's search from one that answers 0)
FFT_NAN_STREAM = {(2048, 0): 7, (2048, 1): 6, (512, 1): 6}


def fft_carrier(rate, do_up):
    return rate * (0.3125 if do_up else 0.1375)  # 30 kHz / 13.2 kHz at 96 kHz


def fft_inputs(n, rate, do_up, frames=FFT_FRAMES):
    """three streams of `frames` frames: a NaN in frame 3, +-3e38 in frame 3, clean"""
    N = n * frames
    gens = [FFT_NAN_STREAM.get((n, do_up), 5), 6, 7]
    xs = [base_stream(g, 0.93, nsamp=N, rate=rate, seed=8400 + n, carrier_hz=fft_carrier(rate, do_up)) for g in gens]
    p = FFT_POISON_FRAME * n
    return [poison(xs[0], [(p + 5, I, NAN)]), poison(xs[1], [(p + 7, I, HUGE), (p + 8, Q, -HUGE)]), np.array(xs[2])]


# ---------------------------------------------------------------------------------------------------------------- 44.1 kHz / 8 kHz
ODD_RATE, ODD_TUNING, ODD_NSAMP = 44100, 8000, 60000
ODD_CALLS = [23000 + 3, 17, 37000 - 20]
ODD_CASES = [("nan_i", [(9001, I, NAN)]), ("inf_q", [(30011, Q, PINF)]), ("clean", [])]


def odd_inputs():
    return [poison(base_stream(2 + s, 0.93, nsamp=ODD_NSAMP, rate=ODD_RATE, seed=SEED + 1, carrier_hz=ODD_TUNING + 1200.0), spec)
            for s, (_, spec) in enumerate(ODD_CASES)]


# ---------------------------------------------------------------------------------------------------------------- PSD
FLT_MAX = np.finfo(np.float32).max


def hz_rule(p, n, rate):
    """fft.java:214-216 on the int index p of the maximum's real part (p = 2 bin; -1: no maximum), in Java's int arithmetic"""
    datlen = 2 * n
    if p >= datlen // 2:
        p -= datlen
    v = (p * rate) & 0xFFFFFFFF
    v = v - (1 << 32) if v >= 1 << 31 else v
    q = abs(v) // datlen
    return np.float32(q if v >= 0 else -q)


def check_psd_nan_frame(g, n, rate, where):
    """a frame with a NaN in it: every bin NaN, no maximum (the p = -1 branch), m = -FLT_MAX"""
    assert np.isnan(g[:n]).all(), (where, int(np.isnan(g[:n]).sum()))
    assert g[n] == hz_rule(-1, n, rate) == np.float32(int(-rate / (2 * n))) and g[n + 1] == -FLT_MAX, (where, g[n], g[n + 1])


def check_psd_inf_frame(g, n, rate, where):
    """a frame with a +Inf in it, as far as the reference's text fixes it (which bins are Inf and which NaN is the transform's order)"""
    bins = g[:n]
    assert (np.isnan(bins) | (bins == np.inf)).all(), where
    hit = np.flatnonzero(bins == np.inf)
    if hit.size:
        assert g[n + 1] == np.inf and g[n] == hz_rule(2 * int(hit[0]), n, rate), (where, g[n], g[n + 1], hit[0])
    else:
        assert g[n + 1] == -FLT_MAX and g[n] == hz_rule(-1, n, rate), (where, g[n], g[n + 1])
