"""The BPSK scope (jsdr_bpsk_scope_i16 / _f32): what the tests share.

Two statements of what FUNcubeBPSKDemod's painter sees after receive() of a frame (FUNcubeBPSKDemod.java:118-125, :231-268):

  rows_of / Restated   the numpy RESTATEMENT: the rows of a frame placed by the geometry of include/jsdr_hip.h from what the C
                       oracle's instruments say of a stream -- jo_bpsk_trace (fi, fq), jo_bpsk_trace_ds, jo_bpsk_declog_pos (g, di,
                       energy2 of every detector instant), jo_bpsk_sincos with the tuner recurrence of :381-396 in Python;
  Literal              the Java text again, line by line: ring arrays and their indices stepped sample by sample (:470-595), and
                       the painter's loops (:232-262).  It owns its whole demodulator, so that tuning changes (actionPerformed,
                       :177-190) and setup (:192-209) are stated by the same text.

tests/test_bpsk_scope_oracle.py holds the two to each other on every case, without a device; tests/test_gpu_bpsk_scope.py holds
the library to them.  Everything is bit for bit: `same` compares doubles as bit patterns, any NaN equal to any NaN.
"""
import json
import math
import os

import numpy as np

import oracle_lib as O

F64, F32, I64, U64 = np.float64, np.float32, np.int64, np.uint64
HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS = os.path.join(HERE, "golden", "bpsk_scope_census.json")
INT_MAX, INT_MIN = 2147483647, -2147483648
TWO_PI = 2.0 * math.pi
OUTPUTS = ("tuned", "ds", "iq", "max", "pts", "bits")


def same(a, b):
    """float64 arrays equal bit for bit, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, F64), np.ascontiguousarray(b, F64)
    return a.shape == b.shape and bool(((a.view(U64) == b.view(U64)) | (np.isnan(a) & np.isnan(b))).all())


def jint(x):
    """Java's (int) of doubles: truncates, saturates, NaN -> 0"""
    x = np.asarray(x, F64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.where(np.isnan(x), 0.0, x))
        return np.clip(t, INT_MIN, INT_MAX).astype(I64).astype(np.int32)


def ring_len(rate, n):
    return n * 9600 // rate  # samples*DOWN_SAMPLE_RATE/adsc.rate, ints (:201)


def g_first(rate, n, n_in, frames, origin=0):
    """G_0 .. G_frames of a call of `frames` frames that starts n_in samples into the stream (n_in a multiple of n)"""
    D = rate // 9600
    return np.array([(n_in + f * n) // D - origin for f in range(frames + 1)], I64)


# ---------------------------------------------------------------------------------------------------------------- the tuner
def tuner_inc(tuning, rate):
    return TWO_PI * tuning / float(rate)  # :188, :196


class Tuner:
    """RxMixTuner's phase (:381-396): per sample the table index, or -1 where the sample passes unmixed"""

    def __init__(self, tuning, rate):
        self.rate, self.phase = rate, 0.0
        self.set(tuning)

    def set(self, tuning):
        self.inc = tuner_inc(tuning, self.rate)

    def step(self, count):
        out = np.empty(count, np.int32)
        ph, inc = self.phase, self.inc
        for k in range(count):
            ph += inc
            if ph > TWO_PI:
                ph -= TWO_PI
            out[k] = int(ph * 256.0 / TWO_PI) % 256 if ph > 0.0 else -1
        self.phase = ph
        return out


def mix(buf, idx, sin_tab, cos_tab):
    """the pairs RxDownSample receives for a frame (float32 [2n]) under the indices idx: [n][2] doubles"""
    x = np.asarray(buf, F32).astype(F64).reshape(-1, 2)
    k = np.where(idx < 0, 0, idx)
    ci = np.where(idx < 0, 1.0, cos_tab[k])  # (i * 1.0 is i: the pass-through of :395)
    si = np.where(idx < 0, 1.0, sin_tab[k])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([x[:, 0] * ci, x[:, 1] * si], axis=1)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def painter(iq, re):
    """:232-262 over the ring images iq [L][2], re [L]: (mi, mq), pts int32 [L][4]"""
    a = np.abs(iq)
    mi = float(np.fmax.reduce(a[:, 0], initial=0.0))  # strict <, from 0.0: the largest |x| that is no NaN
    mq = float(np.fmax.reduce(a[:, 1], initial=0.0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xs, ys = F64(100.0) / F64(mi), F64(100.0) / F64(mq)
        rs = F64(50.0) / (F64(mi) * F64(mq))
        pts = np.stack([jint(iq[:, 0] * xs), jint(iq[:, 1] * ys), jint(iq[:, 1] * xs), jint(re * rs)], axis=1)
    return np.array([mi, mq], F64), pts


def rows_of(L, Ga, Gb, origin, tr, ds, dec_g, dec, tuned):
    """the six rows of one frame.  Ga, Gb: the frame's decimated samples, numbered since creation, [Ga, Gb); origin likewise;
    tr, ds: (fi, fq) and the down-sampler outputs of the stream since creation; dec_g, dec: the detector instants (g since
    creation; di, energy2); tuned: the frame's mixed pairs [n][2]"""
    assert Gb - Ga >= L
    g = np.arange(Gb - L, Gb)  # the last L samples of the frame: each slot's winner
    dsr = np.empty((L, 2), F64)
    iq = np.empty((L, 2), F64)
    dsr[(g - origin) % L] = ds[g]
    iq[(g - origin + 1) % L] = tr[g]
    bits = np.zeros(L, np.int8)
    re = np.zeros(L, F64)
    lo, hi = np.searchsorted(dec_g, [Ga, Gb])
    for k in range(lo, hi):  # ascending: a later bit overwrites
        if dec[k, 1] > 100.0:
            slot = (int(dec_g[k]) - origin + 1) % L
            bits[slot] = 1 if dec[k, 0] < 0.0 else -1
            re[slot] = dec[k, 0]
    mx, pts = painter(iq, re)
    return dict(tuned=np.ascontiguousarray(tuned, F64), ds=dsr, iq=iq, max=mx, pts=pts, bits=bits)


class Restated:
    """one stream through the C oracle, frame by frame; rows() of every frame received so far"""

    def __init__(self, rate, n, tuning, cap_frames):
        self.rate, self.n, self.D, self.L = rate, n, rate // 9600, ring_len(rate, n)
        self.o = O.Bpsk(rate=rate, blen=4 * n, size=4, tuning=int(tuning), trace=cap_frames * (n // self.D + 2))
        self.o.declog_enable(cap_frames * (n // self.D + 2))
        self.sin, self.cos = O.bpsk_sincos()
        self.tuned = []
        self.frames = 0

    def receive(self, buf, idx):
        """a frame (float32 [2n]) whose samples the tuner mixes with the indices idx (Tuner.step: shared by lock-step streams)"""
        self.o.receive(buf)
        self.tuned.append(mix(buf, idx, self.sin, self.cos))
        self.frames += 1

    def rows(self, first, count, origin=0):
        """the rows of frames first .. first + count - 1 (numbered since creation): name -> [count][...]"""
        tr, ds = self.o.trace(), self.o.trace_ds()
        dec_g, dec = self.o.declog_pos()
        n, D = self.n, self.D
        per = [rows_of(self.L, (F * n) // D, ((F + 1) * n) // D, origin, tr, ds, dec_g, dec, self.tuned[F])
               for F in range(first, first + count)]
        return {k: np.stack([r[k] for r in per]) for k in OUTPUTS}


# ---------------------------------------------------------------------------------------------------------------- the Java text
def _seq(prod):
    """a sum from 0.0 in index order, one rounding a term (numpy's cumsum adds in order)"""
    return float(np.cumsum(np.concatenate(([0.0], prod)))[-1])


class Literal:
    """FUNcubeBPSKDemod in the tune mode, as written, up to the bit decision (:544-551): the rings and the painter's first panel"""

    def __init__(self, rate, n, tuning):
        self.rate, self.samples = rate, n
        self.sinTab, self.cosTab = O.bpsk_sincos()
        self.dsFilter, self.dmFilter = O.bpsk_table(0), O.bpsk_table(1)
        assert self.dsFilter.size == 27 and self.dmFilter.size == 130
        self.tuPhase = 0.0
        self.dsBuf = np.zeros((27, 2), F64)
        self.dsPos, self.dsCnt = 26, 0
        self.vcoPhase = 0.0
        self.dmBuf = np.zeros((65, 2), F64)
        self.dmPos = 64
        self.dmEnergy = [0.0] * 10
        self.dmBitPos = self.dmPeakPos = self.dmNewPeak = 0
        self.dmEnergyOut = 1.0
        self.dmBitPhase = 0.0
        self.dmLastIQ = [0.0, 0.0]
        self.cntBit = 0
        self.peak_moves = 0
        self.log_ds, self.log_tr, self.log_dec = [], [], []  # instruments, as the oracle's: per g, and per detector instant (g, di, energy2)
        self.setup(tuning)

    def setup(self, tuning):  # :192-209
        n = self.samples
        self.tuning = float(int(tuning))
        self.tuPhaseInc = TWO_PI * self.tuning / float(self.rate)
        self.tuned = np.zeros(2 * n, F64)
        self.tunedIdx = 0
        self.demodIQ = np.zeros(n * 9600 // self.rate * 2, F64)
        self.demodIdx = 0
        self.downSmpl = np.zeros(self.demodIQ.size, F64)
        self.downSmplIdx = 0
        self.demodBits = np.zeros(self.demodIQ.size // 2, np.int32)
        self.demodRe = np.zeros(self.demodIQ.size // 2, F64)

    def action(self, tuning):  # :175-188, the frequency dialog
        self.tuning = float(tuning)
        self.tuPhaseInc = TWO_PI * self.tuning / float(self.rate)

    def receive(self, buf):  # :366-376
        self.demodBits[:] = 0
        self.demodRe[:] = 0.0
        buf = np.asarray(buf, F32)
        for k in range(self.samples):
            self.RxMixTuner(float(buf[2 * k]), float(buf[2 * k + 1]))

    def RxMixTuner(self, i, q):  # :382-397
        self.tuPhase += self.tuPhaseInc
        if self.tuPhase > TWO_PI:
            self.tuPhase -= TWO_PI
        if self.tuPhase > 0.0:
            k = int(self.tuPhase * 256.0 / TWO_PI) % 256
            self.RxDownSample(i * self.cosTab[k], q * self.sinTab[k])
        else:
            self.RxDownSample(i, q)

    def RxDownSample(self, i, q):  # :470-492
        self.tuned[self.tunedIdx] = i
        self.tuned[self.tunedIdx + 1] = q
        self.tunedIdx = (self.tunedIdx + 2) % self.tuned.size
        self.dsBuf[self.dsPos, 0] = i
        self.dsBuf[self.dsPos, 1] = q
        self.dsCnt += 1
        if self.dsCnt >= self.rate // 9600:
            order = (np.arange(27) + self.dsPos) % 27
            with np.errstate(invalid="ignore", over="ignore"):
                fi = _seq(self.dsBuf[order, 0] * self.dsFilter)
                fq = _seq(self.dsBuf[order, 1] * self.dsFilter)
            self.dsCnt = 0
            H = 0.9 * 32768.0
            self.RxDemodulate(fi * H, fq * H)
        self.dsPos -= 1
        if self.dsPos < 0:
            self.dsPos = 26

    def RxDemodulate(self, i, q):  # :505-595
        self.downSmpl[self.downSmplIdx] = i
        self.downSmpl[self.downSmplIdx + 1] = q
        self.downSmplIdx = (self.downSmplIdx + 2) % self.downSmpl.size
        self.log_ds.append((i, q))
        self.vcoPhase += TWO_PI * 1200.0 / 9600.0
        if self.vcoPhase > TWO_PI:
            self.vcoPhase -= TWO_PI
        k = int(self.vcoPhase * 256.0 / TWO_PI) % 256
        self.dmBuf[self.dmPos, 0] = i * self.cosTab[k]
        self.dmBuf[self.dmPos, 1] = q * self.sinTab[k]
        taps = self.dmFilter[65 - self.dmPos:130 - self.dmPos]
        with np.errstate(invalid="ignore", over="ignore"):
            fi = _seq(self.dmBuf[:, 0] * taps)
            fq = _seq(self.dmBuf[:, 1] * taps)
        self.dmPos -= 1
        if self.dmPos < 0:
            self.dmPos = 64
        self.demodIdx = (self.demodIdx + 2) % self.demodIQ.size
        self.demodIQ[self.demodIdx] = fi
        self.demodIQ[self.demodIdx + 1] = fq
        self.log_tr.append((fi, fq))
        energy1 = fi * fi + fq * fq
        b = self.dmBitPos
        self.dmEnergy[b] = (self.dmEnergy[b] * (1.0 - 1.0 / 200.0)) + (energy1 * (1.0 / 200.0))
        if b == self.dmPeakPos:
            di = -(self.dmLastIQ[0] * fi + self.dmLastIQ[1] * fq)
            dq = self.dmLastIQ[0] * fq - self.dmLastIQ[1] * fi
            self.dmLastIQ = [fi, fq]
            s = di * di + dq * dq
            energy2 = math.sqrt(s) if s == s and s != math.inf else s
            self.log_dec.append((len(self.log_tr) - 1, di, energy2))
            if energy2 > 100.0:
                self.demodRe[self.demodIdx // 2] = di
                self.demodBits[self.demodIdx // 2] = 1 if di < 0.0 else -1
                self.cntBit += 1
        if b == (4, 5, 6, 7, 0, 1, 2, 3)[self.dmPeakPos]:
            if self.dmPeakPos != self.dmNewPeak:
                self.peak_moves += 1
            self.dmPeakPos = self.dmNewPeak
        self.dmBitPos = (b + 1) % 8
        self.dmBitPhase += 1.0 / 9600.0
        if self.dmBitPhase >= 1.0 / 1200.0:
            self.dmBitPhase -= 1.0 / 1200.0
            self.dmBitPos = 0
            eMax = float(F32(-1.0e10))
            for m in range(8):
                if self.dmEnergy[m] > eMax:
                    self.dmNewPeak = m
                    eMax = self.dmEnergy[m]

    def paint(self):  # :232-262: (mi, mq), the integers per slot
        d = self.demodIQ
        mi = mq = 0.0
        for m in range(0, d.size, 2):
            if mi < abs(d[m]):
                mi = abs(float(d[m]))
            if mq < abs(d[m + 1]):
                mq = abs(float(d[m + 1]))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            xs, ys = F64(100.0) / F64(mi), F64(100.0) / F64(mq)
            rs = F64(50.0) / (F64(mi) * F64(mq))
            pts = np.stack([jint(d[0::2] * xs), jint(d[1::2] * ys), jint(d[1::2] * xs), jint(self.demodRe * rs)], axis=1)
        return np.array([mi, mq], F64), pts

    def logs(self):
        """(tr [G][2], ds [G][2], dec_g [K], dec [K][2]) so far, as rows_of takes the oracle's"""
        dec = np.array(self.log_dec, F64).reshape(-1, 3)
        return (np.array(self.log_tr, F64).reshape(-1, 2), np.array(self.log_ds, F64).reshape(-1, 2), dec[:, 0].astype(I64),
                np.ascontiguousarray(dec[:, 1:]))

    def rows(self):
        """what the painter sees now, as the scope's rows of one frame"""
        mx, pts = self.paint()
        return dict(tuned=self.tuned.reshape(-1, 2).copy(), ds=self.downSmpl.reshape(-1, 2).copy(),
                    iq=self.demodIQ.reshape(-1, 2).copy(), max=mx, pts=pts, bits=self.demodBits.astype(np.int8))


def rows_equal(a, b):
    """names of the outputs in which two row dicts differ"""
    bad = []
    for k in OUTPUTS:
        ok = same(a[k], b[k]) if k in ("tuned", "ds", "iq", "max") else np.array_equal(a[k], b[k])
        if not ok:
            bad.append(k)
    return bad


# ---------------------------------------------------------------------------------------------------------------- the cases
def _signal(seed, stream, nsamples, rate, carrier, **kw):
    return O.make_dbpsk_stream(seed, stream, nsamples, rate=rate, carrier_hz=carrier, **kw)[0]


def case_input(case, stream=0):
    """the case's input for one stream: ("i16", int16 [2 total]) or ("f32", float32 [2 total])"""
    c = CASES[case]
    total = c["frames"] * c["n"]
    kind = c["kind"]
    if kind == "silence":
        return "i16", np.zeros(2 * total, np.int16)
    raw = _signal(c.get("seed", 11), stream, total, c["rate"], c["carrier"])
    if kind == "signal":
        return "i16", raw
    x = O.convert_i16(raw).copy()
    if kind == "tiny_i":    # I tiny against Q: xs = 100 / mi is huge and (int)(Q * xs) saturates
        x[0::2] *= F32(1e-12)
    elif kind == "nan":     # one NaN in I and, later, one in Q, inside frame 1
        x[2 * (c["n"] + 700)] = np.nan
        x[2 * (c["n"] + 1500) + 1] = np.nan
    return "f32", x


def as_float(form, data):
    return O.convert_i16(data) if form == "i16" else np.asarray(data, F32)


# rate, frame, tuning, frames looked at, and what the census holds of each
CASES = {
    "96k":     dict(rate=96000, n=2048, tuning=12000, carrier=13200.0, frames=12, kind="signal"),
    "44k1":    dict(rate=44100, n=4410, tuning=12000, carrier=13200.0, frames=4, kind="signal"),
    "48k":     dict(rate=48000, n=4800, tuning=12000, carrier=13200.0, frames=4, kind="signal"),
    "silence": dict(rate=96000, n=2048, tuning=12000, carrier=13200.0, frames=3, kind="silence"),
    "fec":     dict(rate=48000, n=4800, tuning=12000, carrier=13200.0, frames=48, kind="signal", seed=5),
    "untuned": dict(rate=96000, n=2048, tuning=0, carrier=1200.0, frames=3, kind="signal"),  # tuPhase stays 0: every sample passes (:395)
    "tiny_i":  dict(rate=96000, n=2048, tuning=12000, carrier=13200.0, frames=4, kind="tiny_i"),
    "nan":     dict(rate=96000, n=2048, tuning=12000, carrier=13200.0, frames=4, kind="nan"),
}


def run_case(case, stream=0, literal=False):
    """the case through the restatement (and the Java text): (Restated, Literal or None, per frame the literal's rows)"""
    c = CASES[case]
    form, data = case_input(case, stream)
    x = as_float(form, data)
    n = c["n"]
    r = Restated(c["rate"], n, c["tuning"], c["frames"])
    t = Tuner(c["tuning"], c["rate"])
    lit = Literal(c["rate"], n, c["tuning"]) if literal else None
    lrows = []
    for f in range(c["frames"]):
        buf = x[2 * f * n:2 * (f + 1) * n]
        r.receive(buf, t.step(n))
        if lit:
            lit.receive(buf)
            lrows.append(lit.rows())
    return r, lit, lrows


def census_of(case):
    """what the case contains, from the oracle and the restatement alone"""
    c = CASES[case]
    n, rate = c["n"], c["rate"]
    D, L = rate // 9600, ring_len(rate, n)
    form, data = case_input(case)
    x = as_float(form, data)
    o = O.Bpsk(rate=rate, blen=4 * n, size=4, tuning=c["tuning"], trace=c["frames"] * (n // D + 2))
    o.declog_enable(c["frames"] * (n // D + 2))
    peak, dec = [], []
    for f in range(c["frames"]):
        o.receive(x[2 * f * n:2 * (f + 1) * n])
        peak.append(int(o.istate()[4]))
        dec.append(o.counters()["cntDec"])
    dec_g, dv = o.declog_pos()
    outs = [int(((f + 1) * n) // D - (f * n) // D) for f in range(c["frames"])]
    double, nobit = 0, 0
    for f in range(c["frames"]):
        lo, hi = np.searchsorted(dec_g, [(f * n) // D, ((f + 1) * n) // D])
        g = dec_g[lo:hi][dv[lo:hi, 1] > 100.0]
        slots = (g + 1) % L
        double += int(slots.size - np.unique(slots).size)
        nobit += int(g.size == 0)
    r, _, _ = run_case(case)
    rows = r.rows(0, c["frames"])
    return dict(L=L, outputs=sorted(set(outs)), slots_marked_twice=double, frames_without_a_bit=nobit,
                frames_in_which_peak_pos_moved=int(sum(1 for a, b in zip([0] + peak[:-1], peak) if a != b)),
                fec_decoded=int(dec[-1]), frames_with_mi_zero=int((rows["max"][:, 0] == 0.0).sum()),
                pts_saturated=int((np.abs(rows["pts"].astype(I64)) >= INT_MAX).sum()),
                nan_slots=int(np.isnan(rows["iq"]).any(axis=2).sum()), bits=int((rows["bits"] != 0).sum()))


def census():
    return {case: census_of(case) for case in CASES}


def load_census():
    with open(CENSUS) as f:
        return json.load(f)
