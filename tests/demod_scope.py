"""The demod scope (jsdr_demod_scope_*, csrc/demod_scope.hip): what tests/test_demod_scope_abi.py and
tests/test_gpu_demod_scope.py share.  CPU only: numpy and the C oracle (oracle_lib.Demod); no library call.

demod.paintComponent (demod.java:509-558) draws two polylines from what receive() left behind:
  the trace     from sam[]: sam[2k] is the final float of sample k (:472), sam[2k + 1] its mixed Q (0 in MODE_OFF)
  the spectrum  from the PSD of dbg[], the frame's mixed (I, Q) pairs (:436-437)
Ground truth is the oracle: oracle_lib.Demod.d.sam after receive() IS the painter's sam[]; dbg is the sam[] of a twin oracle
with the same band and switches but MODE_RAW and doagc = 0, fed the same frames (RAW leaves the mixed pair alone and a gain of
1 is exact) -- class Painter keeps the pair.

  layout(n, W)                   the two column schedules in float32, vectorised
  trace(sam, W, H), spec(psd, W, H)   the painters, vectorised over columns
  layout_java, trace_java, spec_java  the Java loops letter by letter, scalar; held equal to the above on small cases
  winners(sam, W)                per trace column, who won getAbsMax: -1 the final float, 0 the first Q, k >= 1 a later Q
  CENSUS_CASES                   designed signals and the outcomes each was designed to show
`python tests/demod_scope.py --write` writes tests/golden/demod_scope_census.json (data only) from the oracle alone."""
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS = os.path.join(HERE, "golden", "demod_scope_census.json")
F32 = np.float32
RATE = 96000
OFF, RAW, AM, NFM, WFM = range(5)
MODES = (OFF, RAW, AM, NFM, WFM)
BAND = (3000, 11000)
ALLPASS = (-2 ** 31, 2 ** 31 - 1)
WIDTH_CAP = 32768
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31

LAYOUT_N = (2, 7, 64, 100, 2048, 2049, 4410, 9600, 10241, 20000)
GPU_N = (7, 64, 2048, 2049, 4410, 9600, 10241)
SWITCHES = ((0, 0, 0), (1, 1, 1), (1, 1, 0), (0, 0, 1))  # (dofir, dodwn, doagc)
HEIGHTS = (0, 3, 400, 1001)
S = 3
CALLS = (2, 3, 2)  # frames a call
IC, QC = 37, -1200


def widths(n):
    """the grid's widths at frame size n, clipped to the cap: both sides of n/2 (scale 2 / 1), of n (scale 1 / 0, pi below 1), 2n,
    and two that divide neither the frame nor the tile (1000: scale 9, pi 9.6 at 9600)"""
    w = (1, 2, 3, n // 2, n // 2 + 1, n - 1, n, n + 1, 2 * n, 1000, 1024)
    return tuple(sorted({min(max(x, 1), WIDTH_CAP) for x in w}))


def java_int(x):
    """Java's (int) of float32 values: truncation, saturation, NaN -> 0"""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        t = np.trunc(x.astype(np.float64))
    t = np.where(np.isnan(t), 0.0, np.clip(t, INT_MIN, INT_MAX))
    return t.astype(np.int64)


def wrap32(v):
    """Java's int arithmetic: the low 32 bits, signed"""
    v = np.asarray(v, np.int64) & 0xFFFFFFFF
    return np.where(v >= 2 ** 31, v - 2 ** 32, v).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- vectorised
@functools.lru_cache(maxsize=None)
def layout(n, W):
    """(trace_first, trace_count, spec_first, spec_count), W entries each; the last trace entry and spectrum entry 0 are (0, 0)"""
    scale = F32(n // W)                                   # :519 (an int division)
    x = np.arange(W, dtype=np.int64)
    tf = (x.astype(F32) * scale).astype(np.int32)         # :527
    tc = np.full(W, int(scale), np.int32)
    tf[W - 1] = tc[W - 1] = 0
    pi = F32(F32(n) / F32(W))                             # :544
    sf = (pi * x.astype(F32)).astype(np.int32)            # :550
    sc = np.full(W, int(pi), np.int32)
    sf[0] = sc[0] = 0
    for a in (tf, tc, sf, sc):
        a.setflags(write=False)
    return tf, tc, sf, sc


def layout_inside(n, W):
    """whether the reference stays inside sam[] and psd[] at (n, W)"""
    tf, tc, sf, sc = layout(n, W)
    cnt, pcnt = int(tc[0]) if W > 1 else 0, int(sc[1]) if W > 1 else 0
    t = tf[:W - 1]
    ok = bool(((t >= 0) & (t < n) & (t + cnt // 2 <= n)).all())
    m = sf[1:]
    return ok and bool(((m >= 0) & (m < n) & (m + pcnt <= n)).all())


def absmax_columns(sam, W):
    """getAbsMax(sam, 2i, (int)scale, 2) of every column x < W - 1: (r, winner), winner -1 the final float, k the Q of sample i + k"""
    sam = np.asarray(sam, F32)
    n = sam.size // 2
    tf, tc, _, _ = layout(n, W)
    i = tf[:W - 1].astype(np.int64)
    cnt = int(tc[0]) if W > 1 else 0
    r = sam[2 * i].copy()
    c = np.abs(r)
    win = np.full(i.size, -1, np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(cnt // 2):       # idx = 2i + 1, 2i + 3, .. < 2i + cnt
            q = sam[2 * (i + k) + 1]
            take = np.abs(q) > c
            r = np.where(take, q, r)
            win = np.where(take, k, win)
            c = np.abs(r)
    return r, win


def trace(sam, W, H):
    """int32 [W]: entry 0 is H/4, entry x + 1 is y of column x (:519-531)"""
    r, _ = absmax_columns(sam, W)
    h = F32(H // 4)
    with np.errstate(invalid="ignore", over="ignore"):
        y = wrap32(H // 4 - java_int(r * h))
    return np.concatenate([np.array([H // 4], np.int32), y])


def winners(sam, W):
    return absmax_columns(sam, W)[1]


def spec(psd, W, H):
    """int32 [W]: entry 0 is H/2 + (int)(psd[0] * h), entry m is H/2 + (int)(getMax(psd, i, (int)pi) * h) (:544-555)"""
    psd = np.asarray(psd, F32)
    n = psd.size
    _, _, sf, sc = layout(n, W)
    i = sf.astype(np.int64)
    cnt = int(sc[1]) if W > 1 else 0
    r = psd[i].copy()
    with np.errstate(invalid="ignore"):
        for k in range(1, cnt):
            v = psd[np.minimum(i + k, n - 1)]
            take = v > r
            take[0] = False             # entry 0 is psd[0] alone
            r = np.where(take, v, r)
    h = F32(F32(H // 2) / F32(-100.0))  # :547
    with np.errstate(invalid="ignore", over="ignore"):
        return wrap32(H // 2 + java_int(r * h))


# ---------------------------------------------------------------------------------------------------------------- letter by letter
def layout_java(n, W):
    tf, tc, sf, sc = ([0] * W for _ in range(4))
    scale = F32(n // W)
    for x in range(W - 1):
        tf[x] = int(F32(F32(x) * scale))
        tc[x] = int(scale)
    pi = F32(F32(n) / F32(W))
    for m in range(1, W):
        sf[m] = int(F32(pi * F32(m)))
        sc[m] = int(pi)
    return tuple(np.array(a, np.int32) for a in (tf, tc, sf, sc))


def get_abs_max_java(a, o, l, s):
    r = a[o]
    c = abs(r)
    i = o + 1
    while i < o + l:
        if abs(a[i]) > c:
            r = a[i]
        c = abs(r)     # (no braces in the reference: outside the if)
        i += s
    return r


def get_max_java(a, o, l):
    r = a[o]
    for i in range(o + 1, o + l):
        if a[i] > r:
            r = a[i]
    return r


def java_int1(v):
    return int(java_int(np.array([v], F32))[0])


def trace_java(sam, W, H):
    sam = [F32(v) for v in sam]
    n = len(sam) // 2
    scale = F32(n // W)
    out = [H // 4]
    h = F32(H // 4)
    with np.errstate(invalid="ignore", over="ignore"):
        for x in range(W - 1):
            i = int(F32(F32(x) * scale))
            out.append(H // 4 - java_int1(F32(get_abs_max_java(sam, i * 2, int(scale), 2) * h)))
    return wrap32(out)


def spec_java(psd, W, H):
    psd = [F32(v) for v in psd]
    n = len(psd)
    pi = F32(F32(n) / F32(W))
    h = F32(F32(H // 2) / F32(-100.0))
    with np.errstate(invalid="ignore", over="ignore"):
        out = [H // 2 + java_int1(F32(psd[0] * h))]
        for m in range(1, W):
            i = int(F32(pi * F32(m)))
            out.append(H // 2 + java_int1(F32(get_max_java(psd, i, int(pi)) * h)))
    return wrap32(out)


# ---------------------------------------------------------------------------------------------------------------- the oracle pair
class Painter:
    """one stream of demod.java and its twin (MODE_RAW, doagc = 0): receive() returns (audio int16, sam float32 [2n], dbg float32 [2n])"""

    def __init__(self, mode, dofir, dodwn, doagc, band, rate=RATE):
        import oracle_lib as O
        self.o, self.twin = O.Demod(rate), O.Demod(rate)
        for d in (self.o, self.twin):
            d.weights(*band)
        self.configure(mode, dofir, dodwn, doagc)

    def configure(self, mode, dofir, dodwn, doagc):
        self.o.configure(mode, dofir, dodwn, doagc)
        self.twin.configure(RAW, dofir, dodwn, 0)

    def receive(self, buf):
        buf = np.ascontiguousarray(buf, F32)
        audio = self.o.receive(buf)
        self.twin.receive(buf)
        sam = np.ctypeslib.as_array(self.o.d.sam)[:buf.size].copy()
        dbg = np.ctypeslib.as_array(self.twin.d.sam)[:buf.size].copy()
        return audio, sam, dbg


@functools.lru_cache(maxsize=None)
def signal(n, frames=sum(CALLS), streams=S):
    """int16 IQ [streams][2 * frames * n]: the suite's fm_am_signal, one carrier a stream"""
    from test_gpu_demod import fm_am_signal
    rng = np.random.default_rng(11 * n + 5)
    raws = np.stack([fm_am_signal(rng, frames * n, RATE, fc=5000.0 + 900.0 * s, seed_shift=31.0 * s) for s in range(streams)])
    raws.setflags(write=False)
    return raws


# ---------------------------------------------------------------------------------------------------------------- the census
# name -> (n, W, mode, (dofir, dodwn, doagc), band, outcomes it was designed to show): (int)scale >= 2, mode != OFF
#   with AGC the final float fills [-1, 1] and the Qs stay near the input's 0.35: finals win most columns, Qs where the audio
#   passes through zero; without it RAW's final is the I beside its own Q, a fair fight for every candidate
CENSUS_CASES = {
    "nfm_agc_scale9": (9600, 1000, NFM, (1, 1, 1), BAND, ("final", "first_q", "later_q")),
    "raw_plain_scale4": (2048, 512, RAW, (0, 0, 0), ALLPASS, ("final", "first_q", "later_q")),
    "am_agc_scale4": (4410, 1000, AM, (1, 1, 1), BAND, ("final", "first_q", "later_q")),
    "wfm_scale2_one_q": (2048, 1024, WFM, (1, 1, 0), BAND, ("final", "first_q")),
    "raw_scale3_one_q": (2049, 683, RAW, (0, 0, 1), ALLPASS, ("final", "first_q")),
    "raw_agc_scale5_two_q": (10241, 2048, RAW, (1, 1, 1), BAND, ("final", "first_q", "later_q")),
}


def census_of(name):
    import oracle_lib as O
    n, W, mode, sw, band, _ = CENSUS_CASES[name]
    raws = signal(n)
    final = first = later = cols = 0
    for s in range(S):
        p = Painter(mode, *sw, band)
        buf = O.convert_i16(raws[s], ic=IC, qc=QC)
        for f in range(sum(CALLS)):
            _, sam, _ = p.receive(buf[2 * f * n:2 * (f + 1) * n])
            w = winners(sam, W)
            final += int((w < 0).sum())
            first += int((w == 0).sum())
            later += int((w > 0).sum())
            cols += w.size
    return dict(n=n, width=W, mode=mode, switches=list(sw), columns=cols, final=final, first_q=first, later_q=later)


def summary():
    return {name: census_of(name) for name in CENSUS_CASES}


def dumps(s):
    return json.dumps(s, indent=None, separators=(",", ":")) + "\n"


def load():
    with open(CENSUS) as f:
        return json.load(f)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    s = summary()
    for k, v in s.items():
        print(k, v)
    if "--write" in sys.argv:
        with open(CENSUS, "w") as f:
            f.write(dumps(s))
        print("wrote", CENSUS)
