"""Bit-clock peak walks for the BPSK tail kernels: what tests/golden/make_peak_walk_census.py, tests/test_peak_walk_oracle.py and
tests/test_gpu_peak_walk.py share.

The 9600 Hz tail (FUNcubeBPSKDemod.java:534-593) is the one stage whose control flow depends on the data: a decision falls where
dmBitPos == dmPeakPos (:537), dmPeakPos takes dmNewPeak at dmBitPos == dmHalfTable[dmPeakPos] (:577-579), and dmNewPeak is the first
maximum of the eight smoothed energies after every bit period (:586-592).  k_tail and k_tail8 (csrc/bpsk_tail.hip) speculate that
the peak stays put and otherwise go through a closed form of that machine that shares nothing with the oracle's plain loop.  The
synthetic streams of oracle_lib start symbol 0 at sample 0, so they all lock at position 4; the inputs here lock at each of the eight
positions (a delay in front of the stream), let the argmax wander over every position (noise only) and lose and regain lock at
another position (a fade), and census() counts, ON THE ORACLE ALONE, which moves dmPeakPos -> dmPeakPos' they contain.

Names: g is the index of a 9600 Hz sample (sample g leaves the down-sampler with input sample 10 g + 9 at 96 kHz), its bit position
is g mod 8, its bit period g // 8.  A hand-over (pk, nw, g) is dmPeakPos changing from pk to nw while sample g is processed, which
happens at g mod 8 == h = (pk + 4) mod 8.  In that period the old peak decides first unless h < pk (pk >= 4), and the new peak
decides in the same period if nw > h.

Everything here is CPU only (numpy and the C oracle)."""
import functools
import json
import os

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS = os.path.join(HERE, "golden", "peak_walk_census.json")

RATE, DECIM, SPB = 96000, 10, 8
AMP, SIGMA = 3000, 300.0   # the locked streams: a clean signal
NOISE_SIGMA = 1500.0       # the noise-only streams: energy2 > 100 (:544) at almost every decision

# delay in input samples -> the position the demodulator locks at (measured on the oracle; test_peak_walk_oracle.py re-measures)
DELAY_OF_POSITION = {0: 30, 1: 45, 2: 50, 3: 65, 4: 0, 5: 5, 6: 10, 7: 25}


# ---------------------------------------------------------------------------------------------------------------- generators
def delayed(seed, stream, n, d):
    """make_dbpsk_stream(seed, stream) behind d input samples of silence: symbol 0 starts at sample d"""
    iq = O.make_dbpsk_stream(seed, stream, n, amp=AMP, noise_sigma=SIGMA)[0]
    out = np.zeros(2 * n, np.int16)
    out[2 * d:] = iq[:2 * (n - d)]
    return out


def noise_only(seed, stream, n):
    return O.make_dbpsk_stream(seed, stream, n, amp=0, noise_sigma=NOISE_SIGMA)[0]


def fading(seed, stream, n, d1, d2, fade_at, fade_symbols):
    """the signal at delay d1, nothing but its noise for fade_symbols symbols from symbol fade_at on, then the signal at delay d2"""
    sps = RATE // 1200
    a, b = delayed(seed, stream, n, d1), delayed(seed, stream, n, d2)
    quiet = O.make_dbpsk_stream(seed, stream, n, amp=0, noise_sigma=SIGMA)[0]
    c1, c2 = sps * fade_at, sps * (fade_at + fade_symbols)
    assert 0 < c1 < c2 < n
    return np.concatenate([a[:2 * c1], quiet[2 * c1:2 * c2], b[2 * c2:]])


# ---------------------------------------------------------------------------------------------------------------- the case list
# Chosen offline on the oracle (make_peak_walk_census.py prints what each case adds); fixed here.
N_LOCKED = 2048 * 50   # 1280 bit periods
N_WALK = 2048 * 100
SEED_LOCKED, SEED_WALK = 7, 31
DELAYED = [("delayed", SEED_LOCKED, p, N_LOCKED, DELAY_OF_POSITION[p]) for p in range(8)]  # case p locks at position p
# (of streams 0 .. 63 of seed 31, these four hold 55 of the 56 moves between them, and all 64 together no more; 6 -> 1 turned up
#  once in 256 streams of four more seeds, at g = 6842 of stream 51 of seed 33)
NOISE = [("noise", SEED_WALK, s, N_WALK) for s in (50, 24, 16, 21)] + [("noise", 33, 51, N_WALK)]
FADING = [("fading", SEED_LOCKED, 50, N_WALK, DELAY_OF_POSITION[5], DELAY_OF_POSITION[0], 600, 300),
          ("fading", SEED_LOCKED, 68, N_WALK, DELAY_OF_POSITION[7], DELAY_OF_POSITION[2], 600, 300)]
NINTH_LOCKED = ("delayed", SEED_LOCKED, 8, N_LOCKED, DELAY_OF_POSITION[1])  # alone in a second wave of k_tail8
WALKS = NOISE + FADING
MIXED_WALK = NOISE[4]  # its first N_LOCKED samples ride in a wave of locked streams (6 -> 1 is among them)
CASES = DELAYED + WALKS


@functools.lru_cache(maxsize=None)
def stream_of(case):
    kind, args = case[0], case[1:]
    iq = {"delayed": delayed, "noise": noise_only, "fading": fading}[kind](*args)
    iq.setflags(write=False)
    return iq


def name_of(case):
    return "%s(%s)" % (case[0], ",".join(str(v) for v in case[1:]))


# ---------------------------------------------------------------------------------------------------------------- the census
def walk(iq, rate=RATE, tuning=12000):
    """O.Bpsk stepped one 9600 Hz sample (10 input samples at 96 kHz) at a time -> per g: dmPeakPos and dmNewPeak AFTER sample g,
    cntBit after it"""
    iq = np.ascontiguousarray(iq, np.int16)
    L = O.lib()
    decim = rate // 9600
    o = O.Bpsk(rate=rate, blen=4 * decim, size=4, tuning=tuning)
    nds = iq.size // (2 * decim)
    ist, cnt = np.empty(6, np.int32), np.empty(10, np.int32)
    pi, pc, base = O.ptr(ist), O.ptr(cnt), iq.ctypes.data
    pk, nw, bits = np.empty(nds, np.int8), np.empty(nds, np.int8), np.empty(nds, np.int32)
    for g in range(nds):
        L.jo_bpsk_receive_i16(o.h, base + 4 * decim * g, decim, 0, 0)
        L.jo_bpsk_istate(o.h, pi)
        L.jo_bpsk_counters(o.h, pc)
        # the bit clock is exactly periodic: what both kernels build on (and the handle checks at create time)
        assert ist[3] == (g + 1) % SPB and cnt[1] == g + 1, (g, ist, cnt)
        pk[g], nw[g], bits[g] = ist[4], ist[5], cnt[2]
    return pk, nw, bits


def census(iq, rate=RATE, tuning=12000):
    """what the peak machine does on this input, by the oracle alone:
    handovers  [(g, pk, nw)]: dmPeakPos went from pk to nw while sample g was processed
    two, none  bit periods with two decisions (cntBit rose by 2) / with no decision point at all (no sample of the period met
               dmBitPos == dmPeakPos); none_bits: periods in which cntBit did not rise (these and the silent ones)
    final      (dmPeakPos, dmNewPeak) at the end;  locked: (position, bit clocks, first bit period) of the longest run of whole bit
               periods with dmPeakPos == dmNewPeak == position throughout"""
    pk, nw, bits = walk(iq, rate, tuning)
    nper = pk.size // SPB
    before = np.concatenate([[0], pk[:-1]]).astype(np.int8)  # dmPeakPos starts at 0
    at = np.flatnonzero(pk != before)
    handovers = [(int(g), int(before[g]), int(pk[g])) for g in at]
    assert all(g % SPB == (p + 4) % SPB for g, p, _ in handovers)  # :577-579
    decides = (np.arange(pk.size) % SPB == before)[:nper * SPB].reshape(nper, SPB).sum(1)
    assert decides.max() <= 2
    rose = np.diff(np.concatenate([[0], bits[SPB - 1:nper * SPB:SPB]]))
    assert (rose <= decides).all()
    still = ((pk == nw)[:nper * SPB].reshape(nper, SPB).all(1)) & (pk[:nper * SPB:SPB] == pk[SPB - 1:nper * SPB:SPB])
    best, run, pos = (0, 0, 0), 0, -1
    for p in range(nper):
        here = int(pk[SPB * p]) if still[p] else -1
        run = run + 1 if here >= 0 and here == pos else (1 if here >= 0 else 0)
        pos = here
        if run > best[1]:
            best = (pos, run, p + 1 - run)
    return dict(handovers=handovers, two=int((rose == 2).sum()), none=int((decides == 0).sum()), none_bits=int((rose == 0).sum()),
                final=(int(pk[-1]), int(nw[-1])), locked=best, periods=nper)


def same_period_decision(pk, nw):
    """after the hand-over pk -> nw the new peak still decides in the period of the hand-over"""
    return nw > (pk + 4) % SPB


def moves_of(censuses):
    """8 x 8 counts of the moves pk -> nw over a list of censuses"""
    m = np.zeros((SPB, SPB), np.int64)
    for c in censuses:
        for _, p, q in c["handovers"]:
            m[p, q] += 1
    return m


# ---------------------------------------------------------------------------------------------------------------- call schedules
def locked_calls(n=N_LOCKED):
    """call lengths (input samples) for the locked streams: the acquisition in one call; every length of 1 .. 9 outputs from every
    start position g mod 8 (the nine lengths sum to 45 = 5 mod 8 outputs: eight rounds visit the eight starts); lengths that are
    no multiple of the decimation; one call of more than three chunks of either kernel (64 periods = 5120 samples) with whole
    chunks inside it; the rest"""
    calls = [20480 + 30]
    for _ in range(8):
        calls += [10 * k for k in range(1, 10)]
    calls += [1, 7, 13, 9, 25, 33, 77, 101, 3, 2, 5, 119, 81, 640, 641, 1279, 1281, 6]
    calls += [5 * 5120 + 10 * 3, 1280 * 3 + 10 * 5, 5120 + 70]
    calls.append(n - sum(calls))
    assert calls[-1] > 0
    return calls


def mixed_calls(n=N_LOCKED):
    """for the wave of seven locked streams and a wandering one: short calls, odd lengths, whole chunks of either kernel"""
    calls = [20480 + 30, 10, 30, 7, 640, 1281, 3 * 5120 + 50, 77, 80, 90, 4 * 1280 + 3]
    calls.append(n - sum(calls))
    assert calls[-1] > 0
    return calls


def spans(calls):
    """[(first g, end g)] of the 9600 Hz samples each call produces"""
    out, pos = [], 0
    for L in calls:
        out.append((pos // DECIM, (pos + L) // DECIM))
        pos += L
    return out


def seam_plan(censuses):
    """For every move pk -> nw the censuses hold, hand-overs of it and a call boundary inside the bit period of each: [(case index,
    g, pk, nw, b, kind)] with b the first 9600 Hz sample of the new call, 8 (g // 8) < b <= 8 (g // 8) + 7, and kind
      "old|hand"  the old peak's decision in the earlier call, the hand-over point in the new one (pk < b mod 8 <= h; needs pk < 4)
      "hand|new"  the hand-over point in the earlier call, the new peak's decision in the new one (h < b mod 8 <= nw; needs nw > h)
      "inside"    any other place inside the period
    One hand-over per move takes the first kind it admits; moves that admit both get a second hand-over for the other.  All streams
    of a handle share the boundaries, and they are at least one sample apart, whatever the case."""
    per = {}
    for ci, c in enumerate(censuses):
        for g, p, q in c["handovers"]:
            per.setdefault((p, q), []).append((ci, g))
    plan, used = [], set()

    def place(p, q, kind, skip):
        h = (p + 4) % SPB
        for k, (ci, g) in enumerate(per[(p, q)]):
            if k in skip or g < 2 * SPB:
                continue
            base = g - g % SPB
            if kind == "old|hand":
                pos = list(range(p + 1, h + 1))
            elif kind == "hand|new":
                pos = list(range(h + 1, q + 1))
            else:
                pos = [x for x in range(1, SPB) if not (p < x <= h) and not (h < x <= q)] or list(range(1, SPB))
            pos = pos[(p + q + len(plan)) % len(pos):] + pos[:(p + q + len(plan)) % len(pos)]
            for x in pos:
                # (a boundary of another hand-over may fall into this period only if it is this one)
                if all((b == base + x) or not (base < b <= base + 7) for b in used):
                    used.add(base + x)
                    plan.append((ci, g, p, q, base + x, kind))
                    return k
        return None

    for (p, q) in sorted(per):
        h = (p + 4) % SPB
        kinds = (["old|hand"] if p < h else []) + (["hand|new"] if q > h else [])
        taken = set()
        for kind in kinds or ["inside"]:
            k = place(p, q, kind, taken)
            if k is None and not taken:
                k = place(p, q, "inside", taken)
            if k is not None:
                taken.add(k)
        assert taken, (p, q)
    return plan


def seam_calls(plan, n):
    """the boundaries of a plan as call lengths over n input samples; the new call starts r = b mod 10 input samples late inside the
    gap before sample b's last input (10 b + 9), so that most lengths are no multiple of the decimation"""
    cuts = sorted(set(DECIM * b + b % DECIM for _, _, _, _, b, _ in plan))
    assert cuts[0] > 0 and cuts[-1] < n
    edges = [0] + cuts + [n]
    return [b - a for a, b in zip(edges, edges[1:])]


# ---------------------------------------------------------------------------------------------------------------- the fixture
def summary(censuses, cases=None):
    """the JSON's content, from censuses of CASES in order"""
    cases = CASES if cases is None else cases
    m = moves_of(censuses)
    walks = censuses[len(DELAYED):]
    plan = seam_plan(walks)
    return dict(
        delays={str(p): d for p, d in sorted(DELAY_OF_POSITION.items())},
        cases=[dict(name=name_of(k), handovers=len(c["handovers"]), two=c["two"], none=c["none"], none_bits=c["none_bits"],
                    final=list(c["final"]), locked=list(c["locked"])) for k, c in zip(cases, censuses)],
        moves=[[int(v) for v in row] for row in m],
        missing=[[p, q] for p in range(SPB) for q in range(SPB) if p != q and m[p, q] == 0],
        two=sum(c["two"] for c in censuses), none=sum(c["none"] for c in censuses),
        seams=[[ci, g, p, q, b, kind] for ci, g, p, q, b, kind in plan])


def load():
    with open(CENSUS) as f:
        return json.load(f)
