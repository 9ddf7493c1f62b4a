"""Engineered sync hits on the handle kinds that sync_cases.py does not reach: channel handles (rows input * nchannels + channel),
tuned handles (a tuner per stream), FFT-acquire handles (calls of whole frames), and the edge of a row's hit log.  What
tests/test_sync_handles_oracle.py and tests/test_gpu_sync_handles.py share; everything here is CPU only (numpy and the C oracle).

Every handle kind reaches the sync stage (k_sync_t / k_sync / k_sync_fin, the tail kernels' register, the FEC kernels' window)
through the same host code, but with its own schedule and row layout, and sync_cases.py feeds ordinary tune-mode handles only.
The streams are sync_cases' designed symbol streams, demodulated another way:

  a *variant* is how a stream is made and demodulated -- ("tune", t): the stream on a carrier of t + 1200 Hz, a demodulator tuned
  to t (t <= 0: the tuner passes the samples through, the stream stays at 13 200 Hz and gives garbage bits); ("fft", frame): the
  13 200 Hz stream trimmed to whole frames, a demodulator in FFT-acquire (do_fft = 1, do_up = 0) with frames of that many samples.
  The oracle locks on these streams at frames of 9600 and 8192 samples and at no other that was tried.

  cap       streams whose one call holds 7, 8, 9 and 8 + 4 hits, on handles that log 8 a call (trig_cap): the run begins at
            in-call bit 60, so four slots come from one 64-bit ballot of sync_fin_wave and the rest, with the cap, from the next
  tuned     sync_cases' streams at a period-8 tuning (12000), a short-period one (9000) and a non-periodic one (12345), on
            ragged calls cut from each variant's own decision log
  fft       sync_cases' streams in FFT-acquire, and one *placed* stream per frame size: a call boundary can only sit on a frame
            boundary there, so the hits are moved instead -- to the in-call bits 0, 1, 63 / 64, 255 / 256 (9600) and the last bit
            of a call, each such call with a call of one frame directly before and behind it

A variant shifts the whole bit log by a constant (the bit clock settles differently): census() records that offset per (case,
variant), and the designed places hold after it.  census() is computed from the oracle alone, as sync_cases.census is:

    python tests/sync_handles.py --write        # -> tests/golden/sync_handles_census.json (data only)
"""
import functools
import json
import os
import sys

import numpy as np

import oracle_lib as O
import sync_cases as Y

CENSUS = os.path.join(Y.HERE, "golden", "sync_handles_census.json")


def TUNE(t):
    return ("tune", int(t))


def FFT(frame):
    return ("fft", int(frame))


# ---------------------------------------------------------------------------------------------------------------- variants
def carrier_of(variant):
    return variant[1] + 1200.0 if variant[0] == "tune" and variant[1] > 0 else 13200.0


def samples_of(variant):
    return Y.N if variant[0] == "tune" else (Y.N // variant[1]) * variant[1]


def oracle_config(variant):
    """(tuning, do_fft, do_up, samples a frame) of the reference demodulator of a variant"""
    return (variant[1], 0, 0, 1) if variant[0] == "tune" else (12000, 1, 0, variant[1])


def new_oracle(config):
    tuning, do_fft, do_up, frame = config
    return O.Bpsk(blen=4 * frame, tuning=tuning, do_fft=do_fft, do_up=do_up)


def input_of(case, variant):
    """int16 IQ of a case as the variant's demodulator is fed it"""
    return Y.stream_of(case, carrier_of(variant))[:2 * samples_of(variant)]


@functools.lru_cache(maxsize=None)
def bits_of(case, variant):
    o = new_oracle(oracle_config(variant))
    o.receive_i16(input_of(case, variant))
    b = o.bits().copy()
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def offset_of(case, variant):
    """d: bit j + LEAD + d of the variant's log is designed symbol j (over the part of the stream that holds full-register hits)"""
    if variant[0] == "tune" and variant[1] <= 0:
        return 0  # (garbage bits: nothing is designed there)
    bits, sym = bits_of(case, variant), Y.symbols_of(case)
    lo = 2000
    n = min(bits.size, Y.NSYM) - lo - 8
    found = [d for d in range(-3, 4) if np.array_equal(bits[lo + Y.LEAD + d:lo + Y.LEAD + d + n], sym[lo:lo + n])]
    assert len(found) == 1, (case[1], variant, found)
    return found[0]


@functools.lru_cache(maxsize=None)
def bit_ends(case, variant):
    """sync_cases.bit_ends through the variant's demodulator (tune variants: the boundaries of ragged calls come from it)"""
    o = new_oracle(oracle_config(variant))
    o.declog_enable(Y.NSYM + 64)
    o.receive_i16(input_of(case, variant))
    g, de = o.declog_pos()
    e = Y.DECIM * (g[de[:, 1] > 100.0] + 1)
    assert e.size == o.counters()["cntBit"]
    return e


@functools.lru_cache(maxsize=None)
def newbits(case, variant, calls):
    """the new bits of every call (calls: input samples each)"""
    o = new_oracle(oracle_config(variant))
    iq = input_of(case, variant)
    out, pos, nb = [], 0, 0
    for L in calls:
        o.receive_i16(iq[2 * pos:2 * (pos + L)])
        pos += L
        n = o.counters()["cntBit"]
        out.append(n - nb)
        nb = n
    assert pos == samples_of(variant)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- the cap family
CAP_BATCH = 160000                     # max_batch_samples of the cap handles: trig_cap is 8
CAP_INDEX = 60                         # the in-call bit of a run's first hit: 60 .. 63 in one ballot chunk, the rest in the next
CAP_PLACE = Y.slot(2)
CAP = [("cap", "cap_7", 603, (Y.image(CAP_PLACE, hold=7),)),
       ("cap", "cap_8", 611, (Y.image(CAP_PLACE, hold=8),)),
       ("cap", "cap_9", 602, (Y.image(CAP_PLACE, hold=9),)),
       ("cap", "cap_12", 604, (Y.image(CAP_PLACE, hold=8), Y.image(CAP_PLACE + 100, hold=4)))]
CAP_HITS = {"cap_7": 7, "cap_8": 8, "cap_9": 9, "cap_12": 12}
# rows of a cap handle, in order: the overflowing row has the row of exactly trig_cap hits directly behind it
CAP_ROWS = {9: ("cap_7", "cap_9", "cap_8", "threshold_first"), 12: ("cap_7", "cap_12", "cap_8", "threshold_first")}
CAP_VARIANT = TUNE(12000)


# ---------------------------------------------------------------------------------------------------------------- tuned variants
# (case, tuning): each tuning has a threshold case; the early frame sits at a period-8 and at a non-periodic tuning
TUNED = [("threshold_spread", 12000), ("order", 12000), ("early_frame", 12000),
         ("threshold_last", 9000), ("neighbours_a", 9000), ("early_45", 9000),
         ("threshold_first", 12345), ("frames_a", 12345), ("early_frame", 12345), ("neighbours_b", 11990)]
PASS_THROUGH = ("threshold_first", 0)  # a stream of the same handle whose tuner passes the samples through: no hits
TUNINGS = (12000, 9000, 12345, 11990)


# ---------------------------------------------------------------------------------------------------------------- FFT-acquire
FRAMES = (9600, 8192)
# frames a call; every call of three or four frames is one that a placed hit sits in, with one-frame calls around it
FFT_SCHEDULE = {9600: (46, 1, 3, 1, 3, 1, 3, 1, 3, 1, 4, 1, 7, 2, 53), 8192: (62, 1, 3, 1, 3, 1, 3, 1, 3, 1, 9, 2, 62)}
# (call of the schedule, in-call bit of the first hit or "last", hold)
PLACED_TARGETS = {9600: ((2, 0, 1), (4, 1, 1), (6, "last", 1), (8, 63, 2), (10, 255, 2)),
                  8192: ((2, 0, 1), (4, 1, 1), (6, "last", 1), (8, 63, 2))}
PLACED_SEED = {9600: 701, 8192: 702}
FFT_CASES = {9600: ("threshold_first", "threshold_last", "threshold_spread", "early_45", "early_frame", "neighbours_a", "order",
                    "frames_b", "placed_9600"),
             8192: ("threshold_first", "frames_a", "early_frame", "neighbours_b", "placed_8192")}


def fft_calls(frame):
    calls = tuple(f * frame for f in FFT_SCHEDULE[frame])
    assert sum(calls) == samples_of(FFT(frame))
    return calls


@functools.lru_cache(maxsize=None)
def placed(frame):
    """the placed case of a frame size.  Its filler alone goes through the oracle first, call by call: that log says which bit is
    the first of every call and how far the variant shifts the log, and the images go where the targets ask"""
    seed = PLACED_SEED[frame]
    probe = ("placed", "probe_%d" % frame, seed, ())
    nb = newbits(probe, FFT(frame), fft_calls(frame))
    first = np.concatenate([[0], np.cumsum(nb)])
    d = offset_of(probe, FFT(frame))
    events, at = [], []
    for call, idx, hold in PLACED_TARGETS[frame]:
        bit = int(first[call]) + (nb[call] - 1 if idx == "last" else idx)
        events.append(Y.image(bit - d, hold=hold))
        at += [bit + i for i in range(hold)]
    assert min(at) - Y.REG >= Y.SETTLE + Y.LEAD + 3          # every tap behind the symbols the bit clock may lose
    assert len({b % Y.STRIDE for b in at}) == len(at), at     # no two images share a tap
    return ("placed", "placed_%d" % frame, seed, tuple(events))


def case_of(name):
    if name in Y.BY_NAME:
        return Y.BY_NAME[name]
    if name.startswith("placed_"):
        return placed(int(name[7:]))
    return next(c for c in CAP if c[1] == name)


# ---------------------------------------------------------------------------------------------------------------- call schedules
@functools.lru_cache(maxsize=None)
def cap_calls():
    """calls of at most CAP_BATCH samples, one of which begins on bit CAP_PLACE - CAP_INDEX of every cap stream"""
    first = CAP_PLACE - CAP_INDEX
    lo = max(int(bit_ends(c, CAP_VARIANT)[first - 1]) for c in CAP)
    hi = min(int(bit_ends(c, CAP_VARIANT)[first]) for c in CAP)
    assert hi - lo >= 40, (lo, hi)
    return tuple(Y.capped(Y.calls_of([lo + 17]), CAP_BATCH))


@functools.lru_cache(maxsize=None)
def tuned_calls(variants=tuple(TUNED)):
    """sync_cases.seam_cuts over the targets of these (case, tuning) pairs, each cut placed by that variant's own decision log and
    moved by its offset; the union of all cuts, as ragged call lengths"""
    cuts = set()
    for name, tuning in variants:
        case, v = Y.BY_NAME[name], TUNE(tuning)
        e, d = bit_ends(case, v), offset_of(case, v)
        for tname, bit, k, zb, end, za in Y.TARGETS:
            if tname != name:
                continue
            if k is not None:
                first = bit + d - k
                lo, hi = int(e[first - 1]), int(e[first])
                assert hi - lo >= 60, (name, tuning, bit, lo, hi)
                c = lo + 3 + 2 * (bit % 7)
                cuts.add(c)
                if zb:
                    cuts.add(c + 21)
            if end is not None:
                lo, hi = int(e[end + d]), int(e[end + d + 1])
                assert hi - lo >= 60, (name, tuning, end, lo, hi)
                cuts.add(lo + 4)
                if za:
                    cuts.add(lo + 4 + 23)
    return tuple(Y.calls_of(sorted(cuts)))


# ---------------------------------------------------------------------------------------------------------------- the census
def entry(name, variant, schedules):
    """what the sync stage does on a case under a variant, from the oracle's bit log alone (sync_cases.census), the offset, the
    correlations at the designed places, and per schedule (call, in-call bit, new bits of the call) of every hit"""
    case = case_of(name)
    bits = bits_of(case, variant)
    r = Y.restate(bits)
    hits = [int(b) for b in r["hits"]]
    d = offset_of(case, variant)
    nonhit = r["corr"][r["corr"] < Y.THRESH]
    places = sorted(Y.designed_places(case)) if carrier_of(variant) != 13200.0 or variant[1] > 0 else []
    seen = {}
    for sname, calls in schedules.items():
        nb = newbits(case, variant, tuple(calls))
        seen[sname] = [list(Y.in_call_index(nb, b)) for b in hits]
    return dict(name=name, variant=list(variant), nbits=int(bits.size), offset=d, hits=hits, corr=[int(r["corr"][b]) for b in hits],
                designed=places, designed_corr=[int(r["corr"][p + d]) for p in places],
                max_nonhit=int(nonhit.max()), zeros=[max(0, Y.REG - 1 - b) for b in hits],
                rc=[int(O.fec_decode(Y.window(bits, b))[0]) for b in hits],
                rc_c0=[int(O.fec_decode(Y.window(bits, b, 0xC0))[0]) for b in hits], seen=seen)


@functools.lru_cache(maxsize=None)
def census():
    sched = {"cap": list(cap_calls()), "tuned": list(tuned_calls())}
    for f in FRAMES:
        sched["fft_%d" % f] = list(fft_calls(f))
    out = dict(schedules=sched, cap=[], tuned=[], fft=[])
    for c in CAP:
        out["cap"].append(entry(c[1], CAP_VARIANT, {"cap": sched["cap"]}))
    for name, t in TUNED + [PASS_THROUGH]:
        out["tuned"].append(entry(name, TUNE(t), {"tuned": sched["tuned"]}))
    for f in FRAMES:
        for name in FFT_CASES[f]:
            out["fft"].append(entry(name, FFT(f), {"fft_%d" % f: sched["fft_%d" % f]}))
    return out


def load():
    with open(CENSUS) as f:
        return json.load(f)


def text(c):
    return json.dumps(c, indent=None, separators=(",", ":")) + "\n"


if __name__ == "__main__":
    c = census()
    for kind in ("cap", "tuned", "fft"):
        for e in c[kind]:
            print("%-17s %-14s offset %2d  %s  largest non-hit %d" % (e["name"], e["variant"], e["offset"],
                                                                      " ".join("%d@%d" % p for p in zip(e["corr"], e["hits"])), e["max_nonhit"]))
            for s, seen in e["seen"].items():
                print("      %-9s in-call bits %s" % (s, [(k, i) for k, i, _ in seen]))
    for k, v in c["schedules"].items():
        print("%-9s %3d calls, longest %d samples" % (k, len(v), max(v)))
    if "--write" in sys.argv:
        with open(CENSUS, "w") as f:
            f.write(text(c))
