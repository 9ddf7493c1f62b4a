"""Engineered sync hits for the BPSK sync stage: what tests/golden/make_sync_census.py, tests/test_sync_cases_oracle.py and
tests/test_gpu_sync_cases.py share.

The sync stage (FUNcubeBPSKDemod.java:553-572) shifts every sliced bit into a 5200-entry register, correlates 65 taps at stride 80
with the sync vector, runs FECDecode where dmCorr >= 45 and keeps dmCorr, dmMaxCorr, cntFEC and cntDec.  The device does none of
this as a loop: k_sync_t (csrc/bpsk_tail.hip) correlates from a transposed LDS image with byte alignments and packed dot products,
the strided k_sync is its fallback, sync_fin_wave orders the hits with ballots and rebuilds dmMaxCorr from the last hit on, the tail
kernels carry the register from call to call, and the FEC kernels gather the 5200-byte window at whatever byte alignment the
trigger bit has.  The synthetic streams of oracle_lib hit at full strength once per frame, wherever that happens to fall; the
streams here put hits where those forms can go wrong, and census() counts, ON THE ORACLE'S BIT LOG ALONE, what they contain.

A designed stream is a sequence of +-1 symbols: seeded filler with *images* written over it.  An image is the sync vector (some
taps inverted) at 65 positions 80 apart; the correlation peaks on the bit that completes its 5200-symbol span.  Designed symbol j
comes out of the demodulator as bit j + LEAD (a few of the first SETTLE symbols can be lost while the bit clock settles; no tap is placed there).
All places below are BIT indices of the stream's log.

  threshold   images with 9, 10, 11, 12 inverted taps (correlation 47, 45, 43, 41) in three flip layouts -- the first taps, the
              last taps (with the 65th, which the packed dot product takes as a lone byte), spread taps
  early       streams that begin inside an image: the last m taps arrive, the others are the register's zeros, which must not
              count and must reach the decoder as 0x40 (:563); one of them a valid frame whose first 760 symbols are lost
  neighbours  taps held for 2, 3, 4 symbols (hits on consecutive bits); two images 1, 63, 64, 65, 255, 256, 257 bits apart
              (a ballot chunk of sync_fin_wave is 64 bits, a thread's stride in k_sync / k_sync_t 256)
  order       a 65 then a 45 in one call (dmMaxCorr must come down: :567 resets it), the reverse, and an inverted image (-65)
  frames      four valid frames whose hits fall on the four residues mod 4: the byte alignments of the decoders' window

Everything here is CPU only (numpy and the C oracle)."""
import functools
import json
import os

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS = os.path.join(HERE, "golden", "sync_census.json")

RATE, SPS, DECIM = 96000, 80, 10
REG, NTAP, STRIDE, THRESH = 5200, 65, 80, 45     # dmFECCorr's length, the taps, their distance, :560
LEAD = 2                                         # bit j + LEAD of the log is designed symbol j
SETTLE = 16                                      # ... from symbol SETTLE on
NSYM = 3 * REG                                   # every stream: three register lengths
N = NSYM * SPS                                   # input samples of a stream
AMP, NOISE_GAIN = 3000, 300
FUSED_MAX = 163840                               # the longest call k_sync_t orders itself (16384 down-sampled samples, S = 1)
CHUNK, THREAD_STRIDE = 64, 256                   # sync_fin_wave's ballot; the stride of a thread's outputs
FAMILIES = ("threshold", "early", "neighbours", "order", "frames")


def slot(i):
    """the places designed hits are put at: with the register full, 321 bits apart -- more than a thread's stride, and no two
    of them a multiple of 80 apart (images at such distances would share taps)"""
    return 5800 + 321 * i


# ---------------------------------------------------------------------------------------------------------------- generators
@functools.lru_cache(maxsize=None)
def sync_vector():
    v = O.bpsk_table(2).astype(np.int8)
    assert v.size == NTAP and set(np.unique(v)) == {-1, 1}
    return v


def flip_layout(layout, k):
    """which k taps of an image are inverted"""
    if layout == "first":
        return tuple(range(k))
    if layout == "last":
        return tuple(range(NTAP - k, NTAP))
    assert layout == "spread"
    return tuple((12 + (i * NTAP) // k) % NTAP for i in range(k))


def image(hit, flips=(), hold=1, sign=1):
    """taps that complete at bit `hit`, each held for `hold` symbols (hits on bits hit .. hit + hold - 1)"""
    return ("image", hit, tuple(flips), hold, sign)


def frame(hit, payload_seed):
    """a valid FEC frame (O.fec_encode) that completes at bit `hit`; what lies before the stream's first symbol is lost"""
    return ("frame", hit, payload_seed)


def payload_of(seed):
    return np.random.default_rng(seed).integers(0, 256, 256, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def symbols_of(case):
    """the designed +-1 symbols of a case (family, name, seed, events)"""
    _, _, seed, events = case
    sym = (np.random.default_rng(seed).integers(0, 2, NSYM).astype(np.int8) * 2 - 1).astype(np.int8)
    for ev in events:
        start = ev[1] - LEAD - (REG - 1)  # the symbol under tap 0
        if ev[0] == "image":
            _, _, flips, hold, sign = ev
            taps = sync_vector() * np.int8(sign)
            taps[list(flips)] *= -1
            for k in range(NTAP):
                for i in range(hold):
                    p = start + STRIDE * k + i
                    if 0 <= p < NSYM:
                        sym[p] = taps[k]
        else:
            fr = O.fec_encode(payload_of(ev[2])).astype(np.int8) * 2 - 1
            lo = max(0, -start)
            sym[start + lo:start + REG] = fr[lo:]
    sym.setflags(write=False)
    return sym


@functools.lru_cache(maxsize=None)
def stream_of(case, carrier_hz=13200.0):
    """int16 IQ [2 N] of a case: DBPSK at 1200 symbols/s on a 13 200 Hz carrier (or the one given), 96 kHz, a little noise"""
    sym = symbols_of(case)
    ds = O.synth_diffsign((sym > 0).astype(np.uint8), 1)
    ct, st = O.synth_tables(AMP)
    iq = O.synth_dbpsk(0, N, ds, SPS, 0, O.phase_inc_u32(carrier_hz, RATE), ct, st, NOISE_GAIN, O.mix64(0x53594E43 ^ (case[2] * 0x9E3779B1)))
    iq.setflags(write=False)
    return iq


# ---------------------------------------------------------------------------------------------------------------- the case list
# case = (family, name, seed, events); TARGETS (below) lists what the seam schedule aims at
def _threshold(layout, seed, first_slot):
    return ("threshold", "threshold_" + layout, seed,
            tuple(image(slot(first_slot + 3 * i), flip_layout(layout, k)) for i, k in enumerate((9, 10, 11, 12))))


def early_hit(m):
    """the bit on which an image completes of which only the last m taps were received"""
    return STRIDE * m + 40 + LEAD - 1


# a valid frame whose first 760 symbols (ten taps) fell before the stream began: with the register's zeros as 0x40 it decodes, as 0xc0
# it does not (a frame holds more 0 symbols than 1), so no decoder passes on the wrong mapping, in the trellis or in the error count
EARLY_FRAME_LOST = 760
EARLY_FRAME_HIT = REG - EARLY_FRAME_LOST + LEAD - 1
THRESHOLD = [_threshold("first", 101, 0), _threshold("last", 102, 1), _threshold("spread", 103, 2)]
EARLY = [("early", "early_45", 211, (image(early_hit(45)),)),
         ("early", "early_44", 202, (image(early_hit(44)),)),
         ("early", "early_46_flip", 203, (image(early_hit(46), (61,)),)),
         ("early", "early_47_flip", 214, (image(early_hit(47), (40,)),)),
         ("early", "early_frame", 205, (frame(EARLY_FRAME_HIT, 2051),))]
PAIR_SLOTS = {1: 29, 63: 13, 64: 15, 65: 19, 255: 20, 256: 21, 257: 22}
NEIGHBOURS = [("neighbours", "neighbours_a", 301,
               (image(slot(12), hold=2), image(slot(26), hold=3), image(slot(16), hold=4),
                image(slot(PAIR_SLOTS[1])), image(slot(PAIR_SLOTS[1]) + 1))),
              ("neighbours", "neighbours_b", 302,
               tuple(image(slot(PAIR_SLOTS[d]) + o) for d in (63, 64, 65, 255, 256, 257) for o in (0, d)))]
ORDER = [("order", "order", 401,
          (image(slot(17), sign=-1),
           image(slot(23)), image(slot(23) + 100, flip_layout("spread", 10)),
           image(slot(24), flip_layout("spread", 10)), image(slot(24) + 100)))]
FRAME_HITS = {"frames_a": (21 + REG + LEAD - 1, 5262 + REG + LEAD - 1), "frames_b": (303 + REG + LEAD - 1, 5904 + REG + LEAD - 1)}
FRAMES = [("frames", "frames_a", 501, tuple(frame(h, 5010 + i) for i, h in enumerate(FRAME_HITS["frames_a"]))),
          ("frames", "frames_b", 502, tuple(frame(h, 5020 + i) for i, h in enumerate(FRAME_HITS["frames_b"])))]
CASES = THRESHOLD + EARLY + NEIGHBOURS + ORDER + FRAMES
BY_NAME = {c[1]: c for c in CASES}


def family(name):
    return [c for c in CASES if c[0] == name]


def name_of(case):
    return case[1]


# ---------------------------------------------------------------------------------------------------------------- the census
def oracle_bits(iq):
    o = O.Bpsk(blen=4)
    o.receive_i16(iq)
    return o.bits().copy()


def correlate(bits):
    """dmCorr after every bit of a +-1 log, the register being zeros before the stream (:556-559)"""
    reg = np.concatenate([np.zeros(REG - 1, np.int32), np.asarray(bits, np.int32)])
    nb = len(bits)
    sv = sync_vector().astype(np.int32)
    corr = np.zeros(nb, np.int32)
    for n in range(NTAP):
        corr += reg[STRIDE * n:STRIDE * n + nb] * sv[n]
    return corr


def window(bits, b, zero_as=0x40):
    """the 5200 bytes FECDecode gets at a hit on bit b (:562-564: == 1 ? 0xc0 : 0x40, so the register's zeros arrive as 0x40);
    zero_as = 0xc0 is the wrong mapping, for telling the two apart"""
    w = np.zeros(REG, np.int8)
    lo = b + 1 - REG
    w[max(0, -lo):] = bits[max(0, lo):b + 1]
    return np.where(w == 1, 0xC0, np.where(w == 0, zero_as, 0x40)).astype(np.uint8)


def restate(bits):
    """:553-572 over a whole log, in numpy: per bit dmCorr, dmMaxCorr and cntFEC AFTER it, and the hits"""
    corr = correlate(bits)
    hit = corr >= THRESH
    at = np.flatnonzero(hit)
    mx = np.empty(len(bits), np.int32)
    edges = [0] + [int(b) for b in at] + [len(bits)]
    for k, (a, b) in enumerate(zip(edges, edges[1:])):
        seg = corr[a:b]
        if k == 0:  # dmMaxCorr starts at 0 (:123) and takes only larger values (:571)
            mx[a:b] = np.maximum(np.maximum.accumulate(seg), 0) if b > a else seg
        else:       # a hit sets it to 0 (:567) and then to the hit's own correlation (:571-572)
            mx[a:b] = np.maximum.accumulate(seg)
    return dict(corr=corr, hits=at, max=mx, fec=np.cumsum(hit))


def census(iq):
    """what the sync stage does on this input, from the oracle's bit log alone:
    hits / corr     the bits with dmCorr >= 45 and their correlations
    max_nonhit      the largest correlation below the threshold, and the smallest correlation of all
    zeros           per hit, how many bytes of the window are the register's zeros from before the stream
    align           per hit, (bit + 1) mod 4: the byte alignment of the decoders' window when the stream comes as one call
    rc / rc_c0      per hit, O.fec_decode of the window with the zeros as 0x40 (the reference) and as 0xc0 (wrong)"""
    bits = oracle_bits(iq)
    r = restate(bits)
    hits = [int(b) for b in r["hits"]]
    nonhit = r["corr"][r["corr"] < THRESH]
    return dict(nbits=int(len(bits)), hits=hits, corr=[int(r["corr"][b]) for b in hits], max_nonhit=int(nonhit.max()),
                min_corr=int(r["corr"].min()), zeros=[max(0, REG - 1 - b) for b in hits], align=[(b + 1) % 4 for b in hits],
                rc=[int(O.fec_decode(window(bits, b))[0]) for b in hits],
                rc_c0=[int(O.fec_decode(window(bits, b, 0xC0))[0]) for b in hits],
                final=[int(r["corr"][-1]), int(r["max"][-1]), int(r["fec"][-1])])


def designed_places(case):
    """the bits the case's events aim at"""
    return [ev[1] + i for ev in case[3] for i in range(ev[3] if ev[0] == "image" else 1)]


# ---------------------------------------------------------------------------------------------------------------- call schedules
def bit_ends(iq):
    """E[b]: the number of input samples after which bit b exists (the oracle's decision log; 9600 Hz sample g is complete with
    input sample 10 g + 9)"""
    o = O.Bpsk(blen=4)
    o.declog_enable(NSYM + 64)
    o.receive_i16(iq)
    g, de = o.declog_pos()
    e = DECIM * (g[de[:, 1] > 100.0] + 1)
    assert e.size == o.counters()["cntBit"]
    return e


def stepped(iq, calls):
    """the oracle fed call by call -> per call (new bits, counters, FEC results so far as (rc, bits before the trigger's end))"""
    o = O.Bpsk(blen=4)
    out, pos, nb = [], 0, 0
    for L in calls:
        o.receive_i16(iq[2 * pos:2 * (pos + L)])
        pos += L
        c = o.counters()
        out.append((c["cntBit"] - nb, c, [(rc, int(bi)) for rc, bi, _ in o.fec_results()]))
        nb = c["cntBit"]
    assert pos == N
    return out


def in_call_index(newbits, b):
    """(call, index in the call, new bits of the call) of bit b, from the per-call bit counts of a stream"""
    base = 0
    for k, n in enumerate(newbits):
        if b < base + n:
            return k, b - base, n
        base += n
    raise AssertionError(b)


# A target: the call that holds bit `bit` of `case` starts k bits before it (so the bit has index k in its call); zero_before
# puts a call of no new bit directly before that call (k = 0: directly before the hit); end = the bit that is to be the LAST of
# its call; zero_after puts a call of no new bit directly behind that.
def target(case, bit, k=None, zero_before=False, end=None, zero_after=False):
    return (case, bit, k, zero_before, end, zero_after)


T = slot
TARGETS = [
    # threshold: the 47s, 45s, 43s and 41s of the three layouts
    target("threshold_first", T(0), 0, zero_before=True), target("threshold_first", T(3), 64), target("threshold_first", T(6), 7, end=T(6)),
    target("threshold_first", T(9), 17),
    target("threshold_last", T(1), 1), target("threshold_last", T(4), 63, end=T(4), zero_after=True), target("threshold_last", T(7), 65),
    target("threshold_last", T(10), 9, end=T(10)),
    target("threshold_spread", T(2), 255), target("threshold_spread", T(5), 62), target("threshold_spread", T(8), 256),
    target("threshold_spread", T(11), 5),
    # early
    target("early_44", early_hit(44), 11, end=early_hit(44)), target("early_45", early_hit(45), 0, zero_before=True),
    target("early_46_flip", early_hit(46), 1, end=early_hit(46)), target("early_47_flip", early_hit(47), 62, end=early_hit(47), zero_after=True),
    target("early_frame", EARLY_FRAME_HIT, 63, end=EARLY_FRAME_HIT, zero_after=True),
    # neighbours: held taps across a ballot chunk's and a thread stride's edge; pairs from index 0 (the second at the offset)
    target("neighbours_a", T(12), 63), target("neighbours_a", T(26), 62), target("neighbours_a", T(16), 253),
    target("neighbours_a", T(29), 255, end=T(29) + 1, zero_after=True),
    target("neighbours_b", T(13), 0, zero_before=True), target("neighbours_b", T(15), 0), target("neighbours_b", T(19), 0, end=T(19) + 65, zero_after=True),
    target("neighbours_b", T(20), 0), target("neighbours_b", T(21), 0), target("neighbours_b", T(22), 1, end=T(22) + 257),
    # order
    target("order", T(17), 3, end=T(17)), target("order", T(23), 60, end=T(23) + 100, zero_after=True), target("order", T(24), 0, zero_before=True),
    # frames: the four alignments again, now as indices in a call
    target("frames_a", FRAME_HITS["frames_a"][0], 0, zero_before=True), target("frames_a", FRAME_HITS["frames_a"][1], 1, end=FRAME_HITS["frames_a"][1], zero_after=True),
    target("frames_b", FRAME_HITS["frames_b"][0], 2), target("frames_b", FRAME_HITS["frames_b"][1], 3),
]
SEAM_INDICES = (0, 1, 62, 63, 64, 65, 255, 256)   # in-call bit indices a hit must be seen at (and as the last bit of a call)
LENGTHS = tuple(range(1, 18)) + (79, 80, 81, 255, 256, 257)
# (case, hit, order of the lengths): calls of those many new bits up to and including the hit
LENGTH_ANCHORS = (("early_45", early_hit(45), -1), ("threshold_first", T(3), 1))


def calls_of(cuts):
    edges = [0] + sorted(set(int(c) for c in cuts)) + [N]
    assert edges[1] > 0 and edges[-2] < N
    return [b - a for a, b in zip(edges, edges[1:])]


def seam_cuts(ends, families=FAMILIES):
    """the call boundaries (input samples) of the targets of these families; ends = {case name: bit_ends}"""
    cuts = []
    for name, bit, k, zb, end, za in TARGETS:
        if BY_NAME[name][0] not in families:
            continue
        e = ends[name]
        if k is not None:
            first = bit - k  # the first new bit of the call: the boundary lies in [E[first - 1], E[first])
            lo, hi = int(e[first - 1]), int(e[first])
            assert hi - lo >= 60, (name, bit, lo, hi)
            c = lo + 3 + 2 * (bit % 7)  # (most call lengths are no multiple of the decimation)
            cuts.append(c)
            if zb:
                cuts.append(c + 21)
        if end is not None:
            lo, hi = int(e[end]), int(e[end + 1])
            assert hi - lo >= 60, (name, end, lo, hi)
            cuts.append(lo + 4)
            if za:
                cuts.append(lo + 4 + 23)
    assert len(set(cuts)) == len(cuts)
    return sorted(cuts)


def length_cuts(ends):
    cuts = []
    for name, hit, order in LENGTH_ANCHORS:
        e = ends[name]
        b = hit
        cuts.append(int(e[b]) + 5)  # the hit is the last bit of its call
        for n in LENGTHS[::order]:
            b -= n
            cuts.append(int(e[b]) + 5)
    return sorted(cuts)


def capped(calls, most=160000):
    """no call longer than `most` samples: longer ones are cut into pieces"""
    out = []
    for L in calls:
        while L > most:
            out.append(most)
            L -= most
        out.append(L)
    return out


def trig_cap(max_batch_samples):
    """the hits a stream can log in one call of a handle created for calls of that many samples (csrc/bpsk_handle.hip)"""
    max_bits = (max_batch_samples // DECIM + 2) // 4 + 16
    return max(8, max_bits // 2600 + 4)


def fallback_batch_samples():
    """the smallest max_batch_samples, rounded up to a multiple of 2^20, at which a handle's transposed sync image outgrows 150 KiB
    of LDS and the handle takes the strided k_sync (sync_t_lds / sync_t_applies in csrc/bpsk_tail.hip, max_bits as above)"""
    def lds(max_bits):
        rs = ((REG + max_bits + 79) // 80 + 72 + 3) & ~3
        if (rs // 4) % 2 == 0:
            rs += 4
        return 80 * rs + 16
    n = 1 << 20
    while lds((n // DECIM + 2) // 4 + 16) <= 150 * 1024:
        n += 1 << 20
    return n


# ---------------------------------------------------------------------------------------------------------------- the fixture
@functools.lru_cache(maxsize=None)
def all_ends():
    return {c[1]: bit_ends(stream_of(c)) for c in CASES}


def summary():
    """the JSON's content: the census of every case, and the schedules (call lengths in input samples)"""
    ends = all_ends()
    sched = {"seams": calls_of(seam_cuts(ends)), "lengths": calls_of(length_cuts(ends))}
    for f in FAMILIES:
        sched["fused_" + f] = capped(calls_of(seam_cuts(ends, (f,))))
    return dict(cases=[dict(name=c[1], family=c[0], **census(stream_of(c))) for c in CASES], schedules=sched)


def load():
    with open(CENSUS) as f:
        return json.load(f)


def schedule(name):
    return [N] if name == "one_call" else load()["schedules"][name]
