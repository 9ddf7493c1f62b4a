"""Edge cases of the tune-mode front ends and matched filters (csrc/bpsk_fm.hip, bpsk_fm_f32.hip, bpsk_front.hip, bpsk_front_reg.hip,
bpsk_chan.hip): what tests/test_fm_cases_oracle.py and tests/test_gpu_fm_cases.py share.  CPU only: numpy and, for the signals,
the C oracle's synthesiser; no library call.

geometry(rate, n_in, L, kind) restates, from the kernels' header comments and FUNcubeBPSKDemod.java's decimator (an output at every
sample n with n % D == D - 1), what a call of L samples must be when the stream has taken n_in samples before it:

  every kind   D, R, dsCnt, first_out, g_first, nds, a, tile0
  "fm"         k_fm / k_fm_f32: tiles of TILE = 65 * 62 = 4030 outputs from tile0, the matched filter's block boundary (g == 64 mod 65)
               at or before g_first, so the first tile begins a = (g_first - 64) mod 65 outputs before the call: ntiles, first / last
               (this call's outputs in the first and the last tile), small (nds <= 512: the one-output-per-thread matched half),
               halo_tiles (the tiles that own one of the call's last 64 outputs, which are saved for the next call), splice
               (nds < 64: the old halo's tail is kept in front of them), inherit (L < 26: the next input history keeps samples of
               the old one), overlap (the two 256-sample edge images: 1 share input samples, L < 256; 2 the end image reaches
               back past sample 0, L < 128)
  "split"      k_front_reg / k_front, k_matched, k_dm_history: mtiles (k_matched's tiles of 4160 from the same tile0), mlast,
               waves (the front end's wave tiles of 64 * R outputs)
  "chan"       k_chan_front + k_matched: wgs (workgroups of 256 outputs), mtiles, mlast

The lists are in OUTPUTS (9600 Hz samples), so they are the same lists at /4, /5, /10 and /20; a schedule turns them into sample
counts with the decimation phases it rotates through.  Where a case needs an alignment a or a phase first_out, the call before it is
sized by reach().  A schedule is at most BUDGET outputs a stream (133 000 samples at /10).

  seam_cases         a in SEAM_A x k in SEAM_K x delta in SEAM_DELTA: nds = 4030 k - a + delta, the last tile then holds delta outputs
                     (1 .. 5 straddle a job of R; 63 / 64 / 65: the saved halo inside one tile, exactly one tile, across two); then a
                     call of 1, 63, 64 or 65 outputs (SMALL half, splice), then a two-tile call (batch half)
  split_seam_cases   the same around k_matched's 4160 (delta -1, 0, 1) and the front end's wave tiles of 64 R
  walk_schedules     calls of 66 outputs (SMALL half) and of 513 (batch half): a advances by 1 and by 58 a call, 65 calls take it
                     through 0 .. 64; the lengths are no multiples of D, the decimation phase rotates
  boundary_schedule  nds = 511, 512, 513 at a = 0 and 64
  short_schedules    L in SHORT_L as a stream's first call, after a long call, after the same and after another short call; x DCS
  zero_schedule      runs of calls without any output, then a long call

`python tests/fm_cases.py --write` writes tests/golden/fm_census.json (data only): what the lists contain, class by class, which
tests/test_fm_cases_oracle.py recomputes and holds the conditions against."""
import collections
import functools
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS = os.path.join(HERE, "golden", "fm_census.json")

FM_NB, FM_NT, FM_THREADS, FM_EDGE = 62, 4094, 512, 128
BLOCK, HALO, HIST = 65, 64, 26
TILE = BLOCK * FM_NB   # 4030
MTILE = 4160           # k_matched: 64 lanes x 65
CHAN_WG = 256
S = 3                  # streams a handle
BUDGET = 13300         # outputs a stream and schedule
RATES = (96000, 192000, 48000, 44100)
# (rate, tuning): the 8-phase form, period 4, no tuner twice, /20, /5, /4 (11 025 Hz at 44.1 kHz: a quarter turn a sample, period 4)
CONFIGS = ((96000, 12000), (96000, 24000), (96000, 0), (96000, -5000), (192000, 24000), (48000, 12000), (44100, 11025))
DCS = ((0, 0), (1234, -4321), (40000, -40000), (-32768, 32767))  # off, ordinary, wrapping twice

Call = collections.namedtuple("Call", "L role why")
Schedule = collections.namedtuple("Schedule", "name rate calls ic qc idx")


def decim(rate):
    return rate // 9600


def job(rate):
    """R: outputs a job of k_fm (and a lane of k_front_reg)"""
    return 5 if decim(rate) == 4 else 4


# ---------------------------------------------------------------------------------------------------------------- geometry
def geometry(rate, n_in, L, kind):
    D, R = decim(rate), job(rate)
    dsCnt = n_in % D
    first_out = D - 1 - dsCnt
    g_first = n_in // D
    nds = (n_in + L) // D - g_first
    a = (g_first - HALO) % BLOCK
    g = dict(D=D, R=R, dsCnt=dsCnt, first_out=first_out, g_first=g_first, nds=nds, a=a, tile0=g_first - a)
    if kind == "fm":
        ntiles = -(-(a + nds) // TILE) if nds > 0 else 0
        g.update(ntiles=ntiles, first=min(nds, TILE - a), last=a + nds - (ntiles - 1) * TILE if ntiles > 1 else nds,
                 small=0 < nds <= FM_THREADS, splice=0 < nds < HALO,
                 halo_tiles=sorted({(a + j) // TILE for j in (max(nds - HALO, 0), nds - 1)}) if nds > 0 else [],
                 inherit=L < HIST, overlap=2 if L < FM_EDGE else 1 if L < 2 * FM_EDGE else 0)
        assert not g["small"] or ntiles == 1
    elif kind == "split":
        mtiles = -(-(a + nds) // MTILE) if nds > 0 else 0
        g.update(mtiles=mtiles, mlast=a + nds - (mtiles - 1) * MTILE if mtiles > 1 else nds, waves=-(-nds // (64 * R)))
    elif kind == "chan":
        mtiles = -(-(a + nds) // MTILE) if nds > 0 else 0
        g.update(mtiles=mtiles, mlast=a + nds - (mtiles - 1) * MTILE if mtiles > 1 else nds, wgs=-(-nds // CHAN_WG))
    else:
        raise ValueError(kind)
    return g


def tuner_period(rate, tuning):
    """samples after which the tuner's table index repeats; 0: no tuner (FUNcubeBPSKDemod.java:388 mixes for tuPhase > 0 only)"""
    return rate // math.gcd(rate, tuning) if tuning > 0 else 0


def fm_takes(rate, tuning, n_in, L):
    """does the fused kernel take this call of a handle tuned from its first sample?  With a tuner it needs the table index to be
    periodic over every sample of the call AND the 26 history samples before it (bpsk_sched.hip, compute_schedule); only a stream's
    first call is excused the history, which is zeros then.  The places before the stream carry index 0, which is also what the
    period asks of sample -1 (the tuner steps, then looks up: sample n has phase (n + 1) inc, sample -1 phase 0) and of no other.
    So a call that begins 1 .. 24 samples into the stream takes the three-kernel path, and so does one too short to show a period."""
    p = tuner_period(rate, tuning)
    if p == 0:
        return True
    if 0 < n_in < HIST - 1:
        return False
    return (L if n_in == 0 else L + HIST) > p


def reach(rate, n_in, a, first_out, min_out=1):
    """length of a call from n_in after which the stream is at alignment a and decimation phase first_out; at least min_out outputs"""
    D = decim(rate)
    g = n_in // D + min_out
    while (g - HALO) % BLOCK != a:
        g += 1
    return g * D + (D - 1 - first_out) - n_in


def outputs(rate, n_in, nds, ds_next):
    """length of a call from n_in of exactly nds outputs that leaves dsCnt = ds_next"""
    D = decim(rate)
    L = (n_in // D + nds) * D + ds_next % D - n_in
    assert L > 0 and geometry(rate, n_in, L, "fm")["nds"] == nds
    return L


class _Builder:
    def __init__(self, rate):
        self.rate, self.n, self.calls = rate, 0, []

    def add(self, L, role, why):
        self.calls.append(Call(int(L), role, why))
        self.n += L

    def reach(self, a, first_out, min_out, why):
        self.add(reach(self.rate, self.n, a, first_out, min_out), "prep", why)

    def out(self, nds, ds_next, role, why):
        self.add(outputs(self.rate, self.n, nds, ds_next), role, why)

    def done(self, name, idx, dc=(0, 0)):
        total = sum(c.L for c in self.calls)
        assert total // decim(self.rate) <= BUDGET, (name, total)
        return Schedule(name, self.rate, tuple(self.calls), dc[0], dc[1], idx)


# ---------------------------------------------------------------------------------------------------------------- seams
SEAM_A = (0, 1, 32, 63, 64)
SEAM_K = (1, 2)
SEAM_DELTA = (-1, 0, 1, 2, 3, 4, 5, 63, 64, 65)
FOLLOW = (1, 63, 64, 65)          # outputs of the call behind a seam call, rotated over the cases
TWO_TILE_LAST = (1, 4, 65, 777)   # outputs in the second tile of the two-tile call behind it, rotated
SPLIT_DELTA = (-1, 0, 1)
SPLIT_WAVES = (1, 2, 16)          # front-end wave tiles: nds = 64 R m + delta


def _phases(rate, idx):
    D = decim(rate)
    return (0, D - 1, D // 2)[idx % 3]


def _rot(idx):
    """a rotation that takes every delta of a cross (idx = 10 x + delta's place) through all four followers"""
    return (idx + idx // 10) % 4


def _seam_schedule(rate, name, idx, a, nds, why):
    b = _Builder(rate)
    b.reach(a, _phases(rate, idx), 66 + idx % 61, "to a = %d at decimation phase %d" % (a, _phases(rate, idx)))
    b.out(nds, 3 * idx + 1, "seam", why)
    m = FOLLOW[_rot(idx)]
    b.out(m, 7 * idx + 2, "follow", "%d outputs behind the seam: the halo through the SMALL half%s" % (m, ", spliced" if m < HALO else ""))
    a2 = geometry(rate, b.n, 1, "fm")["a"]
    b.out(TILE - a2 + TWO_TILE_LAST[(_rot(idx) + idx // 20) % 4], 5 * idx + 3, "two", "two tiles: the short call's halo through the batch half")
    return b.done(name, idx, DCS[(idx + idx // 10) % 2])


@functools.lru_cache(maxsize=None)
def seam_cases(rate):
    """((a, k, delta), schedule) for the cross SEAM_A x SEAM_K x SEAM_DELTA"""
    out, idx = [], 0
    for a in SEAM_A:
        for k in SEAM_K:
            for d in SEAM_DELTA:
                why = "nds = %d * %d - %d %+d: the last tile holds %d" % (TILE, k, a, d, d if d >= 1 else TILE + d)
                out.append(((a, k, d), _seam_schedule(rate, "seam-a%d-k%d-d%d" % (a, k, d), idx, a, TILE * k - a + d, why)))
                idx += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def split_seam_cases(rate):
    """((kind, a or m, delta), schedule): k_matched's tile seams at 4160 - a + delta, the front end's wave tiles at 64 R m + delta"""
    out, idx, R = [], 0, job(rate)
    for a in SEAM_A:
        for d in SPLIT_DELTA:
            why = "nds = %d - %d %+d: k_matched's last tile holds %d" % (MTILE, a, d, d if d >= 1 else MTILE + d)
            out.append((("matched", a, d), _seam_schedule(rate, "mseam-a%d-d%d" % (a, d), idx, a, MTILE - a + d, why)))
            idx += 1
    for m in SPLIT_WAVES:
        for d in SPLIT_DELTA:
            why = "nds = 64 * %d * %d %+d: the front end's last wave tile" % (R, m, d)
            out.append((("front", m, d), _seam_schedule(rate, "fseam-m%d-d%d" % (m, d), idx, SEAM_A[idx % 5], 64 * R * m + d, why)))
            idx += 1
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- alignment walk
WALK_SMALL, WALK_BATCH, WALK_CALLS, WALK_CHUNK = 66, 513, 65, 22


@functools.lru_cache(maxsize=None)
def walk_schedules(rate):
    """[walk of 66] + three chunks of the walk of 513 (each reaches its first alignment with a call of its own)"""
    D = decim(rate)
    b = _Builder(rate)
    for i in range(WALK_CALLS):
        b.out(WALK_SMALL, b.n % D + 3, "walk", "66 outputs: a moves on by one")
    b.out(131, 0, "flush", "takes the last call's halo")
    out = [b.done("walk-66", 0)]
    a = 1  # (a stream's first call: g_first = 0)
    for c in range(-(-WALK_CALLS // WALK_CHUNK)):
        b = _Builder(rate)
        if c:
            b.reach(a, (3 * c) % D, 66, "to a = %d, where the chunk before ended" % a)
        for i in range(c * WALK_CHUNK, min((c + 1) * WALK_CHUNK, WALK_CALLS)):
            assert geometry(rate, b.n, 1, "fm")["a"] == a
            b.out(WALK_BATCH, b.n % D + 3, "walk", "513 outputs: a moves on by 58")
            a = (a + WALK_BATCH) % BLOCK
        b.out(131, 0, "flush", "takes the last call's halo")
        out.append(b.done("walk-513-%d" % c, 1 + c, DCS[1] if c == 1 else DCS[0]))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- form boundary
BOUNDARY_NDS = (511, 512, 513)
BOUNDARY_A = (0, 64)


@functools.lru_cache(maxsize=None)
def boundary_schedule(rate):
    b, i = _Builder(rate), 0
    for a in BOUNDARY_A:
        for nds in BOUNDARY_NDS:
            b.reach(a, _phases(rate, i), 66, "to a = %d" % a)
            b.out(nds, 3 * i + 2, "boundary", "%d outputs at a = %d: %s" % (nds, a, "SMALL" if nds <= FM_THREADS else "the batch kernel"))
            i += 1
    b.out(131, 0, "flush", "takes the last call's halo")
    return b.done("boundary", 0, DCS[1])


# ---------------------------------------------------------------------------------------------------------------- short calls
SHORT_L = ((1, "one sample"), (2, "two samples: no output in most calls"), (25, "one short of the 26-sample history"), (26, "exactly the history"),
           (27, "the history and one"), (56, "one short of a /10 job's window of 57"), (57, "a /10 job's window"), (58, "a window and one"),
           (60, "the window's fifteen quads"), (61, "the quads and one"), (87, "a /20 job's window"),
           (88, "its 22 quads"), (89, "the quads and one"), (127, "one short of an edge image's half"), (128, "FM_EDGE: the images meet"),
           (129, "FM_EDGE and one"), (255, "one short of two image halves"), (256, "the images touch and share nothing"),
           (257, "one sample in neither image"))
SHORT_LIST = tuple(L for L, _ in SHORT_L)
LONG = 3001


@functools.lru_cache(maxsize=None)
def short_schedules(rate, dc):
    """one schedule an entry of SHORT_L: first call, after itself, after a long call, after another short length"""
    out = []
    for i, (L, why) in enumerate(SHORT_L):
        other = SHORT_LIST[(i + 7) % len(SHORT_LIST)]
        b = _Builder(rate)
        b.add(L, "short-first", "a stream's first call; " + why)
        b.add(L, "short-short", "after a short call")
        b.add(LONG + 2 * i, "long", "a long call")
        b.add(L, "short-long", "after a long call")
        b.add(other, "short-other", "another short length")
        b.add(L, "short-short", "after another short call")
        b.add(1207 + i, "flush", "takes what the short calls left")
        out.append(b.done("short-%d-dc%d" % (L, DCS.index(dc)), i, dc))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def zero_schedule(rate):
    b = _Builder(rate)
    for L in (1, 1, 1):
        b.add(L, "zero", "three samples in three calls: no output at any rate")
    for L in (2, 1, 1, 2, 1, 3, 1):
        b.add(L, "tiny", "shorter than D")
    b.add(LONG, "long", "a long call behind them")
    for L in (1, 1, 2):
        b.add(L, "tiny", "shorter than D, behind a long call")
    b.add(1207, "flush", "a long call behind them")
    return b.done("zero", 0, DCS[1])


def all_schedules(rate):
    """every schedule of the fused path's lists at one rate"""
    out = [s for _, s in seam_cases(rate)] + list(walk_schedules(rate)) + [boundary_schedule(rate), zero_schedule(rate)]
    for dc in DCS:
        out += list(short_schedules(rate, dc))
    return out


def walk(sch, kind="fm"):
    """[(call, n_in, geometry)] of a schedule"""
    out, n = [], 0
    for c in sch.calls:
        out.append((c, n, geometry(sch.rate, n, c.L, kind)))
        n += c.L
    return out


# ---------------------------------------------------------------------------------------------------------------- signals
NBASE = BUDGET * 20 + 30000


@functools.lru_cache(maxsize=8)
def base_streams(rate, tuning):
    """int16 IQ [S][2 * NBASE]: a DBPSK signal 1200 Hz above the tuning with noise; full-scale uniform noise; I = n mod 65536 - 32768
    with a fixed permutation of it in Q (a misplaced or missing sample cannot cancel).  No silence: zeros hide these errors."""
    import oracle_lib as O
    rng = np.random.default_rng(rate + 7 * abs(tuning) + 1)
    raws = np.empty((S, 2 * NBASE), np.int16)
    raws[0] = O.make_dbpsk_stream(4243, 3, NBASE, rate=rate, carrier_hz=max(tuning, 0) + 1200.0, noise_sigma=600.0)[0]
    raws[1] = rng.integers(-32768, 32768, 2 * NBASE).astype(np.int16)
    raws[2, 0::2] = (np.arange(NBASE, dtype=np.int64) % 65536 - 32768).astype(np.int16)
    raws[2, 1::2] = np.tile(rng.permutation(np.arange(-32768, 32768, dtype=np.int32)).astype(np.int16), NBASE // 65536 + 1)[:NBASE]
    raws.setflags(write=False)
    return raws


def streams(rate, tuning, sch):
    """int16 IQ [S][2 * total] of a schedule: the base streams from an offset of the schedule's own"""
    total = sum(c.L for c in sch.calls)
    off = (1009 * sch.idx + 17 * len(sch.calls)) % 20000
    assert off + total <= NBASE
    return np.ascontiguousarray(base_streams(rate, tuning)[:, 2 * off:2 * (off + total)])


# ---------------------------------------------------------------------------------------------------------------- the census
def census(rate):
    """what the lists of one rate contain, class by class (geometry alone)"""
    tiles = collections.Counter()
    last = collections.Counter()
    a_small, a_batch = set(), set()
    c = collections.Counter()
    follow = collections.Counter()
    phases = set()
    for sch in all_schedules(rate):
        prev = None
        for call, n_in, g in walk(sch):
            c["calls"] += 1
            if g["nds"] == 0:
                c["zero_output_calls"] += 1
                c["zero_output_calls_in_a_row"] += int(prev is not None and prev["nds"] == 0)
            else:
                tiles[g["ntiles"]] += 1
                (a_small if g["small"] else a_batch).add(g["a"])
                if g["ntiles"] > 1 and (g["last"] <= 5 or 63 <= g["last"] <= 65):
                    last[g["last"]] += 1
                c["splices"] += int(g["splice"])
                c["halo_from_two_tiles"] += int(len(g["halo_tiles"]) == 2)
                c["halo_exactly_the_last_tile"] += int(g["ntiles"] > 1 and g["last"] == HALO)
                c["small_calls"] += int(g["small"])
                c["inherit"] += int(g["inherit"])
                c["overlap_%d" % g["overlap"]] += 1
                c["splice_behind_a_splice"] += int(g["splice"] and prev is not None and 0 < prev["nds"] < HALO)
            if call.role == "seam":
                phases.add(g["first_out"])
            if call.role == "follow":
                follow[g["nds"]] += 1
            prev = g
        c["samples"] += sum(x.L for x in sch.calls)
        c["schedules"] += 1
    return dict(rate=rate, D=decim(rate), counts=dict(sorted(c.items())), tiles={str(k): v for k, v in sorted(tiles.items())},
                last_tile_fill={str(k): v for k, v in sorted(last.items())}, alignments_small=len(a_small), alignments_batch=len(a_batch),
                follow={str(k): v for k, v in sorted(follow.items())}, seam_phases=sorted(phases),
                walk_small=sorted({g["a"] for call, _, g in walk(walk_schedules(rate)[0]) if call.role == "walk"}) == list(range(BLOCK)),
                walk_batch=sorted({g["a"] for s in walk_schedules(rate)[1:] for call, _, g in walk(s) if call.role == "walk"}) == list(range(BLOCK)),
                split=dict(collections.Counter("%s:%d" % (key[0], geometry(rate, n_in, call.L, "split")["mtiles"])
                                               for key, s in split_seam_cases(rate) for call, n_in, _ in walk(s) if call.role == "seam")))


def summary():
    return dict(constants=dict(TILE=TILE, FM_NT=FM_NT, FM_THREADS=FM_THREADS, FM_EDGE=FM_EDGE, MTILE=MTILE, CHAN_WG=CHAN_WG, BUDGET=BUDGET),
                configs=[list(c) for c in CONFIGS], rates=[census(rate) for rate in RATES])


def dumps(s):
    return json.dumps(s, indent=None, separators=(",", ":")) + "\n"


def load():
    with open(CENSUS) as f:
        return json.load(f)


def main(argv):
    """print the census; `--write [PATH]` writes it (to tests/golden/fm_census.json by default)"""
    s = summary()
    for r in s["rates"]:
        print(r)
    if "--write" in argv:
        rest = argv[argv.index("--write") + 1:]
        path = rest[0] if rest else CENSUS
        with open(path, "w") as f:
            f.write(dumps(s))
        print("wrote", path)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    main(sys.argv[1:])
