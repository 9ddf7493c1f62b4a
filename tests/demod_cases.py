"""Edge cases of the demod.java AM/FM chain (csrc/demod.hip, csrc/demod_chan.hip): what tests/test_demod_cases_oracle.py and
tests/test_gpu_demod_cases.py share.  CPU only: numpy and, for the census, the C oracle (oracle_lib.Demod); no library call.

The kernels cut a frame into tiles of DTILE = 2048 samples, read DHALO = 21 samples of halo before each tile, give every thread
DPER = 8 consecutive samples, keep a frame of at most FUSED_TILES = 5 tiles in one workgroup (k_demod_fused<*, NT> /
k_demod_chan<*, NT>) and send every other frame, and every AM frame of an ordinary handle, through k_demod_front + k_demod_out
(chunks of OUT_CHUNK = 1024 samples); k_demod_mean walks the AM running mean in blocks of MEAN_BLOCK = 64 frames by 64 columns.
Every list below is made of the edges of that geometry, and geometry() says, from (n, mode, fused_ok), what a case must launch.

  SIZES          frame sizes, each with its reason: tiny frames (shorter than a thread's run, than the halo, exactly 8 / 21 / 22),
                 k_demod_out's chunk edges, last-tile lengths 1, 7, 8, 9, 20, 21, 22 behind a full tile, two tiles exact and three
                 with a 1-sample tail, the NT = 4 instantiation, five tiles
  calls_of(n)    frames per call: [2, 1, 3] from 21 samples on; below that a schedule whose calls are shorter than 21 samples,
                 exactly 21 where n divides 21, and longer, two of the short ones in a row (k_demod_state then builds a history
                 from one that was itself partly inherited)
  grid_signal    the suite's fm_am_signal with one carrier per stream
  planted        int16 frames that alternate loud (about 30000) and quiet (at most 1000), each quiet frame with ONE sample of
                 magnitude 20000 at an edge of the tile geometry: a frame maximum taken over a few samples too many (the padded
                 lanes of a ragged tile, the neighbour frame, the next stream's row) or too few changes the frame's AGC factor
  runout         frames of a loud tone at half the sample rate, which the band-pass removes: past a ragged tile's last sample the
                 filter runs out over zeros and its partial sums are far larger than anything inside the frame
  MEAN_BLOCKS    (frame size, streams, frames per call) for k_demod_mean: 63, 64, 65, 129 and 200 frames in all, frame sizes
                 with vector chunks then a ragged chunk (100, 68) and scalar chunks throughout (130)
  SWITCH_CALLS   eight calls at n = 2049 on one live handle: filter off and on again over a stale ring, mixer off and on again,
                 FM -> RAW -> AM -> FM, AGC toggled, a weights() call in between

`python tests/demod_cases.py --write` writes tests/golden/demod_census.json (data only): what the oracle alone says about these
inputs, which tests/test_demod_cases_oracle.py recomputes and holds the conditions against."""
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS = os.path.join(HERE, "golden", "demod_census.json")

RATE = 96000
DTILE, DHALO, DPER, FUSED_TILES, OUT_CHUNK, MEAN_BLOCK = 2048, 21, 8, 5, 1024, 64
OFF, RAW, AM, NFM, WFM = range(5)
MODES = (OFF, RAW, AM, NFM, WFM)
BAND = (3000, 11000)
S = 3            # streams: row offsets s * L are no multiples of 4 for odd L (the scalar store paths)
IC, QC = 37, -1200
f32 = np.float32

# ---------------------------------------------------------------------------------------------------------------- frame sizes
TINY = ((1, "one sample: every frame of a call but those past the 21st reaches into the history"),
        (2, "shorter than a thread's run of 8"),
        (3, "odd, divides 21: a call of exactly the halo"),
        (7, "one short of a thread's run, divides 21"),
        (8, "exactly a thread's run"),
        (9, "a thread's run and one: thread 1 holds one sample"),
        (20, "one short of the halo"),
        (21, "exactly the halo: frame 1 is the first on the fast-load branch"),
        (22, "the halo and one"),
        (63, "one short of a wave's 64 columns in k_demod_mean"),
        (64, "exactly one vector chunk in k_demod_mean"),
        (65, "64 and one: scalar chunks, the second of one column"),
        (100, "vector chunk then a ragged chunk of 36 in k_demod_mean"))
OUT_EDGES = ((1023, "one short of a k_demod_out chunk"), (1024, "exactly one k_demod_out chunk"),
             (1025, "a k_demod_out chunk and one sample: a second workgroup for it"))
TILE_EDGES = ((2047, "one short of a tile"), (2048, "exactly a tile"), (2049, "last tile of 1 sample"),
              (2055, "last tile of 7"), (2056, "last tile of 8: one whole thread"), (2057, "last tile of 9"),
              (2068, "last tile of 20"), (2069, "last tile of 21: the halo"), (2070, "last tile of 22"))
TWO_THREE = ((4096, "two tiles exact"), (4097, "three tiles, the last of 1 sample (chained, odd tile start)"))
FOUR = ((6145, "NT = 4, last tile of 1"), (8191, "NT = 4, last tile one short"), (8192, "NT = 4, four full tiles"))
FIVE_TILES = ((8193, "NT = 5, last tile of 1"), (10239, "NT = 5, last tile one short"))
SIZES = TINY + OUT_EDGES + TILE_EDGES + TWO_THREE + FOUR + FIVE_TILES
SIZE_LIST = tuple(n for n, _ in SIZES)
TILE_EDGE_SIZES = tuple(n for n, _ in TILE_EDGES)
LAST_TILE_LENGTHS = (1, 7, 8, 9, 20, 21, 22)
# (dofir, dodwn, doagc)
SWITCHES = ((1, 1, 1), (0, 1, 0))
SWITCHES_AT_TILE_EDGES = SWITCHES + ((1, 0, 1), (0, 0, 1))


def switches_of(n):
    return SWITCHES_AT_TILE_EDGES if n in TILE_EDGE_SIZES else SWITCHES


def geometry(n, mode, fused_ok=True):
    """what an ORDINARY handle must launch for frames of n samples in `mode`:
    fused       k_demod_fused<*, tiles> alone (else k_demod_front + k_demod_out)
    tiles       tiles per frame
    last        length of the frame's last tile
    mean        (vector branch runs, ragged / scalar branch runs) of k_demod_mean; (False, False) outside AM
    chunks      k_demod_out workgroups per frame (0 when fused)
    A channel handle ignores fused_ok: k_demod_chan<*, tiles> up to five tiles, its AM channels through k_demod_mean."""
    tiles = (n + DTILE - 1) // DTILE
    fused = bool(fused_ok) and mode != AM and tiles <= FUSED_TILES
    vector = mode == AM and n % 4 == 0 and n >= MEAN_BLOCK  # (a call is whole frames: L % 4 == 0 with n % 4 == 0)
    ragged = mode == AM and (n % 4 != 0 or n % MEAN_BLOCK != 0)
    return dict(fused=fused, tiles=tiles, last=n - (tiles - 1) * DTILE, mean=(vector, ragged),
                chunks=0 if fused else (n + OUT_CHUNK - 1) // OUT_CHUNK)


def mean_blocks(frames_total):
    """(full 64-frame blocks, rows of the partial block behind them) of one k_demod_mean launch"""
    return frames_total // MEAN_BLOCK, frames_total % MEAN_BLOCK


def coverage():
    """the classes SIZES and MEAN_BLOCKS reach"""
    nt = sorted({geometry(n, NFM)["tiles"] for n in SIZE_LIST})
    last_behind_full = sorted({geometry(n, NFM)["last"] for n in SIZE_LIST if geometry(n, NFM)["tiles"] > 1} & set(LAST_TILE_LENGTHS))
    forms = {geometry(n, AM)["mean"] for n in SIZE_LIST + tuple(m[0] for m in MEAN_BLOCKS)}
    names = {(True, False): "vector", (False, True): "scalar", (True, True): "vector+ragged"}
    chained_unaligned = sorted(n for n in SIZE_LIST if geometry(n, NFM)["tiles"] > 1 and n % 2 and geometry(n, NFM)["last"] % DPER)
    return dict(tiles=nt, last_tile_lengths=last_behind_full, mean_forms=sorted(names[f] for f in forms),
                three_kernel_tiles=sorted({geometry(n, NFM, False)["tiles"] for n in SIZE_LIST}),
                out_chunks=sorted({geometry(n, AM)["chunks"] for n in SIZE_LIST}),
                odd_frames_with_ragged_chained_tiles=chained_unaligned,
                mean_rows=sorted({mean_blocks(s * nf) for _, s, nf in MEAN_BLOCKS}))


# ---------------------------------------------------------------------------------------------------------------- call schedules
def calls_of(n):
    """frames per call"""
    if n >= DHALO:
        return (2, 1, 3)  # a call's later frames take the fast-load branch; odd n enters the NCO table at both parities
    below = max(1, (DHALO - 1) // n)                        # the longest call below 21 samples
    at = DHALO // n if DHALO % n == 0 else -(-DHALO // n)   # exactly 21 where n divides it, else the first length above
    return (1, below, 1, at, DHALO // n + 2, 1)


def short_calls(n):
    """(calls shorter than 21 samples, those of them that follow another such call)"""
    lens = [nf * n for nf in calls_of(n)]
    short = [L < DHALO for L in lens]
    return sum(short), sum(a and b for a, b in zip(short, short[1:]))


# ---------------------------------------------------------------------------------------------------------------- signals
@functools.lru_cache(maxsize=None)
def grid_signal(n, streams=S, shift=0.0):
    """int16 IQ [streams][2 * total] for calls_of(n): fm_am_signal, one carrier per stream"""
    from test_gpu_demod import fm_am_signal
    total = sum(calls_of(n)) * n
    rng = np.random.default_rng(7 * n + 1)
    raws = np.stack([fm_am_signal(rng, total, RATE, fc=5000.0 + 900.0 * s + shift, seed_shift=31.0 * s) for s in range(streams)])
    raws.setflags(write=False)
    return raws


PLANT, PLANT_Q, QUIET, LOUD_LO, LOUD_HI = 20000, 300, 1000, 29000, 31000
PLANTED_SIZES = (8, 2049, 2056, 4097, 8192, 10239)
PLANT_SEED_STEP = {8: 3, 2056: 2}
PLANTED_CALLS = (2, 4, 2)  # every call: loud, quiet, (loud, quiet): its last frame is quiet, the next row's first frame loud


def planted_positions(n):
    """where a quiet frame's one large sample is put: the frame's first and last sample, the first and last sample of every
    tile, offsets 7 and 8 of the last tile (the end of thread 0's run and the start of thread 1's), the last sample of a
    ragged tile"""
    g = geometry(n, RAW)
    pos = {0, n - 1}
    for j in range(g["tiles"]):
        pos |= {j * DTILE, min((j + 1) * DTILE, n) - 1}
    base = (g["tiles"] - 1) * DTILE
    pos |= {base + o for o in (DPER - 1, DPER) if o < g["last"]}
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def planted(n):
    """(int16 IQ [S][2 * total], plan): plan = [(stream, frame of the stream, position, I, Q)] of every quiet frame"""
    nfr = sum(PLANTED_CALLS)
    assert all(c % 2 == 0 for c in PLANTED_CALLS)
    pos = planted_positions(n)
    assert len(pos) <= S * nfr // 2, (n, pos)
    # (seeds at which, in AM, the oracle's max + avg is the planted magnitude to the bit in EVERY quiet frame: max is left as
    # max - avg (:465), and adding avg back rounds away from it in about one frame in ten)
    rng = np.random.default_rng(900 + n + 100000 * PLANT_SEED_STEP.get(n, 0))
    raws = np.empty((S, nfr, n, 2), np.int16)
    plan = []
    for s in range(S):
        for f in range(nfr):
            if f % 2 == 0:
                raws[s, f] = rng.integers(LOUD_LO, LOUD_HI + 1, (n, 2)) * rng.choice((-1, 1), (n, 2))
            else:
                raws[s, f] = rng.integers(-QUIET, QUIET + 1, (n, 2))
                k = (f // 2) * S + s  # (stream s: positions s, s + 3, s + 6, s + 9 of the list, taken round)
                p, i = pos[k % len(pos)], (PLANT if k % 2 == 0 else -PLANT)
                raws[s, f, p] = (i, PLANT_Q)
                plan.append((s, f, p, i, PLANT_Q))
    raws = raws.reshape(S, 2 * nfr * n)
    raws.setflags(write=False)
    return raws, tuple(plan)


def convert(v):
    """JavaAudio's (float)s / 32767f"""
    return f32(v) / f32(32767)


def planted_magnitude(mode, i, q):
    """what the reference's detector gives at the planted sample with filter and mixer off (demod.java:441-463)"""
    x, y = convert(i), convert(q)
    if mode == RAW:
        return f32(abs(x))
    assert mode == AM
    return f32(np.sqrt(np.float64(f32(f32(x * x) + f32(y * y)))))


RUNOUT_SIZES = (9, 2049, 2057, 4097, 10239)
RUNOUT_AMP = 24000


@functools.lru_cache(maxsize=None)
def runout(n):
    """int16 IQ [S][2 * total] for calls_of(n): a tone at half the sample rate (sign alternates from sample to sample) and a
    little noise.  BAND's filter removes it, so the frame's maximum is small -- and the filter's outputs just past a ragged
    tile's end, where it runs out over the zeros of the padded lanes, are partial sums many times larger."""
    total = sum(calls_of(n)) * n
    rng = np.random.default_rng(3100 + n)
    t = np.arange(total)
    sign = 1 - 2 * (t & 1)
    raws = np.empty((S, total, 2), np.int64)
    for s in range(S):
        raws[s, :, 0] = sign * (RUNOUT_AMP - 1000 * s) + rng.integers(-40, 41, total)
        raws[s, :, 1] = -sign * (RUNOUT_AMP // 2) + rng.integers(-40, 41, total)
    raws = raws.astype(np.int16).reshape(S, 2 * total)
    raws.setflags(write=False)
    return raws


# ---------------------------------------------------------------------------------------------------------------- mean blocks
# (frame size, streams, frames per call): AM on an ordinary handle, two calls each
MEAN_BLOCKS = ((16, 1, 63), (16, 1, 64), (16, 1, 65), (16, 5, 13), (16, 3, 43), (16, 1, 200),
               (100, 3, 2), (100, 1, 65), (68, 3, 2), (68, 1, 65),   # vector chunks, then a ragged chunk (36 and 4 columns)
               (130, 1, 65))                                          # scalar throughout, three chunks
# channel handles: (frame size, inputs, frames per call) with ONE AM channel of five: 65 and 129 AM rows
MEAN_CHANNEL_BLOCKS = ((100, 13, 5), (16, 43, 3))


@functools.lru_cache(maxsize=None)
def mean_signal(n, streams, nf, ncalls=2):
    from test_gpu_demod import fm_am_signal
    rng = np.random.default_rng(5000 + 131 * n + 7 * streams + nf)
    base = fm_am_signal(rng, ncalls * nf * n + 4 * streams, RATE, fc=6100.0)
    # cheap distinct streams: shifts of one signal (I/Q kept paired) with a gain of their own, so that no two frames share a mean
    raws = np.stack([((base[8 * s:8 * s + 2 * ncalls * nf * n].astype(np.int32) * (64 - s % 50)) // 64).astype(np.int16)
                     for s in range(streams)])
    raws.setflags(write=False)
    return raws


# ---------------------------------------------------------------------------------------------------------------- live switches
SWITCH_N = 2049
SWITCH_FRAMES = (2, 1, 2, 1, 2, 1, 2, 1)
# per call: (mode, dofir, dodwn, doagc), and whether weights(*SWITCH_BAND2) is called before it
SWITCH_CALLS = (((NFM, 1, 1, 1), False),   # 1
                ((NFM, 0, 1, 1), False),   # 2 filter off: the ring must stay as it is
                ((NFM, 1, 1, 1), False),   # 3 filter on again, over the ring call 1 left
                ((NFM, 1, 0, 1), False),   # 4 mixer off: car neither advances nor resets
                ((RAW, 1, 0, 1), False),   # 5 li / lq must be kept
                ((AM, 1, 0, 1), False),    # 6
                ((WFM, 1, 1, 1), False),   # 7 FM again, mixer on again: car goes on from call 3's end, li / lq from call 4's
                ((WFM, 1, 1, 0), True))    # 8 AGC toggled, behind a weights() call (ring cleared, car = 0)
SWITCH_BAND2 = (-9000, 2000)


@functools.lru_cache(maxsize=None)
def switch_signal():
    from test_gpu_demod import fm_am_signal
    total = sum(SWITCH_FRAMES) * SWITCH_N
    rng = np.random.default_rng(4242)
    raws = np.stack([fm_am_signal(rng, total, RATE, fc=5000.0 + 900.0 * s, seed_shift=31.0 * s) for s in range(S)])
    raws.setflags(write=False)
    return raws


# ---------------------------------------------------------------------------------------------------------------- the census
def planted_census(n, mode):
    """the oracle alone, filter and mixer off: in how many quiet frames its `max` field is exactly the planted sample's
    magnitude (AM: less the frame's mean, as :465 leaves it), and the smallest magnitude of any loud sample"""
    import oracle_lib as O
    raws, plan = planted(n)
    nfr = sum(PLANTED_CALLS)
    exact = exact_sum = 0
    loud_min = np.inf
    for s in range(S):
        o = O.Demod(RATE)
        o.configure(mode, 0, 0, 1)
        buf = O.convert_i16(raws[s])
        for f in range(nfr):
            o.receive(buf[2 * f * n:2 * (f + 1) * n])
            if f % 2:
                _, _, p, i, q = next(e for e in plan if e[0] == s and e[1] == f)
                mag = planted_magnitude(mode, i, q)
                exact += int(o.max == (f32(mag - o.avg) if mode == AM else mag))
                exact_sum += int(f32(o.max + o.avg) == mag)
            else:
                fr = buf[2 * f * n:2 * (f + 1) * n]
                m = np.abs(fr[0::2]) if mode == RAW else np.sqrt(fr[0::2].astype(np.float64) ** 2 + fr[1::2].astype(np.float64) ** 2)
                loud_min = min(loud_min, float(m.min()))
    return dict(n=n, mode=mode, quiet_frames=len(plan), exact=exact, exact_as_sum=exact_sum, positions=planted_positions(n),
                planted=float(planted_magnitude(mode, PLANT, PLANT_Q)), loud_min=round(loud_min, 6))


def switch_census():
    """the oracle alone on the switch schedule, stream 0: car after every call, and whether the first frame after the filter
    returns (call 3) differs from what a freshly cleared ring would give"""
    import oracle_lib as O
    raws = switch_signal()
    o, fresh = O.Demod(RATE), O.Demod(RATE)
    for d in (o, fresh):
        d.weights(*BAND)
    cars, lilq, pos, stale = [], [], 0, None
    for k, (nf, (cfg, reweight)) in enumerate(zip(SWITCH_FRAMES, SWITCH_CALLS)):
        for d in (o, fresh):
            if reweight:
                d.weights(*SWITCH_BAND2)
            d.configure(*cfg)
        if k == 2:
            for i in range(42):
                fresh.d.fir[i] = 0.0
        buf = O.convert_i16(raws[0][2 * pos:2 * (pos + nf * SWITCH_N)])
        for f in range(nf):
            a = o.receive(buf[2 * f * SWITCH_N:2 * (f + 1) * SWITCH_N])
            b = fresh.receive(buf[2 * f * SWITCH_N:2 * (f + 1) * SWITCH_N])
            if k == 2 and f == 0:
                stale = int(np.count_nonzero(a != b))
        cars.append(float(o.car))
        lilq.append([float(o.d.li), float(o.d.lq)])
        pos += nf * SWITCH_N
    return dict(car_after_call=cars, lilq_after_call=lilq, stale_ring_samples=stale)


def runout_census(n):
    """the oracle alone, RAW with the filter on and the mixer off: per frame, the largest |filter output| over the 20 places
    past the frame's last sample when zeros follow it, over the frame's `max`; the smallest such ratio of all frames that
    start 21 samples or more into the stream"""
    import oracle_lib as O
    raws = runout(n)
    worst, frames = np.inf, 0
    for s in range(S):
        o = O.Demod(RATE)
        w, _ = o.weights(*BAND)
        o.configure(RAW, 1, 0, 1)
        buf = O.convert_i16(raws[s])
        x = np.concatenate([np.zeros(DHALO - 1), buf[0::2].astype(np.float64)])  # (I alone: RAW takes sam[s])
        for f in range(sum(calls_of(n))):
            o.receive(buf[2 * f * n:2 * (f + 1) * n])
            end = DHALO - 1 + (f + 1) * n  # x[end - 1] is the frame's last sample
            past = max(abs(sum(float(w[k]) * x[end - 1 - (k - m)] for k in range(m, DHALO))) for m in range(1, DHALO))
            if f * n >= DHALO:  # (the stream's first 20 outputs run IN over the zeros of a new ring: as large, and inside the frame)
                worst = min(worst, past / float(o.max))
                frames += 1
    return dict(n=n, frames=frames, smallest_ratio=round(float(worst), 3))


def summary():
    return dict(runout=[runout_census(n) for n in RUNOUT_SIZES],
sizes=[[n, why] for n, why in SIZES], coverage={k: [list(x) if isinstance(x, tuple) else x for x in v]
                                                                for k, v in coverage().items()},
                schedules={str(n): dict(frames=list(calls_of(n)), short=list(short_calls(n))) for n in SIZE_LIST if n < DHALO},
                planted=[planted_census(n, mode) for n in PLANTED_SIZES for mode in (RAW, AM)],
                switches=switch_census())


def dumps(s):
    return json.dumps(s, indent=None, separators=(",", ":")) + "\n"


def load():
    with open(CENSUS) as f:
        return json.load(f)


def main(argv):
    """print the census; `--write [PATH]` writes it (to tests/golden/demod_census.json by default)"""
    s = summary()
    for p in s["planted"]:
        print("planted n=%5d mode %d: %2d quiet frames, exact in %2d (as max + avg in %2d), loud >= %.4f > %.4f" % (
            p["n"], p["mode"], p["quiet_frames"], p["exact"], p["exact_as_sum"], p["loud_min"], p["planted"]))
    for k in ("runout", "coverage", "schedules", "switches"):
        print(k, s[k])
    if "--write" in argv:
        rest = argv[argv.index("--write") + 1:]
        path = rest[0] if rest else CENSUS
        with open(path, "w") as f:
            f.write(dumps(s))
        print("wrote", path)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    main(sys.argv[1:])
