"""CPU: the inputs of tests/test_gpu_peak_walk.py take the peak machine (FUNcubeBPSKDemod.java:537, :577-579, :586-592) where they are
meant to -- counted on the oracle alone, before any kernel is asked -- and the oracle itself is right there.

1. The census of peak_walk.CASES, recomputed, equals tests/golden/peak_walk_census.json, and meets the conditions that make the GPU
   tests bite: a stream locked at each of the eight bit positions, every one of the 56 moves dmPeakPos -> dmPeakPos', either order of
   the old peak's decision and the hand-over point, a second decision in the period of the hand-over and none, periods with two
   decisions and with none.  A generator change that breaks one of these calls for other cases, not for a weaker condition.
2. The call schedules of the GPU test have the seams they claim: a call that starts at each bit position with each length of 1 .. 9
   outputs while every stream is locked; for every move a call boundary inside the bit period of one of its hand-overs.
3. The C oracle against the pure-Python restatement of the Java text on a noise-only stream, frame by frame: the existing fixtures
   are locked signals, which pin the oracle's peak machine at one position only."""
import functools
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import peak_walk as P

ND, SPB = len(P.DELAYED), P.SPB


@functools.lru_cache(maxsize=None)
def censuses():
    return tuple(P.census(P.stream_of(case)) for case in P.CASES)


def test_the_census_is_the_committed_one(capsys):
    got, want = P.summary(list(censuses())), P.load()
    with capsys.disabled():
        print("\npeak-walk census, moves dmPeakPos (row) -> dmPeakPos' (column):")
        for row in got["moves"]:
            print("   " + " ".join("%5d" % v for v in row))
        print("   missing %s, periods with two decisions %d, with none %d, seams %d" % (got["missing"], got["two"], got["none"], len(got["seams"])))
    assert sorted(got) == sorted(want)
    for k in got:
        assert got[k] == want[k], k


def test_a_stream_locks_at_every_bit_position():
    for p, (case, c) in enumerate(zip(P.DELAYED, censuses()[:ND])):
        assert case[4] == P.DELAY_OF_POSITION[p]
        pos, clocks, first = c["locked"]
        assert c["final"] == (p, p) and pos == p and clocks >= 1000, (p, c["final"], c["locked"])
        assert first + clocks == c["periods"], (p, c["locked"])  # locked to its end
    assert sorted(P.DELAY_OF_POSITION) == list(range(SPB)) and all(0 <= d < 80 for d in P.DELAY_OF_POSITION.values())
    ninth = P.census(P.stream_of(P.NINTH_LOCKED))
    assert ninth["final"] == (1, 1) and ninth["locked"][1] >= 1000 and P.NINTH_LOCKED not in P.DELAYED


def test_every_move_of_the_peak_occurs():
    m = P.moves_of(censuses())
    assert not np.diag(m).any()
    for p in range(SPB):
        for q in ((p + 1) % SPB, (p - 1) % SPB):
            assert m[p, q] >= 3, (p, q, int(m[p, q]))
    missing = [(p, q) for p in range(SPB) for q in range(SPB) if p != q and m[p, q] == 0]
    assert int((m > 0).sum()) == 56 and missing == [] and P.load()["missing"] == []
    # the walks alone (one handle of the GPU test) hold them all
    assert int((P.moves_of(censuses()[ND:]) > 0).sum()) == 56


def test_the_moves_hold_every_order_of_decision_and_hand_over():
    m = P.moves_of(censuses()[ND:])
    kinds = {}
    for p in range(SPB):
        for q in range(SPB):
            if m[p, q]:
                h = (p + 4) % SPB
                assert (h < p) == (p >= 4)
                k = ("h<pk" if h < p else "h>pk", bool(P.same_period_decision(p, q)))
                kinds[k] = kinds.get(k, 0) + int(m[p, q])
    for k in (("h<pk", True), ("h<pk", False), ("h>pk", True), ("h>pk", False)):
        assert kinds.get(k, 0) >= 1, (k, kinds)
    cs = censuses()
    assert sum(c["two"] for c in cs[ND:]) >= 20 and sum(c["none"] for c in cs[ND:]) >= 20
    # a period with two decisions is a hand-over to a later position, one with none a hand-over to an earlier one
    assert all(c["none_bits"] >= c["none"] for c in cs)


def test_the_locked_schedule_starts_and_ends_calls_at_every_bit_position():
    calls = P.locked_calls()
    assert sum(calls) == P.N_LOCKED and min(calls) > 0
    sp = P.spans(calls)
    locked_from = max(c["locked"][2] for c in censuses()[:ND])
    seen = set()
    for (a, b), L in zip(sp, calls):
        if a >= SPB * locked_from and L % P.DECIM == 0 and 1 <= b - a <= 9:
            seen.add((a % SPB, b - a))
    assert seen == {(s, n) for s in range(SPB) for n in range(1, 10)}
    # calls without a decision, with nothing but the decision, with nothing but the hand-over point -- for every locked position v
    for v in range(SPB):
        h = (v + 4) % SPB
        inside = [(a, b) for a, b in sp if a >= SPB * locked_from and 0 < b - a < SPB]
        assert any(all(g % SPB != v for g in range(a, b)) for a, b in inside), v
        assert any(b - a == 1 and a % SPB == v for a, b in inside), v
        assert any(b - a == 1 and a % SPB == h for a, b in inside), v
    assert any(L % P.DECIM for L in calls) and any(b == a for a, b in sp)  # odd lengths; a call that yields no output
    # one call holds more than three whole chunks of either kernel (64 bit periods), whatever its start
    assert max(b - a for a, b in sp[1:]) >= 4 * 64 * SPB + SPB


def test_the_seam_schedule_cuts_a_hand_over_of_every_move():
    walks = list(censuses()[ND:])
    plan = P.seam_plan(walks)
    assert [list(x) for x in plan] == P.load()["seams"]
    calls = P.seam_calls(plan, P.N_WALK)
    assert sum(calls) == P.N_WALK and min(calls) > 0
    starts = {a for a, _ in P.spans(calls)[1:]}  # first 9600 Hz sample of every call but the first
    assert any(L % P.DECIM for L in calls)
    cut, old_hand, hand_new = set(), 0, 0
    for ci, c in enumerate(walks):
        for g, p, q in c["handovers"]:
            base, h = g - g % SPB, (p + 4) % SPB
            inside = [b - base for b in starts if base < b <= base + 7]
            if inside:
                cut.add((p, q))
            old_hand += any(p < x <= h for x in inside)                       # the old peak decided in the call before
            hand_new += any(h < x <= q for x in inside)                       # the new peak decides in the call after
    present = {(p, q) for c in walks for _, p, q in c["handovers"]}
    assert cut == present and len(present) == 56
    assert old_hand >= 1 and hand_new >= 1, (old_hand, hand_new)
    for ci, g, p, q, b, kind in plan:
        assert (g, p, q) in walks[ci]["handovers"] and b in starts and g - g % SPB < b <= g - g % SPB + 7


def test_the_mixed_wave_case_walks_within_the_locked_length():
    c = P.census(P.stream_of(P.MIXED_WALK)[:2 * P.N_LOCKED])
    assert len(c["handovers"]) >= 100 and int((P.moves_of([c]) > 0).sum()) >= 30, len(c["handovers"])
    calls = P.mixed_calls()
    assert sum(calls) == P.N_LOCKED and min(calls) > 0 and any(L % P.DECIM for L in calls)
    # the wandering stream walks in every call that holds a whole chunk of either kernel (64 bit periods)
    sp = P.spans(calls)
    assert all(any(a <= g < b for g, _, _ in c["handovers"]) for (a, b) in sp if b - a >= 64 * SPB)


RESTATED_HANDOVERS = 40


def test_the_restatement_and_the_oracle_agree_on_a_wandering_peak():
    """frames of one 9600 Hz sample over the shortest prefix of the first noise-only case that holds 40 hand-overs, rounded up to a
    whole bit period (under a second in pure Python)"""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    ref = os.environ.get("JSDR_REFERENCE", "/root/reference")  # (where java_restatement looks for the reference's text)
    if not all(os.path.isfile(os.path.join(ref, f)) for f in ("FECDecoder.java", "FUNcubeBPSKDemod.java")):
        pytest.skip("java_restatement parses its tables out of the reference's text, which is not present here")
    import java_restatement as R
    case = P.NOISE[0]
    hand = censuses()[ND + P.WALKS.index(case)]["handovers"]
    nds = hand[RESTATED_HANDOVERS - 1][0] + 1
    nds += -nds % SPB
    iq = P.stream_of(case)[:2 * P.DECIM * nds]
    o = O.Bpsk(blen=4 * P.DECIM, size=4, trace=nds + 8)
    r = R.Demod(trace_cap=nds + 8)
    x = R.convert_i16(iq)
    seen, last = 0, 0
    for g in range(nds):
        o.receive_i16(iq[2 * P.DECIM * g:2 * P.DECIM * (g + 1)])
        r.receive(x[2 * P.DECIM * g:2 * P.DECIM * (g + 1)])
        assert list(o.istate()) == r.istate(), (g, o.istate(), r.istate())
        seen += r.dmPeakPos != last
        last = r.dmPeakPos
    assert seen >= RESTATED_HANDOVERS
    assert np.array_equal(o.bits(), np.array(r.bits, np.int8))
    oc = o.counters()
    assert [oc[k] for k in ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK")] == r.counters()[:9]
    assert o.state().tobytes() == np.array(r.state(), np.float64).tobytes()
    assert o.trace().tobytes() == np.array(r.trace, np.float64).tobytes()
