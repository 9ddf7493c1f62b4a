"""CPU: the inputs of tests/test_gpu_sync_cases.py take the sync stage (FUNcubeBPSKDemod.java:553-572) where they are meant to --
counted on the oracle's bit log alone, before any kernel is asked -- and the oracle's own sync code is right there.

1. The census of sync_cases.CASES and the call schedules, recomputed, equal tests/golden/sync_census.json.
2. The census meets the conditions that make the GPU tests bite, all exact: 45 and 43 with a full register (in each flip layout),
   44 and 45 with zeros in the register, hits on adjacent bits, two hits at each of the offsets 1, 63, 64, 65, 255, 256, 257, a
   stronger hit followed by a weaker one, a correlation of -65, hits that decode at all four alignments, and a hit whose window
   decodes differently under the two mappings of the register's zero bytes.  A generator change that breaks one of these calls
   for other cases, not for a weaker condition.
3. The schedules have the seams they claim: a hit at each of the in-call bit indices 0, 1, 62, 63, 64, 65, 255, 256 and as the
   last bit of a call, per family a call of no new bit directly before a hit and one directly after, both orders of a 65 and a 45
   inside one call, calls of 1 .. 17, 79, 80, 81, 255, 256 and 257 new bits with a hit as the last bit of one, no call with more
   hits than a handle logs, and the one-stream schedules within the length that k_sync_t orders itself.
4. sync_cases.restate -- :553-572 in numpy over the bit log, which shares no line with oracle/o_bpsk.c -- agrees with O.Bpsk on
   cntFEC, dmCorr and dmMaxCorr after every call of every schedule and on the trigger bit and rc of every FEC result."""
import functools

import numpy as np

import oracle_lib as O
import sync_cases as Y

SCHEDULES = ("one_call", "seams", "lengths")


@functools.lru_cache(maxsize=None)
def summary():
    return Y.summary()


@functools.lru_cache(maxsize=None)
def cen(name):
    return next(c for c in summary()["cases"] if c["name"] == name)


@functools.lru_cache(maxsize=None)
def bits_of(name):
    return Y.oracle_bits(Y.stream_of(Y.BY_NAME[name]))


@functools.lru_cache(maxsize=None)
def restated(name):
    return Y.restate(bits_of(name))


@functools.lru_cache(maxsize=None)
def stepped(name, sched):
    calls = [Y.N] if sched == "one_call" else summary()["schedules"][sched]
    return Y.stepped(Y.stream_of(Y.BY_NAME[name]), calls)


def schedules_of(case):
    return SCHEDULES + ("fused_" + case[0],)


def corr_at(name, b):
    return int(restated(name)["corr"][b])


# ---------------------------------------------------------------------------------------------------------------- 1
def test_the_census_is_the_committed_one(capsys):
    got, want = summary(), Y.load()
    with capsys.disabled():
        print("\nsync census (hits: correlation at bit):")
        for c in got["cases"]:
            print("   %-17s %s  largest non-hit %d, smallest %d" % (c["name"], " ".join("%d@%d" % p for p in zip(c["corr"], c["hits"])),
                                                                    c["max_nonhit"], c["min_corr"]))
    assert sorted(got) == sorted(want)
    assert got["cases"] == want["cases"]
    assert got["schedules"] == want["schedules"]


def test_the_designed_symbols_arrive_as_designed():
    for case in Y.CASES:
        bits, sym = bits_of(case[1]), Y.symbols_of(case)
        assert bits.size == Y.NSYM - Y.LEAD, (case[1], bits.size)  # (no bit lost while the bit clock settles: the places hold)
        assert np.array_equal(bits[Y.LEAD + Y.SETTLE:], sym[Y.SETTLE:bits.size - Y.LEAD]), case[1]
        # every hit is a designed one
        assert set(cen(case[1])["hits"]) <= set(Y.designed_places(case)), case[1]


# ---------------------------------------------------------------------------------------------------------------- 2
def test_the_threshold_is_met_from_both_sides_with_a_full_register():
    for layout, first in (("first", 0), ("last", 1), ("spread", 2)):
        name = "threshold_" + layout
        c = cen(name)
        places = [Y.slot(first + 3 * i) for i in range(4)]
        assert [corr_at(name, b) for b in places] == [47, 45, 43, 41], name
        assert c["hits"] == places[:2] and c["corr"] == [47, 45] and c["max_nonhit"] == 43 and c["zeros"] == [0, 0], name
    # the inverted taps: every dword of the packed dot product, and the 65th tap, decide a threshold
    dwords = set()
    for layout in ("first", "last", "spread"):
        for k in (10, 11):
            dwords |= {t // 4 for t in Y.flip_layout(layout, k)}
            assert len(set(Y.flip_layout(layout, k))) == k
    assert dwords == set(range(17)) and 64 in Y.flip_layout("last", 10)


def test_hits_and_misses_with_zeros_in_the_register():
    assert cen("early_45")["hits"] == [Y.early_hit(45)] and cen("early_45")["corr"] == [45]
    assert cen("early_45")["zeros"] == [Y.REG - 1 - Y.early_hit(45)] and cen("early_45")["zeros"][0] > 20 * Y.STRIDE - 80
    assert cen("early_44")["hits"] == [] and corr_at("early_44", Y.early_hit(44)) == 44 and cen("early_44")["max_nonhit"] == 44
    assert cen("early_46_flip")["hits"] == [] and corr_at("early_46_flip", Y.early_hit(46)) == 44
    assert cen("early_47_flip")["hits"] == [Y.early_hit(47)] and cen("early_47_flip")["corr"] == [45]
    # an even correlation exists only while the register holds zeros
    for case in Y.CASES:
        corr = restated(case[1])["corr"]
        assert (corr[Y.REG - 1:] % 2 == 1).all(), case[1]


def test_the_two_mappings_of_the_zero_bytes_decode_differently():
    """the decodable early hit: 0x40 recovers the payload, 0xc0 fails"""
    c = cen("early_frame")
    assert c["hits"] == [Y.EARLY_FRAME_HIT] and c["corr"] == [55] and c["zeros"] == [Y.EARLY_FRAME_LOST - Y.LEAD]
    assert c["rc"][0] > 0 and c["rc_c0"][0] != c["rc"][0], (c["rc"], c["rc_c0"])
    assert c["rc_c0"] == [-1]  # (more than different: the wrong mapping does not decode at all)
    bits, b = bits_of("early_frame"), c["hits"][0]
    rc, out = O.fec_decode(Y.window(bits, b))
    assert rc == c["rc"][0] and np.array_equal(out, Y.payload_of(2051))  # 0x40: the payload, through the lost symbols
    o = O.Bpsk(blen=4)
    o.receive_i16(Y.stream_of(Y.BY_NAME["early_frame"]))
    assert [(r, bi) for r, bi, _ in o.fec_results()] == [(rc, b + 1)] and np.array_equal(o.decoded(), out)


def test_hits_on_adjacent_bits_and_at_every_offset():
    a = cen("neighbours_a")
    runs = {2: Y.slot(12), 3: Y.slot(26), 4: Y.slot(16)}
    for n, at in runs.items():
        assert all(b in a["hits"] for b in range(at, at + n)) and at - 1 not in a["hits"] and at + n not in a["hits"], n
    hits = {1: a["hits"]}
    hits.update({d: cen("neighbours_b")["hits"] for d in (63, 64, 65, 255, 256, 257)})
    for d, s in Y.PAIR_SLOTS.items():
        assert Y.slot(s) in hits[d] and Y.slot(s) + d in hits[d], d
    assert sorted(Y.PAIR_SLOTS) == [1, 63, 64, 65, 255, 256, 257] and not any(d % Y.STRIDE == 0 for d in Y.PAIR_SLOTS)
    assert set(a["corr"]) == {65} and set(cen("neighbours_b")["corr"]) == {65}
    assert len(a["hits"]) == 11 and len(cen("neighbours_b")["hits"]) == 12


def test_a_weaker_hit_behind_a_stronger_one_and_an_inverted_image():
    c = cen("order")
    assert c["hits"] == [Y.slot(23), Y.slot(23) + 100, Y.slot(24), Y.slot(24) + 100] and c["corr"] == [65, 45, 45, 65]
    r = restated("order")
    assert int(r["max"][Y.slot(23) + 99]) == 65 and int(r["max"][Y.slot(23) + 100]) == 45  # dmMaxCorr comes down (:567)
    assert int(r["max"][Y.slot(24) - 1]) == 45 and int(r["max"][Y.slot(24) + 100]) == 65
    assert corr_at("order", Y.slot(17)) == -65 and c["min_corr"] == -65


def test_frames_decode_at_all_four_alignments():
    al = set()
    for name in ("frames_a", "frames_b"):
        c = cen(name)
        assert c["hits"] == list(Y.FRAME_HITS[name]) and c["corr"] == [65, 65] and c["rc"] == [0, 0], name
        al |= set(c["align"])
        for i, b in enumerate(c["hits"]):
            seed = (5010 if name == "frames_a" else 5020) + i
            assert np.array_equal(O.fec_decode(Y.window(bits_of(name), b))[1], Y.payload_of(seed)), (name, i)
    assert al == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------------------------- 3
def seen_at(sched, name, bit):
    return Y.in_call_index([n for n, _, _ in stepped(name, sched)], bit)


def test_the_seam_schedule_puts_hits_where_it_claims():
    calls = summary()["schedules"]["seams"]
    assert sum(calls) == Y.N and min(calls) > 0 and any(L % Y.DECIM for L in calls)
    index_of_hits, last_hits = set(), 0
    before, after = set(), set()
    for name, bit, k, zb, end, za in Y.TARGETS:
        fam = Y.BY_NAME[name][0]
        newbits = [n for n, _, _ in stepped(name, "seams")]
        call, idx, n = seen_at("seams", name, bit)
        is_hit = bit in cen(name)["hits"]
        if k is not None:
            assert idx == k, (name, bit, idx, k)
            if is_hit:
                index_of_hits.add(idx)
        if zb:
            assert is_hit and idx == 0 and newbits[call - 1] == 0, (name, bit)
            before.add(fam)
        if end is not None:
            ecall, eidx, en = seen_at("seams", name, end)
            assert eidx == en - 1, (name, end, eidx, en)
            assert ecall == call  # (what lies between the two is one call)
            if end in cen(name)["hits"]:
                last_hits += 1
                if za:
                    assert newbits[ecall + 1] == 0, (name, end)
                    after.add(fam)
        # every hit of every case: its index in the call (held taps and pairs reach the indices behind their first hit)
    for case in Y.CASES:
        for b in cen(case[1])["hits"]:
            index_of_hits.add(seen_at("seams", case[1], b)[1])
    assert set(Y.SEAM_INDICES) <= index_of_hits, sorted(index_of_hits)
    assert last_hits >= 5 and before == set(Y.FAMILIES) and after == set(Y.FAMILIES), (last_hits, before, after)
    # a correlation of 43, of 44 and of -65 is what a call leaves in dmCorr
    left = {c["dmCorr"] for case in Y.CASES for _, c, _ in stepped(case[1], "seams")}
    assert {43, 44, 45, -65} <= left, sorted(left)
    # both orders of a 65 and a 45 inside one call; held taps across a ballot chunk's and a thread stride's edge
    for at in (Y.slot(23), Y.slot(24)):
        assert seen_at("seams", "order", at)[0] == seen_at("seams", "order", at + 100)[0]
    assert [seen_at("seams", "neighbours_a", Y.slot(12) + i)[1] for i in range(2)] == [Y.CHUNK - 1, Y.CHUNK]
    assert [seen_at("seams", "neighbours_a", Y.slot(16) + i)[1] for i in range(4)] == [253, 254, 255, Y.THREAD_STRIDE]
    # the four alignments of the decoders' window, as indices in a call
    al = {(seen_at("seams", n, b)[1] + 1) % 4 for n in Y.FRAME_HITS for b in Y.FRAME_HITS[n]}
    assert al == {0, 1, 2, 3}


def test_the_lengths_schedule_has_calls_of_every_listed_length_that_end_on_hits():
    calls = summary()["schedules"]["lengths"]
    assert sum(calls) == Y.N and min(calls) > 0
    for name, hit, order in Y.LENGTH_ANCHORS:
        newbits = [n for n, _, _ in stepped(name, "lengths")]
        call, idx, n = seen_at("lengths", name, hit)
        assert hit in cen(name)["hits"] and idx == n - 1, (name, hit, idx, n)
        want = list(Y.LENGTHS[::order])[::-1]
        assert newbits[call - len(want) + 1:call + 1] == want, (name, newbits[call - len(want) + 1:call + 1])
    assert set(Y.LENGTHS) == set(range(1, 18)) | {79, 80, 81, 255, 256, 257}
    # (one anchor ends a call of one new bit, the other a call of 257)
    assert {seen_at("lengths", name, hit)[2] for name, hit, _ in Y.LENGTH_ANCHORS} == {1, 257}


def test_no_call_holds_more_hits_than_a_handle_logs_and_the_fused_calls_are_short_enough():
    for case in Y.CASES:
        for sched in schedules_of(case):
            calls = [Y.N] if sched == "one_call" else summary()["schedules"][sched]
            # (the GPU test creates the handles of several streams for calls of N samples, those of one stream for the longest call)
            cap = Y.trig_cap(max(calls) if sched.startswith("fused_") else Y.N)
            done = 0
            for _, c, _ in stepped(case[1], sched):
                assert c["cntFEC"] - done <= cap, (case[1], sched, c["cntFEC"] - done, cap)
                done = c["cntFEC"]
    for f in Y.FAMILIES:
        calls = summary()["schedules"]["fused_" + f]
        assert sum(calls) == Y.N and max(calls) <= Y.FUSED_MAX and len(calls) <= 40, f
    assert len(summary()["schedules"]["seams"]) <= 70 and len(summary()["schedules"]["lengths"]) <= 60
    assert Y.N > Y.FUSED_MAX  # (the one-call schedule on one stream is the unfused k_sync_t)
    assert 5 << 20 <= Y.fallback_batch_samples() <= 6 << 20


# ---------------------------------------------------------------------------------------------------------------- 4
def test_the_restatement_and_the_oracle_agree_after_every_call():
    ncalls = 0
    for case in Y.CASES:
        name = case[1]
        r, c = restated(name), cen(name)
        for sched in schedules_of(case):
            nb = 0
            for n, cnt, fec in stepped(name, sched):
                nb += n
                where = (name, sched, nb)
                assert cnt["cntBit"] == nb
                assert cnt["dmCorr"] == (int(r["corr"][nb - 1]) if nb else 0), where
                assert cnt["dmMaxCorr"] == (int(r["max"][nb - 1]) if nb else 0), where
                assert cnt["cntFEC"] == (int(r["fec"][nb - 1]) if nb else 0), where
                k = cnt["cntFEC"]
                assert fec == [(rc, b + 1) for rc, b in zip(c["rc"][:k], c["hits"][:k])], where
                assert cnt["cntDec"] == sum(rc >= 0 for rc in c["rc"][:k]), where
                if k:
                    assert cnt["dmErrBits"] == c["rc"][k - 1] and cnt["decodeOK"] == int(c["rc"][k - 1] >= 0), where
                ncalls += 1
        assert cen(name)["final"] == [int(r["corr"][-1]), int(r["max"][-1]), int(r["fec"][-1])]
    assert ncalls > 1500
