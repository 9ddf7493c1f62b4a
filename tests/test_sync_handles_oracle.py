"""CPU: the inputs of tests/test_gpu_sync_handles.py take the sync stage where they are meant to -- counted on the oracle's bit log
alone (sync_handles.census), per (case, variant), before any kernel is asked.  The conditions are caps, not measurements: where
one fails, a hit is moved or a seed changed, never the condition.

1. sync_cases.stream_of with its new carrier argument still produces the streams of the committed sync census, byte for byte,
   and the census of sync_handles, recomputed, is tests/golden/sync_handles_census.json to the byte.
2. Under every variant a case is used in, the oracle's hits are the designed ones after the constant offset the census records
   (for sync_cases' streams: the hits and correlations of the committed 12000 Hz census, moved by the offset).  Nothing is
   dropped: every case sync_handles lists is in the census and meets this.
3. The cap streams hold exactly 7, 8, 9 and 12 hits in one call of their schedule, the first at in-call bit 60, on handles that
   log 8 hits a call; no other call of any schedule holds more hits than its handle logs.
4. The threshold family gives 47 and 45 (hits) and 43 / 41 (no hits) at every tuning and at 9600 in FFT-acquire; the early frame
   decodes with the register's zeros as 0x40 and does not as 0xc0 wherever it is used; the pass-through stream has no hit.
5. The FFT-acquire schedules reach the in-call bits 0, 1, 63, 64 and the last bit of a call (9600: 255 and 256 too, in a call of
   three frames or more), with a call of one frame directly before and directly after each such call; the tuned schedule keeps
   the seams of sync_cases (a hit at in-call bits 0, 1, 62 .. 65, 255, 256, as the last bit of a call, calls of no new bit)."""
import numpy as np

import sync_cases as Y
import sync_handles as H


def entries(kind):
    return H.census()[kind]


def test_the_default_carrier_gives_the_committed_streams():
    """(the assertions of test_sync_cases_oracle.py stay as they are; this is the byte identity they rest on)"""
    want = {c["name"]: c for c in Y.load()["cases"]}
    for case in Y.CASES:
        a, b = Y.stream_of(case), Y.stream_of(case, 13200.0)
        assert a.dtype == np.int16 and a.tobytes() == b.tobytes(), case[1]
        assert a.tobytes() == H.input_of(case, H.TUNE(12000)).tobytes(), case[1]
        assert Y.census(a) == {k: v for k, v in want[case[1]].items() if k not in ("name", "family")}, case[1]
        assert Y.stream_of(case, 10200.0).tobytes() != a.tobytes()
    assert Y.load()["schedules"] == Y.summary()["schedules"]


def test_the_census_is_the_committed_one(capsys):
    got = H.census()
    with capsys.disabled():
        print("\nsync census per handle kind (correlation at bit; offset of the variant):")
        for kind in ("cap", "tuned", "fft"):
            for e in got[kind]:
                print("   %-17s %-14s %+d  %s" % (e["name"], "%s %d" % tuple(e["variant"]), e["offset"],
                                                  " ".join("%d@%d" % p for p in zip(e["corr"], e["hits"]))))
    with open(H.CENSUS) as f:
        assert f.read() == H.text(got)
    assert H.load() == got


def test_every_listed_case_is_in_the_census_and_hits_where_it_was_designed_to():
    listed = [(c[1], H.CAP_VARIANT) for c in H.CAP] + [(n, H.TUNE(t)) for n, t in H.TUNED + [H.PASS_THROUGH]]
    listed += [(n, H.FFT(f)) for f in H.FRAMES for n in H.FFT_CASES[f]]
    got = [(e["name"], tuple(e["variant"])) for kind in ("cap", "tuned", "fft") for e in entries(kind)]
    assert got == listed and len(set(listed)) == len(listed)
    original = {c["name"]: c for c in Y.load()["cases"]}
    for kind in ("cap", "tuned", "fft"):
        for e in entries(kind):
            where = (e["name"], e["variant"])
            d = e["offset"]
            assert abs(d) <= 2, where
            if (e["name"], tuple(e["variant"])) == (H.PASS_THROUGH[0], H.TUNE(H.PASS_THROUGH[1])):
                continue
            if e["name"] in original:  # the 12000 Hz census, moved
                o = original[e["name"]]
                assert e["hits"] == [b + d for b in o["hits"]] and e["corr"] == o["corr"], where
                assert e["max_nonhit"] <= max(o["max_nonhit"], 43), where
                assert e["nbits"] >= o["nbits"] - 40, where  # (whole frames: up to 38 bits fewer)
            else:                      # cap and placed streams: every designed place a full hit, nothing else
                assert e["hits"] == [p + d for p in e["designed"]] and set(e["corr"]) == {65}, where
                assert e["zeros"] == [0] * len(e["hits"]), where
            assert set(e["hits"]) <= {p + d for p in e["designed"]}, where
    # each tuning kind is there: a period of eight samples, a short period, no period; one stream is passed through
    tunings = {t for _, t in H.TUNED}
    assert {12000, 9000} <= tunings and tunings & {12345, 11990} and H.PASS_THROUGH[1] <= 0
    assert {tuple(e["variant"]) for e in entries("fft")} == {H.FFT(9600), H.FFT(8192)}


def test_the_cap_streams_fill_their_log_exactly_as_designed():
    assert Y.trig_cap(H.CAP_BATCH) == 8 and max(H.cap_calls()) <= H.CAP_BATCH <= 160000 and sum(H.cap_calls()) == Y.N
    for e in entries("cap"):
        seen = e["seen"]["cap"]
        assert len(seen) == H.CAP_HITS[e["name"]] and len({k for k, _, _ in seen}) == 1, e["name"]  # one call holds them all
        assert seen[0][1] == H.CAP_INDEX == 60, e["name"]
        idx = [i for _, i, _ in seen]
        assert idx[:8] == list(range(60, 68))[:len(idx)], e["name"]  # four slots from one 64-bit ballot, the rest from the next
    assert sorted(H.CAP_HITS.values()) == [7, 8, 9, 12] == sorted(len(e["hits"]) for e in entries("cap"))
    for over, rows in H.CAP_ROWS.items():
        n = [H.CAP_HITS.get(r, 0) for r in rows]
        assert n[:3] == [7, over, 8] and rows[3].startswith("threshold")  # the full row directly behind the overflowing one
        # the threshold stream on the cap schedule: a row whose calls never come near the cap
        case = Y.BY_NAME[rows[3]]
        nb = H.newbits(case, H.CAP_VARIANT, H.cap_calls())
        hits = next(c for c in Y.load()["cases"] if c["name"] == rows[3])["hits"]
        assert len(hits) == 2 and len({Y.in_call_index(nb, b)[0] for b in hits}) == 2


def test_no_other_call_holds_more_hits_than_its_handle_logs():
    """(the GPU test creates the tuned and FFT-acquire handles for calls of N samples)"""
    cap = Y.trig_cap(Y.N)
    for kind in ("tuned", "fft"):
        for e in entries(kind):
            for seen in e["seen"].values():
                calls = [k for k, _, _ in seen]
                assert max([calls.count(k) for k in set(calls)] or [0]) <= cap, (e["name"], e["variant"])
    for name in ("seams", "one_call", "lengths"):  # sync_cases' streams on channel handles, created the same way
        assert max(Y.schedule(name)) <= Y.N


def test_the_threshold_is_met_from_both_sides_at_every_tuning_and_in_fft_acquire():
    found = set()
    for kind in ("tuned", "fft"):
        for e in entries(kind):
            if e["name"].startswith("threshold") and e["variant"] != ["tune", 0]:
                assert e["designed_corr"] == [47, 45, 43, 41] and e["corr"] == [47, 45] and e["max_nonhit"] == 43, (e["name"], e["variant"])
                found.add(tuple(e["variant"]))
    assert {H.TUNE(12000), H.TUNE(9000), H.TUNE(12345), H.FFT(9600)} <= found, found
    assert sum(v == H.FFT(9600) for v in found) == 1 and sum(e["name"].startswith("threshold") for e in entries("fft") if e["variant"][1] == 9600) == 3
    p = next(e for e in entries("tuned") if e["variant"] == ["tune", 0])
    assert p["hits"] == [] and p["nbits"] > 0  # passed through: garbage bits, no hit


def test_the_early_frame_needs_the_zeros_as_0x40_wherever_it_is_used():
    used = [e for kind in ("tuned", "fft") for e in entries(kind) if e["name"] == "early_frame"]
    assert {tuple(e["variant"]) for e in used} >= {H.TUNE(12000), H.TUNE(12345), H.FFT(9600), H.FFT(8192)}
    for e in used:
        assert e["corr"] == [55] and e["rc"][0] > 0 and e["rc_c0"] == [-1], (e["variant"], e["rc"], e["rc_c0"])
        assert e["zeros"][0] == Y.EARLY_FRAME_LOST - Y.LEAD - e["offset"], e["variant"]


def test_the_whole_frame_schedules_put_hits_on_the_in_call_bits_they_claim():
    for frame in H.FRAMES:
        sched = H.FFT_SCHEDULE[frame]
        assert sum(sched) * frame == H.samples_of(H.FFT(frame)) and Y.N - sum(sched) * frame < frame
        es = [e for e in entries("fft") if e["variant"][1] == frame]
        reached, last = set(), 0
        for e in es:
            for k, i, n in e["seen"]["fft_%d" % frame]:
                reached.add(i)
                last += i == n - 1
        want = {0, 1, 63, 64} | ({255, 256} if frame == 9600 else set())
        assert want <= reached and last >= 1, (frame, sorted(reached))
        p = next(e for e in es if e["name"] == "placed_%d" % frame)
        seen = p["seen"]["fft_%d" % frame]
        targets = H.PLACED_TARGETS[frame]
        assert [k for k, _, _ in seen] == [c for c, _, hold in targets for _ in range(hold)]
        assert [i for _, i, _ in seen] == [(n - 1 if idx == "last" else idx) + h for (c, idx, hold) in targets for h in range(hold)
                                           for n in [next(m for k, _, m in seen if k == c)]]
        for c, idx, hold in targets:
            assert sched[c] >= 3 and sched[c - 1] == 1 and sched[c + 1] == 1, (frame, c)  # one frame before, one frame behind
            if idx == 255:
                assert frame == 9600 and sched[c] >= 3
        # the one-frame calls hold no hit of the placed stream, and the streams of sync_cases are seen in other calls too
        assert len({k for e in es for k, _, _ in e["seen"]["fft_%d" % frame]}) >= 6


def test_the_tuned_schedule_keeps_the_seams():
    calls = H.tuned_calls()
    assert sum(calls) == Y.N and min(calls) > 0 and any(L % Y.DECIM for L in calls) and len(calls) <= 70
    reached, last = set(), 0
    for e in entries("tuned"):
        for k, i, n in e["seen"]["tuned"]:
            reached.add(i)
            last += i == n - 1
    assert set(Y.SEAM_INDICES) <= reached and last >= 3, (sorted(reached), last)
    # calls of no new bit, directly before a hit at in-call bit 0 and directly behind a hit that ends its call
    before = after = 0
    for name, t in H.TUNED:
        e = next(x for x in entries("tuned") if x["name"] == name and x["variant"][1] == t)
        nb = H.newbits(Y.BY_NAME[name], H.TUNE(t), calls)
        for k, i, n in e["seen"]["tuned"]:
            before += i == 0 and nb[k - 1] == 0
            after += i == n - 1 and k + 1 < len(nb) and nb[k + 1] == 0
    assert before >= 3 and after >= 2, (before, after)
