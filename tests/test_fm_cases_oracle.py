"""CPU: the schedules of tests/test_gpu_fm_cases.py take k_fm and its relatives where they are meant to -- counted from the
definitions and on the oracle alone, before any kernel is asked (tests/fm_cases.py has the lists and the why).

1. The census, recomputed, equals tests/golden/fm_census.json, and the file regenerates byte for byte.
2. Class coverage at every rate: calls of one, two and three tiles; last tiles that hold 1 .. 5 and 63, 64, 65 outputs; the saved halo
   from one tile, from exactly the last tile and from two; every alignment 0 .. 64 under the SMALL half and under the batch half, the
   two walks complete on their own; splices, a splice behind a splice; calls without output, two in a row; calls that inherit input
   history, both image overlaps; every follower behind every delta; decimation phases 0, D - 1 and one between at the seams.  An
   edit of a list that drops a class fails here.
3. geometry() against a brute-force count on EVERY call of every list, all three kinds: the call's outputs are enumerated sample by
   sample, each is given its block and tile by the definitions, and the tiles are counted.
4. The oracle over every schedule of every (rate, tuning), three streams: cut as the schedule says == in one piece (trace, bits,
   counters, state, FEC results); its dsCnt and cntDS before every call are geometry's.
5. In every seam case, each of the first 64 outputs of the call behind the seam call differs from what the oracle gives when its
   matched-filter ring is zeroed in front of that call: the halo matters in the data chosen."""
import functools

import numpy as np
import pytest

import fm_cases as F
import oracle_lib as O

CKEYS = ("cntRaw", "cntDS", "cntBit", "cntFEC", "cntDec", "dmErrBits", "dmCorr", "dmMaxCorr", "decodeOK")
STATE = [i for i in range(18) if i not in (6, 7)]  # (avePeakPower, aveCentreBin: live in FFT-acquire only)


@functools.lru_cache(maxsize=None)
def summary():
    return F.summary()


# ---------------------------------------------------------------------------------------------------------------- 1
def test_the_census_is_the_committed_one():
    got = summary()
    with open(F.CENSUS) as f:
        assert f.read() == F.dumps(got)
    assert F.load() == got


def test_the_write_entry_regenerates_the_file_byte_for_byte(tmp_path, capsys):
    with open(F.CENSUS, "rb") as f:
        want = f.read()
    assert len(want) < 16384
    F.main(["--write", str(tmp_path / "census.json")])
    assert (tmp_path / "census.json").read_bytes() == want


# ---------------------------------------------------------------------------------------------------------------- 2
def test_the_lists_cover_every_class():
    s = summary()
    assert [r["rate"] for r in s["rates"]] == list(F.RATES) and {c[0] for c in s["configs"]} == set(F.RATES)
    assert [r["D"] for r in s["rates"]] == [10, 20, 5, 4] and [F.job(r) for r in F.RATES] == [4, 4, 4, 5]
    for r in s["rates"]:
        c = r["counts"]
        assert set(r["tiles"]) == {"1", "2", "3"} and min(r["tiles"].values()) >= 40, r["tiles"]
        assert set(r["last_tile_fill"]) == {"1", "2", "3", "4", "5", "63", "64", "65"} and min(r["last_tile_fill"].values()) >= 10
        assert r["alignments_small"] == r["alignments_batch"] == F.BLOCK == 65 and r["walk_small"] and r["walk_batch"]
        assert c["splices"] >= 100 and c["splice_behind_a_splice"] > 0 and c["halo_from_two_tiles"] >= 20 and c["halo_exactly_the_last_tile"] == 10
        assert c["zero_output_calls"] >= 3 and c["zero_output_calls_in_a_row"] >= 2
        assert c["inherit"] > 0 and c["overlap_1"] > 0 and c["overlap_2"] > 0 and c["overlap_0"] > 0
        assert set(r["follow"]) == {"1", "63", "64", "65"} and min(r["follow"].values()) >= 20 and sum(r["follow"].values()) == 100
        assert r["seam_phases"] == sorted({0, r["D"] - 1, r["D"] // 2}) and len(r["seam_phases"]) == 3
        assert c["samples"] // r["D"] <= F.BUDGET * c["schedules"]
        assert r["split"]["matched:1"] == 10 and r["split"]["matched:2"] == 5  # delta -1, 0 stay in one tile of 4160, +1 opens a second
    # every delta of the cross meets every follower, and both DC forms
    for rate in F.RATES:
        cases = F.seam_cases(rate)
        assert [k for k, _ in cases] == [(a, k, d) for a in F.SEAM_A for k in F.SEAM_K for d in F.SEAM_DELTA] and len(cases) == 100
        for d in F.SEAM_DELTA:
            follow = {g["nds"] for (_, _, dd), sch in cases if dd == d for call, _, g in F.walk(sch) if call.role == "follow"}
            assert follow == set(F.FOLLOW) == {1, 63, 64, 65}, (rate, d, follow)
            assert {(sch.ic, sch.qc) for (_, _, dd), sch in cases if dd == d} == set(F.DCS[:2])
        for (a, k, d), sch in cases:
            roles = [c.role for c in sch.calls]
            assert roles == ["prep", "seam", "follow", "two"], roles
            (_, _, g), (_, _, gf), (_, _, g2) = F.walk(sch)[1:]
            assert g["a"] == a and g["nds"] == F.TILE * k - a + d and g["ntiles"] == k + (d >= 1), (rate, a, k, d, g)
            assert g["last"] == (d if d >= 1 else F.TILE + d - (a if k == 1 else 0)) and g["first"] == F.TILE - a + min(d, 0) * (k == 1)
            assert g["halo_tiles"] == ([k - 1, k] if 1 <= d < 64 else [k] if d >= 64 else [k - 1]), (a, k, d, g)
            assert gf["small"] and gf["splice"] == (gf["nds"] < 64) and g2["ntiles"] == 2 and not g2["small"]
    # the short lengths the images and the history turn on, each with its reason, under every DC form
    assert list(F.SHORT_LIST) == [1, 2, 25, 26, 27, 56, 57, 58, 60, 61, 87, 88, 89, 127, 128, 129, 255, 256, 257]
    assert all(len(why) > 5 for _, why in F.SHORT_L) and len(F.DCS) == 4 and F.DCS[0] == (0, 0)
    for rate in F.RATES:
        for dc in F.DCS:
            for sch, L in zip(F.short_schedules(rate, dc), F.SHORT_LIST):
                roles = [c.role for c in sch.calls if c.L == L]
                assert {"short-first", "short-short", "short-long"} <= set(roles) and sch.calls[0].L == L and (sch.ic, sch.qc) == dc
        assert [c.L for c in F.zero_schedule(rate).calls[:3]] == [1, 1, 1]
        assert [g["nds"] for c, _, g in F.walk(F.boundary_schedule(rate)) if c.role == "boundary"] == [511, 512, 513] * 2
        assert [g["a"] for c, _, g in F.walk(F.boundary_schedule(rate)) if c.role == "boundary"] == [0] * 3 + [64] * 3
        assert [g["small"] for c, _, g in F.walk(F.boundary_schedule(rate)) if c.role == "boundary"] == [True, True, False] * 2
        # the walks: lengths that are no multiples of D
        for sch in F.walk_schedules(rate):
            assert all(c.L % F.decim(rate) for c in sch.calls if c.role == "walk"), sch.name


# ---------------------------------------------------------------------------------------------------------------- 3
def brute(rate, n_in, L):
    """the call by enumeration: every sample, every output, every output's block and tile"""
    D = rate // 9600
    R = 5 if D == 4 else 4
    before = sum(1 for _ in range(D - 1, n_in, D))          # outputs of the stream so far: the first new output's number
    n = np.arange(n_in, n_in + L, dtype=np.int64)
    at = n[n % D == D - 1]                                   # the samples that complete an output
    g = before + np.arange(at.size)
    t0 = before
    while t0 % 65 != 64:                                     # the block boundary at or before g_first (-1 for a new stream)
        t0 -= 1
    out = dict(D=D, R=R, dsCnt=n_in - before * D, first_out=int(at[0] - n_in) if at.size else D - 1 - (n_in - before * D),
               g_first=before, nds=int(at.size), a=before - t0, tile0=t0)
    j = np.arange(at.size)
    for kind, span in (("fm", 4030), ("m", 4160)):
        tile = (g - t0) // span
        cnt = np.bincount(tile) if at.size else np.zeros(0, np.int64)
        out[kind] = dict(ntiles=int(cnt.size), first=int(cnt[0]) if cnt.size else 0, last=int(cnt[-1]) if cnt.size else 0,
                         halo_tiles=sorted(set(tile[-64:].tolist())))
        assert cnt.size == 0 or cnt.min() > 0
    out["waves"] = len(set((j // (64 * R)).tolist()))
    out["wgs"] = len(set((j // 256).tolist()))
    return out


def check_geometry(sch):
    for call, n_in, g in F.walk(sch):
        b = brute(sch.rate, n_in, call.L)
        where = (sch.name, sch.rate, n_in, call)
        for k in ("D", "R", "dsCnt", "first_out", "g_first", "nds", "a", "tile0"):
            assert g[k] == b[k], (where, k, g[k], b[k])
        assert (g["ntiles"], g["halo_tiles"]) == (b["fm"]["ntiles"], b["fm"]["halo_tiles"]), (where, g, b)
        assert (g["first"], g["last"]) == (b["fm"]["first"], b["fm"]["last"]), (where, g, b)
        assert g["small"] == (0 < b["nds"] <= 512) and g["splice"] == (0 < b["nds"] < 64)
        assert g["inherit"] == (call.L < 26) and g["overlap"] == (call.L < 256) + (call.L < 128)
        sp, ch = F.geometry(sch.rate, n_in, call.L, "split"), F.geometry(sch.rate, n_in, call.L, "chan")
        assert sp["mtiles"] == ch["mtiles"] == b["m"]["ntiles"] and sp["waves"] == b["waves"] and ch["wgs"] == b["wgs"], (where, sp, ch, b)
        assert sp["mlast"] == ch["mlast"] == b["m"]["last"], (where, sp, b)


@pytest.mark.parametrize("rate", F.RATES)
def test_geometry_is_the_brute_force_count_on_every_call(rate):
    ncalls = 0
    for sch in F.all_schedules(rate) + [s for _, s in F.split_seam_cases(rate)]:
        check_geometry(sch)
        ncalls += len(sch.calls)
    assert ncalls >= 1096 + 4 * 24


# ---------------------------------------------------------------------------------------------------------------- 4, 5
def snapshot(o):
    return dict(trace=o.trace().tobytes(), bits=o.bits().tobytes(), counters=[o.counters()[k] for k in CKEYS],
                state=o.state()[STATE].tobytes(), fec=[(rc, data.tobytes()) for rc, _, data in o.fec_results()])


def run_oracles(rate, tuning, sch):
    """-> sliced bits of the schedule's DBPSK stream"""
    raws = F.streams(rate, tuning, sch)
    total = raws.shape[1] // 2
    seam = sch.calls[1].role == "seam" if len(sch.calls) > 1 else False
    nbits = 0
    for s in range(F.S):
        cut, whole = (O.Bpsk(rate=rate, tuning=tuning, blen=1, size=1, trace=total // F.decim(rate) + 8) for _ in range(2))
        lost = O.Bpsk(rate=rate, tuning=tuning, blen=1, size=1, trace=total // F.decim(rate) + 8) if seam else None
        for call, n_in, g in F.walk(sch):
            ist = cut.istate()
            assert ist[1] == g["dsCnt"] and cut.counters()["cntDS"] == g["g_first"], (sch.name, n_in, ist, g)
            chunk = raws[s, 2 * n_in:2 * (n_in + call.L)]
            cut.receive_i16(chunk, sch.ic, sch.qc)
            if seam and call.role in ("prep", "seam", "follow"):
                if call.role == "follow":
                    lost.clear_dm_history()
                    n0 = cut.counters()["cntDS"] - g["nds"]
                lost.receive_i16(chunk, sch.ic, sch.qc)
                if call.role == "follow":
                    m = min(g["nds"], 64)
                    a, b = cut.trace()[n0:n0 + m], lost.trace()[n0:n0 + m]
                    assert a.shape == b.shape == (m, 2) and np.all((a != b).any(axis=1)), (sch.name, s, "the halo does not matter", m)
                    assert np.array_equal(cut.trace()[:n0], lost.trace()[:n0])
                    if g["nds"] > 64:  # (and nothing behind the 64 outputs that reach into it)
                        assert np.array_equal(cut.trace()[n0 + 64:], lost.trace()[n0 + 64:])
        whole.receive_i16(raws[s], sch.ic, sch.qc)
        assert snapshot(cut) == snapshot(whole), (sch.name, s)
        assert cut.counters()["cntRaw"] == total and len(cut.trace()) == total // F.decim(rate)
        if s == 0:
            nbits = len(cut.bits())
    return nbits


@pytest.mark.parametrize("rate,tuning", F.CONFIGS)
def test_the_oracle_cut_as_scheduled_is_the_oracle_in_one_piece_and_the_halo_matters(rate, tuning):
    bits = {sch.name: run_oracles(rate, tuning, sch) for sch in F.all_schedules(rate) + [s for _, s in F.split_seam_cases(rate)]}
    # bits are sliced over every schedule that is long enough for a few (8 outputs a bit)
    assert all(n > 50 for name, n in bits.items() if not name.startswith(("short", "zero"))), bits
    assert sum(bits.values()) > 100000
