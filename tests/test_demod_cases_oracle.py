"""CPU: the inputs of tests/test_gpu_demod_cases.py take the demod.java chain where they are meant to -- counted on the oracle
alone, before any kernel is asked (tests/demod_cases.py has the lists and the why).

1. The census, recomputed, equals tests/golden/demod_census.json, and the file regenerates byte for byte.
2. Class coverage: the frame sizes reach every tile count 1 .. 5 (fused and three-kernel), every last-tile length 1, 7, 8, 9, 20,
   21, 22 behind a full tile, odd frames whose chained tiles start off a multiple of 8, k_demod_out's chunk edges and every
   column form of k_demod_mean; the mean-block list has a lone partial block, exactly one block, a partial block of one row behind
   a full one, two blocks and a row, and more.  An edit of a list that drops a class fails here.
3. Short-call schedules: every frame size below 21 has calls shorter than 21 samples, two of them in a row, and a longer call;
   exactly 21 where the size divides 21.
4. Planted maxima: in RAW and AM with filter and mixer off the oracle's `max` after EVERY quiet frame is the planted sample's
   magnitude to the bit (AM: max + avg, and max == magnitude - avg), and every sample of the loud neighbours is larger.
5. The run-out signal: with zeros behind a frame's last sample, the filter's outputs past it exceed the frame's maximum in every
   frame -- a maximum that took in the padded lanes of a ragged tile would be another number.
6. The switch schedule: car is the same, and not zero, across the calls with the mixer off; li / lq stay through RAW and AM; the
   first frame after the filter returns differs from what a freshly cleared ring gives."""
import functools

import numpy as np

import demod_cases as D


@functools.lru_cache(maxsize=None)
def summary():
    return D.summary()


# ---------------------------------------------------------------------------------------------------------------- 1
def test_the_census_is_the_committed_one(capsys):
    got = summary()
    with capsys.disabled():
        print("\ndemod census:")
        for p in got["planted"]:
            print("   planted n=%5d mode %d: exact in %d of %d quiet frames, loud >= %.4f > %.4f" % (
                p["n"], p["mode"], p["exact"], p["quiet_frames"], p["loud_min"], p["planted"]))
        for r in got["runout"]:
            print("   run-out n=%5d: past the end / frame max >= %.1f over %d frames" % (r["n"], r["smallest_ratio"], r["frames"]))
    with open(D.CENSUS) as f:
        assert f.read() == D.dumps(got)
    assert D.load() == got


def test_the_write_entry_regenerates_the_file_byte_for_byte(tmp_path, capsys):
    with open(D.CENSUS, "rb") as f:
        want = f.read()
    assert len(want) < 16384
    D.main(["--write", str(tmp_path / "census.json")])
    assert (tmp_path / "census.json").read_bytes() == want


# ---------------------------------------------------------------------------------------------------------------- 2
def test_the_lists_cover_every_class():
    cov = D.coverage()
    assert cov["tiles"] == [1, 2, 3, 4, 5] and cov["three_kernel_tiles"] == [1, 2, 3, 4, 5]
    assert cov["last_tile_lengths"] == list(D.LAST_TILE_LENGTHS) == [1, 7, 8, 9, 20, 21, 22]
    assert cov["mean_forms"] == ["scalar", "vector", "vector+ragged"]
    assert {1, 2} <= set(cov["out_chunks"])
    assert {D.geometry(n, D.AM)["chunks"] for n in (1023, 1024, 1025)} == {1, 2} and D.geometry(1025, D.AM)["chunks"] == 2
    assert cov["odd_frames_with_ragged_chained_tiles"]  # demod_tile<*, true> at a tile start that is no multiple of 8 in the call
    # NT = 4 three times over: a 1-sample tail, a tail one short, four full tiles
    assert [D.geometry(n, D.NFM)["last"] for n in D.SIZE_LIST if D.geometry(n, D.NFM)["tiles"] == 4] == [1, 2047, 2048]
    # every size the issue lists, each once, each with a reason
    assert sorted(D.SIZE_LIST) == sorted({1, 2, 3, 7, 8, 9, 20, 21, 22, 63, 64, 65, 100, 1023, 1024, 1025, 2047, 2048, 2049, 2055,
                                          2056, 2057, 2068, 2069, 2070, 4096, 4097, 6145, 8191, 8192, 8193, 10239})
    assert len(set(D.SIZE_LIST)) == len(D.SIZE_LIST) and all(len(why) > 10 for _, why in D.SIZES)
    # the launch form: fused exactly outside AM, up to five tiles, with the knob at its default
    for n in D.SIZE_LIST + (10240, 10241, 12288):
        for mode in D.MODES:
            g = D.geometry(n, mode)
            assert g["fused"] == (mode != D.AM and n <= 5 * D.DTILE) and not D.geometry(n, mode, False)["fused"]
            assert (g["chunks"] == 0) == g["fused"] and g["mean"] == ((False, False) if mode != D.AM else g["mean"])
            assert (g["tiles"] - 1) * D.DTILE + g["last"] == n and 1 <= g["last"] <= D.DTILE
    # k_demod_mean's rows: (full blocks, rows of the partial block)
    rows = {tuple(r) for r in cov["mean_rows"]}
    assert {(0, 63), (1, 0), (1, 1), (2, 1), (3, 8)} <= rows, rows
    assert {D.mean_blocks(nin * nf) for _, nin, nf in D.MEAN_CHANNEL_BLOCKS} == {(1, 1), (2, 1)}
    assert {D.geometry(n, D.AM)["mean"] for n, _, _ in D.MEAN_BLOCKS} == {(False, True), (True, True)}
    assert D.geometry(100, D.AM)["mean"] == D.geometry(68, D.AM)["mean"] == (True, True) and D.geometry(130, D.AM)["mean"] == (False, True)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_short_frames_get_calls_below_at_and_above_the_halo():
    for n in D.SIZE_LIST:
        frames = D.calls_of(n)
        if n >= D.DHALO:
            assert frames == (2, 1, 3)
            continue
        lens = [nf * n for nf in frames]
        nshort, nfollow = D.short_calls(n)
        assert nshort > 0 and nfollow > 0, (n, lens)
        assert any(L > D.DHALO for L in lens) and min(frames) >= 1, (n, lens)
        assert (D.DHALO in lens) == (D.DHALO % n == 0), (n, lens)
        assert any(L < D.DHALO for L in lens[-1:]), (n, lens)  # a short call behind a long one as well
        assert summary()["schedules"][str(n)] == dict(frames=list(frames), short=[nshort, nfollow])
    assert D.calls_of(7) == (1, 2, 1, 3, 5, 1)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_the_planted_sample_is_the_maximum_of_every_quiet_frame():
    cases = summary()["planted"]
    assert [(c["n"], c["mode"]) for c in cases] == [(n, m) for n in D.PLANTED_SIZES for m in (D.RAW, D.AM)]
    for c in cases:
        assert c["quiet_frames"] == D.S * sum(D.PLANTED_CALLS) // 2 == 12
        assert c["exact"] == c["quiet_frames"] and c["exact_as_sum"] == c["quiet_frames"], c
        assert c["loud_min"] > c["planted"] > 0.6, c
        assert len(c["positions"]) <= c["quiet_frames"]


def test_the_planted_positions_and_the_frame_order():
    assert D.planted_positions(8) == [0, 7]
    assert D.planted_positions(2049) == [0, 2047, 2048]
    assert D.planted_positions(2056) == [0, 2047, 2048, 2055]
    assert D.planted_positions(4097) == [0, 2047, 2048, 4095, 4096]
    assert D.planted_positions(8192) == [0, 2047, 2048, 4095, 4096, 6143, 6144, 6151, 6152, 8191]
    assert D.planted_positions(10239) == [0, 2047, 2048, 4095, 4096, 6143, 6144, 8191, 8192, 8199, 8200, 10238]
    for n in D.PLANTED_SIZES:
        raws, plan = D.planted(n)
        assert {p for _, _, p, _, _ in plan} == set(D.planted_positions(n)), n  # every position is used
        fr = raws.reshape(D.S, sum(D.PLANTED_CALLS), n, 2).astype(np.int32)
        for s, f, p, i, q in plan:
            assert f % 2 == 1 and tuple(fr[s, f, p]) == (i, q)
            rest = np.delete(fr[s, f], p, axis=0)
            assert np.abs(rest).max() <= D.QUIET and np.abs(fr[s, f - 1]).min() >= D.LOUD_LO
        # the last frame of every call is quiet, the first loud: behind a call's last frame lies the next row's loud first one
        pos = 0
        for nf in D.PLANTED_CALLS:
            assert np.abs(fr[:, pos]).min() >= D.LOUD_LO and np.abs(fr[:, pos + nf - 1]).max() == D.PLANT
            pos += nf
        assert {i for _, _, _, i, _ in plan} == {D.PLANT, -D.PLANT}


# ---------------------------------------------------------------------------------------------------------------- 5
def test_the_filter_run_out_past_a_frame_exceeds_the_frame_maximum():
    for r in summary()["runout"]:
        n, total = r["n"], sum(D.calls_of(r["n"]))
        assert r["frames"] == D.S * sum(f * n >= D.DHALO for f in range(total)) >= D.S * (total - 3) and r["smallest_ratio"] > 2.0, r
    assert all(D.geometry(n, D.RAW)["last"] % D.DTILE for n in D.RUNOUT_SIZES)  # every one has a ragged last tile


# ---------------------------------------------------------------------------------------------------------------- 6
def test_the_switch_schedule_sees_a_stale_ring_and_a_resting_carrier():
    sw = summary()["switches"]
    car, lilq = sw["car_after_call"], sw["lilq_after_call"]
    cfg = [c for c, _ in D.SWITCH_CALLS]
    assert len(cfg) == len(D.SWITCH_FRAMES) == 8 and D.SWITCH_N == 2049
    assert [c[0] for c in cfg] == [D.NFM, D.NFM, D.NFM, D.NFM, D.RAW, D.AM, D.WFM, D.WFM]
    assert [c[1] for c in cfg] == [1, 0, 1, 1, 1, 1, 1, 1] and [c[2] for c in cfg] == [1, 1, 1, 0, 0, 0, 1, 1]
    assert cfg[6][3] != cfg[7][3] and sum(w for _, w in D.SWITCH_CALLS) == 1
    assert car[2] == car[3] == car[4] == car[5] != 0.0 and car[6] != car[5] and car[1] != car[2]
    assert lilq[3] == lilq[4] == lilq[5] and lilq[3] != [0.0, 0.0] and lilq[6] != lilq[5]
    assert sw["stale_ring_samples"] > 0
