"""The BPSK scope's spectra without a device: tests/bpsk_scope_spectra.py's restatement of the contract (spectra_of) against its
literal transliteration of FUNcubeBPSKDemod.java:270-327 (literal_of) on every case, frame and width, bit for bit; the column
layout; and the census that keeps the cases meaningful, held against tests/golden/bpsk_scope_spectra_census.json."""
import numpy as np
import pytest

import bpsk_scope as B
import bpsk_scope_spectra as SP


@pytest.mark.parametrize("case", list(SP.CASES))
def test_restatement_equals_the_java_text(case):
    rows = SP.run_case(case)
    for name in ("tuned", "ds"):
        for f in range(rows[name].shape[0]):
            for Wp in SP.widths(case):
                a, b = SP.spectra_of(rows[name][f], Wp), SP.literal_of(rows[name][f].reshape(-1), Wp)
                assert SP.spectra_equal(a, b), (case, name, f, Wp)
                assert a["spec"].shape == (Wp,) and a["psd"].shape == (rows[name].shape[1],)


def test_the_impulse_ties_every_bin_and_the_first_wins():
    rows = SP.run_case("impulse")
    s = SP.spectra_of(rows["tuned"][0], 749)
    assert (s["psd"] == SP.IMPULSE_X).all() and s["peak"].tolist() == [SP.IMPULSE_X, 0.0] and (s["spec"] == 100).all()
    s = SP.spectra_of(rows["tuned"][1], 749)  # (off slot 0: the bins differ in phase alone, and round apart)
    assert s["peak"][0] > 0.0


def test_silence_and_nan_rows():
    z = SP.spectra_of(np.zeros((204, 2)), 17)
    assert z["peak"].tolist() == [0.0, 0.0] and not z["spec"].any()  # ys = Infinity, 0 * Infinity = NaN -> 0
    x = np.ones((204, 2))
    x[5, 0] = np.nan
    s = SP.spectra_of(x, 17)
    assert np.isnan(s["psd"]).all() and s["peak"].tolist() == [0.0, 0.0] and not s["spec"].any()  # a NaN never wins
    assert SP.spectra_equal(s, SP.literal_of(x.reshape(-1), 17))


def test_the_layout_stays_inside_the_lower_half():
    for length in (2, 3, 64, 102, 204, 409, 819, 960, 1024, 2048, 4410, 4800, 8192, 9600):
        for Wp in (1, 2, 17, 100, 749, 1024, 2048, 4097, 32768):
            first, count = SP.layout(length, Wp)
            assert first[0] == 0 and count[0] == 0
            assert (first + np.maximum(count, 1) <= length).all() and (first + count <= length // 2 + 1).all(), (length, Wp)
    assert SP.layout(2048, 749)[1][1] == 1 and SP.layout(2048, 1024)[0][5] == 5 and SP.layout(2048, 100)[1][1] == 10
    assert SP.layout(2048, 2048)[1][1] == 0 and SP.layout(204, 749)[1][1] == 0 and SP.layout(204, 17)[0][3] == 18
    assert SP.layout(4800, 749)[1][1] == 3


def test_the_census_is_the_committed_one_and_the_cases_hold_what_they_are_for():
    c = SP.census()
    assert c == SP.load_census()
    both = [c[k][h] for k in c for h in ("t", "d")]
    for cls in ("frames_with_max_zero", "frames_with_nan", "frames_with_mo_in_upper_half", "frames_with_tied_max", "columns_at_100"):
        assert sum(x[cls] for x in both) >= 1, cls
    assert c["silence"]["t"]["frames_with_max_zero"] == c["silence"]["d"]["frames_with_max_zero"] == B.CASES["silence"]["frames"]
    assert c["nan"]["t"]["frames_with_nan"] >= 1 and c["nan"]["d"]["frames_with_nan"] >= 1
    assert c["neg_raw"]["t"]["frames_with_mo_in_upper_half"] == c["neg_raw"]["d"]["frames_with_mo_in_upper_half"] == SP.CASES["neg_raw"]["frames"]
    assert c["impulse"]["t"]["frames_with_tied_max"] >= 1
    ls = set(c["96k"]["l_values"]) | set(c["48k"]["l_values"])
    assert 0 in ls and 1 in ls and any(v >= 2 for v in ls)
    assert (c["96k"]["n"], c["96k"]["L"], c["96k"]["radices_n"], c["96k"]["radices_L"]) == (2048, 204, [], [4, 3, 17])
    assert c["r192k"]["radices_L"] == [2, 3, 17] and c["p1024"]["L"] == 102
    assert c["r48k_2048"]["radices_L"] == [409]                     # a lone prime
    assert c["p8192"]["radices_L"] == [3, 3, 7, 13]                 # a radix 13
    assert c["48k"]["radices_n"] == [4, 4, 4, 3, 5, 5] and c["44k1"]["radices_n"] == [2, 3, 3, 5, 7, 7]
