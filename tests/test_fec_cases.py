"""CPU: the constructed FEC blocks of tests/fec_cases.py do on the oracle what their construction claims.

Every block of every family goes through O.fec_decode (2345 blocks; about 5 s with their construction); a sample of each
family -- every 25th block, every miscorrection, the grid's corners -- also goes through the pure-Python restatement
java_restatement.FECDecode, which parses its tables out of the reference's text and so runs only where that text is present
(116 blocks, 0.1 s each: 11 s of the file's 17 s on the build machine).  tests/test_gpu_fec_forms.py sends the same blocks
through the GPU decoders.
"""
import os
import sys

import numpy as np
import pytest

import fec_cases as F
import oracle_lib as O


def distance(pay, soft):
    """symbols in which the block differs from the clean encoding of its payload"""
    return int(np.count_nonzero(O.fec_encode(pay) != (soft >> 7)))


def decode_all(rows):
    return [O.fec_decode(soft) for _, _, soft in rows]


def viterbi(soft):
    """the oracle's Viterbi decoder alone (FECDecoder.java:203-278) on a block: the 320 bytes in front of the de-scrambler"""
    sym = np.zeros(2 * F.NBITS + 68, np.uint8)
    sym[:2 * F.NBITS] = soft[F.tables()["pos"]]
    out = np.zeros(320, np.uint8)
    O.lib().jo_viterbi27(O.ptr(out), O.ptr(sym), F.NBITS)
    return out


def test_stream_encoder_equals_the_oracles():
    rng = np.random.default_rng(20261100)
    pays = [rng.integers(0, 256, 256, dtype=np.uint8) for _ in range(64)] + [np.zeros(256, np.uint8), np.full(256, 255, np.uint8)]
    for pay in pays:
        assert np.array_equal(F.symbols_of_stream(np.concatenate([pay, F.rs_parity(pay)])), O.fec_encode(pay))
        for w in range(2):
            assert not any(F.syndromes(F.codeword_of(pay, w)))  # H as fec_cases states it annihilates the encoder's words


def test_viterbi_returns_exactly_the_chosen_byte_errors():
    """a stream with byte errors behind the parity is a valid convolutional code word: on a clean channel the RS stage sees
    exactly the chosen pattern"""
    rng = np.random.default_rng(20261108)
    scr = F.tables()["scr"]
    for n0, n1 in ((0, 0), (1, 16), (16, 17), (40, 40), (160, 160)):
        pay = rng.integers(0, 256, 256, dtype=np.uint8)
        e0, e1 = F._errs(rng, n0), F._errs(rng, n1)
        s = F.errored_stream(pay, e0, e1)
        assert np.count_nonzero(s != F.stream_of(pay)) == n0 + n1
        assert np.array_equal(viterbi(F.soft_of(F.symbols_of_stream(s))) ^ scr, s)


def test_weight33_codeword_is_a_code_word_on_its_support():
    rng = np.random.default_rng(20261109)
    for support in (list(range(33)), list(range(222, 255)), [int(v) for v in rng.choice(255, 33, replace=False)]):
        d = F.weight33_codeword(support)
        assert sorted(np.flatnonzero(d)) == sorted(support)
        assert not any(F.syndromes(d))


def test_grid_decodes_up_to_16_errors_a_word_and_fails_beyond():
    rows = F.family("grid")
    assert len(rows) == 361
    for (name, pay, soft), (rc, out) in zip(rows, decode_all(rows)):
        n0, n1 = (int(v) for v in name.split("_")[1:])
        if n0 <= 16 and n1 <= 16:
            assert rc == distance(pay, soft) and np.array_equal(out, pay), (name, rc)
            assert (rc == 0) == (n0 + n1 == 0), name
        else:
            assert rc == -1, (name, rc)


def test_beyond_the_limit_fails():
    rows = F.family("beyond")
    assert len(rows) >= 200
    for (name, _, _), (rc, _) in zip(rows, decode_all(rows)):
        assert rc == -1, (name, rc)  # (a chance miscorrection, probability about 1/16!, would have to become a named case)


def test_positions_decode():
    rows = F.family("positions")
    names = [r[0] for r in rows]
    for c in F.SPECIAL_COLUMNS:
        assert f"pos_single_{c}_w0" in names and f"pos_set16_{c}_w1" in names
    assert sum(n.startswith("pos_mask_") for n in names) == 255
    for (name, pay, soft), (rc, out) in zip(rows, decode_all(rows)):
        assert rc == distance(pay, soft) and rc > 0 and np.array_equal(out, pay), (name, rc)


def test_miscorrections_are_taken_for_corrections():
    rows = F.family("miscorrections")
    assert len(rows) >= 12
    for (name, pay, soft), (rc, out) in zip(rows, decode_all(rows)):
        assert rc >= 0, name
        assert np.array_equal(out, F.MISC_EXPECTED[name]), name  # the valid word 16 symbols away, not the one sent
        assert np.array_equal(out, pay) == name.startswith("misc_p_"), name
        assert rc == distance(out, soft), name


def test_miscorrection_patches_land_in_the_padding():
    """kinds b and c: decode_rs_8 alone on the received word patches padding columns, 0 and 94 among them (FECDecoder.java:509)"""
    rng = np.random.default_rng(20261110)
    for kind, npad in (("a", 0), ("b", 8), ("c", 16)):
        pay = rng.integers(0, 256, 256, dtype=np.uint8)
        errs, d = F.miscorrection_errors(rng, kind)
        word = F.codeword_of(pay, 0)
        sent = word.copy()
        for c, m in errs.items():
            word[c] ^= m
        assert O.lib().jo_decode_rs_8(O.ptr(word), None, 0) == 16
        assert np.array_equal(word, sent ^ d)
        assert np.count_nonzero(word[:F.RSPAD]) == npad and (npad == 0 or (word[0] and word[94]))


@pytest.mark.parametrize("fam", ["chain_back_soft", "chain_back_hard"])
def test_spans_straddle_the_parallel_chain_backs_warm_up_on_blocks_that_decode(fam):
    """a span of k trellis steps costs at most (k + a few constraint lengths) / 8 bytes, half of them in each word: up to k = 200
    both words stay within 16 errors, so spans on either side of the chain-back's 128-step warm-up sit on blocks that decode"""
    rows = F.family(fam)
    ok = fail = 0
    for (name, pay, soft), (rc, out) in zip(rows, decode_all(rows)):
        if name.startswith("span_"):
            k = int(name.rsplit("_", 1)[1])
            if k <= 200:
                assert rc >= 0 and np.array_equal(out, pay), (name, rc)
        elif name.startswith("soft_value_"):
            v, sent = int(name.split("_")[2]), int(name[-1])
            assert rc == int((v >> 7) != sent) and np.array_equal(out, pay), (name, rc)
        else:
            assert name == "soft_all_128"
        ok += rc >= 0
        fail += rc < 0
    print(f"{fam}: {ok} blocks decode, {fail} fail")
    assert ok >= 100 and fail >= 30
    ks = {int(n.rsplit("_", 1)[1]) for n, _, _ in rows if n.startswith("span_")}
    assert set(range(120, 137)) <= ks and {0, 8, 400} <= ks


def test_dense_noise_straddles_the_limit():
    rows = F.family("dense")
    res = decode_all(rows)
    per = len(rows) // len(F.DENSE_RATES)
    for i, rate in enumerate(F.DENSE_RATES):
        print(f"dense {rate} %: {sum(rc >= 0 for rc, _ in res[per * i:per * (i + 1)])} of {per} decode")
    ok = sum(rc >= 0 for rc, _ in res)
    print(f"dense: {ok} decode, {len(rows) - ok} fail")
    assert ok >= 32 and len(rows) - ok >= 32
    for (name, pay, soft), (rc, out) in zip(rows, res):
        if rc >= 0 and np.array_equal(out, pay):
            assert rc == distance(pay, soft), name


def restatement_sample():
    rows = []
    for fam in F.FAMILIES:
        r = F.family(fam)
        rows += r if fam == "miscorrections" else r[::25]
    grid = {r[0]: r for r in F.family("grid")}
    rows += [grid[n] for n in ("grid_16_0", "grid_0_16", "grid_1_16", "grid_17_0", "grid_0_17", "grid_16_17", "grid_16_16")]
    return rows


def test_python_restatement_agrees_on_a_sample_of_every_family():
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    try:
        import java_restatement as R
    except FileNotFoundError:
        pytest.skip("java_restatement parses its tables out of the reference's text, which is not present here")
    rows = restatement_sample()
    assert len(rows) >= 100
    for name, _, soft in rows:
        dec = [0xEE] * 256
        rc = R.FECDecode([int(v) for v in soft], dec)
        buf = np.full(256, 0xEE, np.uint8)
        orc = O.lib().jo_fec_decode(O.ptr(np.ascontiguousarray(soft)), O.ptr(buf))
        assert rc == orc and list(buf) == dec, (name, rc, orc)  # (on failure both leave the caller's bytes, :780)
